// Band-averaged contribution functions and transmittance (contrib.hip): BART's post-processing
// (reference code/cf.py) on the optical depths the engine's own walk produces.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.hpp"

namespace bartrt {

enum { kCfContrib = 0, kCfTransmit = 1 };

// Filter windows on the FULL grid (the engine must not be sharded): filter f covers samples
// idx0[f] .. idx0[f] + npts[f] - 1 with the response resp[f] already interpolated onto them
// (concatenated).  Replaces an earlier setup.  Throws on bad windows.
void cf_setup(Engine &e, int nfilters, const int *idx0, const int *npts, const double *resp);
int cf_nfilters(const Engine &e);
// d_prof [n][nprof] -> d_band [n][nfilters][L] (atm layer order); d_full [n][W][L] (atm layer order)
// or null; d_ok [n] or null (flags in the module's own workspace).  Asynchronous on st.
void cf_run_dev(Engine &e, const double *d_prof, int n, int kind, double *d_band, double *d_full,
                unsigned char *d_ok, hipStream_t st);
// the same from / to host buffers (returns when the results are there); ok null: a non-finite
// profile fails the call
void cf_run_host(Engine &e, const double *prof, int n, int kind, double *band, double *full, unsigned char *ok);
// frees the engine's filter tables and workspaces (~Engine, an earlier setup's)
void cf_release(Engine &e);

}  // namespace bartrt
