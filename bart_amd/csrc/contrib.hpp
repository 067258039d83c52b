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
// d_over [n][3] or null: each walker's own reference radius (km), log10 cloud-top pressure (bar) and Rayleigh value --
// what bartrt_set_radius / _set_cloudtop / _set_scattering take -- NaN in a slot = the engine-wide setting
// (prep_profiles' own sentinel, prep.hpp).  Null: exactly the launches of the call without overrides.  A radius that
// is not positive and finite: the walker is flagged (device form) / the call throws (host form).
void cf_run_dev(Engine &e, const double *d_prof, int n, int kind, double *d_band, double *d_full,
                unsigned char *d_ok, hipStream_t st, const double *d_over = nullptr);
// the same from / to host buffers (returns when the results are there); ok null: a non-finite
// profile fails the call
void cf_run_host(Engine &e, const double *prof, int n, int kind, double *band, double *full, unsigned char *ok,
                 const double *over = nullptr);
// Parameters in (after step_setup): params [n][npars] as step_run_dev takes them go through the step's converter
// (step_convert_dev: T(p), abundances, the declared radius / cloud-top / Rayleigh slots as per-walker overrides) into
// this module's workspaces, then through the records and kernels above.  status [n] or null: 0, 1 (temperature),
// 2 (abundance) as the step reports them; the band rows of a rejected sample (and of a profile the preparation
// flags) are NaN, its rows of `full` undefined.  A rejected sample does not fail the call.
void cf_params_dev(Engine &e, const double *d_params, int n, int npars, int kind, double *d_band, double *d_full,
                   int *d_status, hipStream_t st);
void cf_params_host(Engine &e, const double *params, int n, int npars, int kind, double *band, double *full,
                    int *status);
// frees the engine's filter tables and workspaces (~Engine, an earlier setup's)
void cf_release(Engine &e);

}  // namespace bartrt
