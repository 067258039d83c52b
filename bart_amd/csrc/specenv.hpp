// The display quantity of model spectra on the device and the posterior spectrum / band-flux envelope on top of it
// (specenv.hip; the arithmetic is specenv_core.hpp's, the selection quant.hpp's).  The scratch is the engine's and
// serves one call at a time (scratch.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "specenv_core.hpp"

namespace bartrt {

// the kept output columns one workgroup of spec_display owns at most (fewer where the staged window of a large stride
// would not fit the LDS: spec_tile_out); the result does not depend on it
constexpr int kSpecTileOut = 256;
int spec_tile_out(int r, long stride);

// spec[nrows][ld] (nwave <= ld samples read), sflux[nwave] or null -> out[nrows][ldo] (Wk = ceil(nwave / stride)
// columns written), all device memory, asynchronous on st; half[0..r] host.  The arguments are the caller's to check.
void spectrum_display_dev(const double *d_spec, long nrows, int nwave, long ld, const double *d_sflux, double rprs, int r,
                          const double *half, long stride, double *d_out, long ldo, hipStream_t st);
// params[nsamples][npars] through the step (step_run_dev, no carry-over) in chunks of posterior_set_chunk rows; every
// chunk's spectra go through spec_display into one [nsamples][Wk] matrix in HBM, its band fluxes into [nsamples][F];
// status == 0 is the mask.  env_spec[nq][Wk], env_band[nq][F] the percentiles q, status[nsamples], *ngood.  No
// accepted sample: NaN rows.  sflux[Wfull] (host) or null.
void posterior_spectrum(Engine &e, const double *params, long nsamples, int npars, int nq, const double *q,
                        const double *sflux, int r, const double *half, long stride, double *env_spec, double *env_band,
                        int *status, long *ngood);
// the order statistics behind the latest envelope: ranks[2 nq], order_spec[2 nq][Wk], order_band[2 nq][F]; false when
// there is none (no call yet, or no accepted sample) or the shape is another
bool posterior_spectrum_order(const Engine &e, int nq, long Wk, int F, long *ranks, double *order_spec, double *order_band);
// rows [row0, row0 + nrows) of the latest sample matrix -> out[nrows][Wk] (host); false when there is no matrix or
// the range is outside it.  Waits.
bool posterior_spectrum_rows(Engine &e, long row0, long nrows, double *out);
long posterior_spectrum_cols(const Engine &e);   // Wk of the latest matrix, 0 without one
void specenv_release(Engine &e);

}  // namespace bartrt
