// Band-averaged contribution functions and transmittance (contrib.hip): BART's post-processing
// (reference code/cf.py) on the optical depths the engine's own walk produces.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.hpp"

namespace bartrt {

enum { kCfContrib = 0, kCfTransmit = 1 };

// Filter windows on the FULL grid: filter f covers samples idx0[f] .. idx0[f] + npts[f] - 1 with the response resp[f]
// already interpolated onto them (concatenated).  The tables are built for the engine's block [lo, hi): each window
// clipped to it, the half weights at the window's true ends only, trapz(resp) of the whole window; a filter without
// a sample in the block has no entries.  Replaces an earlier setup.  Throws on bad windows.
void cf_setup(Engine &e, int nfilters, const int *idx0, const int *npts, const double *resp);
int cf_nfilters(const Engine &e);
// The two halves of a call, for a caller that runs its own collective (and for one GPU standing in for any rank
// count).  cf_partials_dev: this engine's band sums d_part [n][nfilters][L] -- layers from the top, entries added in
// tile order, not divided -- with d_full [n][W][L] of its own block, d_ok and d_over as cf_run_dev.  cf_combine_dev:
// d_slots = nranks slots of n * nfilters * L doubles, added in rank order, divided by trapz(resp), atm layer order
// into d_band [n][nfilters][L]; NaN rows where d_ok (optional) is 0.  No atomics: the bits depend on nranks only.
void cf_partials_dev(Engine &e, const double *d_prof, int n, int kind, const double *d_over, double *d_part,
                     double *d_full, unsigned char *d_ok, hipStream_t st);
void cf_combine_dev(Engine &e, const double *d_slots, int nranks, int n, const unsigned char *d_ok, double *d_band,
                    hipStream_t st);
// The calls below combine the ranks' sums themselves: an unsharded engine's only slot is a workspace; an engine with
// a communicator (sharded or not) writes its slot of the receive buffer, issues ONE in-place all-gather per chunk
// and combines the slots -- every rank makes the same call and gets the same rows; d_full is the block's own
// [n][W][L].  A sharded engine without a communicator: std::invalid_argument.
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
