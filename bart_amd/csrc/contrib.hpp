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
// Everything ONE contribution-function call is asked to do (cf_run), as RunRequest is for Engine::run: it travels by
// const reference from the entry point (capi.hip, which has validated it) into the one chunk loop; the engine keeps
// nothing of it.  Four choices -- input, overrides, destination, buffers -- and the plain outputs.
struct CfRequest {
  int n = 0;                     // walkers: profiles, or parameter rows
  int kind = kCfContrib;         // kCfContrib (eclipse geometry) or kCfTransmit
  const double *in = nullptr;    // [n][(S+1) L] profiles, or (from_params) [n][npars] rows as step_run_dev takes them
  bool from_params = false;      // `in` goes through the step's converter (step_convert_dev; after step_setup) first:
  int npars = 0;                 //   T(p), abundances, the declared radius / cloud-top / Rayleigh slots as overrides
  const double *over = nullptr;  // [n][3] or null, profile calls: each walker's radius (km), log10 cloud top (bar), Rayleigh
                                 //   value as the setters take them; NaN in a slot = the engine-wide setting
  double *out = nullptr;         // [n][nfilters][L]: band rows, atm layer order, divided by trapz(resp); or (partials)
  bool partials = false;         //   this engine's own sums, layers from the top, tile order, not divided, no collective
  double *full = nullptr;        // [n][W][L] or null: the block's own per-wavenumber values, atm layer order
  unsigned char *ok = nullptr;   // [n] or null, profile calls: 0 for a walker the preparation (or its radius) flags
  int *status = nullptr;         // [n] or null, parameter calls: 0, 1 (temperature), 2 (abundance) as the step reports
  hipStream_t stream = nullptr;  // device buffers: asynchronous on it; host buffers run on the engine's own stream
  bool host = false;             // the buffers are the host's: staged chunk by chunk, back when the call returns
};
// The one driver of bartrt_cf_batch / _over / _params, their _dev forms and bartrt_cf_partials_dev.  The walkers go
// through the per-walker workspaces in chunks that stay under BARTRT_CF_WORKSPACE_BYTES; per chunk: the input (host
// buffers: staged in; parameters: converted), the overrides, the preparation, the CF kernel, this engine's band sums,
// and -- unless rq.partials -- the ranks' sums combined: an unsharded engine's only slot is a workspace; an engine with
// a communicator (sharded or not) writes its slot of the receive buffer, issues ONE in-place all-gather per chunk and
// combines the slots -- every rank makes the same call and gets the same rows.  A sharded engine without a
// communicator serves rq.partials only (else std::invalid_argument).
// Overrides: device buffers are converted on the device and a radius that is not positive and finite flags the walker
// (ok = 0, NaN rows); host buffers are converted with the setters' own arithmetic and such a radius throws before any
// launch.  Null: exactly the launches of the call without overrides.
// Flags: the band rows of a flagged walker or a rejected sample are NaN, its rows of `full` undefined.  A host-buffer
// profile call without `ok` throws on a flagged profile; a parameter call never fails on a rejected sample.
void cf_run(Engine &e, const CfRequest &rq);
// The other half of rq.partials, for a caller that runs its own collective (and for one GPU standing in for any rank
// count): d_slots = nranks slots of n * nfilters * L doubles, added in rank order, divided by trapz(resp), atm layer
// order into d_band [n][nfilters][L]; NaN rows where d_ok (optional) is 0.  No atomics: the bits depend on nranks only.
void cf_combine_dev(Engine &e, const double *d_slots, int nranks, int n, const unsigned char *d_ok, double *d_band,
                    hipStream_t st);
// Diagnostics (bartrt_cf_get_records): what the CF kernel of the latest chunk read for one of its walkers, and the
// filter tables of the latest setup, copied to the host after a synchronisation of the module's last stream.  Host code
// only: no kernel runs.  Every buffer may be null.  Throws std::invalid_argument without a chunk (no call since the
// latest setup, or the latest call was refused) and for a walker outside it.
struct CfSeen {
  int n = 0, nf = 0, ntiles = 0, nent = 0;   // walkers of the latest chunk; the tables' shapes
  int form = 0;                              // kCfFormEclipse / kCfFormStaged / kCfFormUnstaged
  size_t lds = 0;                            // dynamic LDS bytes of the latest launch
};
enum { kCfFormEclipse = 0, kCfFormStaged = 1, kCfFormUnstaged = 2 };
struct CfReadback {
  double *coef = nullptr;   // [L][coef_stride]
  idx_t *idx = nullptr;     // [L][idx_stride]
  int *kstop = nullptr;
  unsigned char *ok = nullptr;
  double *rdlp = nullptr;   // [L]
  double *rtop = nullptr, *ds = nullptr;   // transit: [L], [chord_table_size(L)] as it lies in memory
  int *tile_ptr = nullptr, *f_ptr = nullptr, *f_ent = nullptr;   // [ntiles + 1], [nf + 1], [nent]
  double *wt = nullptr, *trapz = nullptr;                        // [nent][64], [nf]
};
CfSeen cf_seen(const Engine &e);   // (zeros without a setup)
void cf_get_records(Engine &e, int walker, const CfReadback &out);
// frees the engine's filter tables and workspaces (~Engine, an earlier setup's)
void cf_release(Engine &e);

}  // namespace bartrt
