// Column-wise order statistics of a row-major matrix in HBM, and the posterior T(p) envelope on top of them
// (quant.hip; the arithmetic is quant_core.hpp's).  The scratch is the engine's.  It serves one call at a time: a call
// comes after the previous one's device work before it reuses the scratch (scratch.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "quant_core.hpp"

namespace bartrt {

// what one workgroup of the counting kernel owns: kQuantSlabRows consecutive rows of kQuantTileCols columns
constexpr long kQuantSlabRows = 4096;
constexpr int kQuantTileCols = 64;
constexpr long kQuantMaxRows = 0x7fffffffl;                      // the counts are 32-bit
constexpr long kQuantMaxCols = 65535l * kQuantTileCols;          // column tiles on the grid's y axis

// x[nrows][ld] (ncols <= ld columns read), ok[nrows] or null (rows with 0 do not exist), ranks[nranks] (host,
// zero-based among the rows that count) -> out[nranks][ncols], all device memory, asynchronous on st.  A rank at or
// above the number of rows that count gives NaN.  The arguments are the caller's to check (capi.hip).  slab_rows:
// the rows per workgroup (0: kQuantSlabRows); the result does not depend on it.
void colselect_dev(Engine &e, const double *d_x, long nrows, int ncols, long ld, const unsigned char *d_ok, int nranks,
                   const long *ranks, double *d_out, hipStream_t st, long slab_rows = 0);
// the same from and to host memory on the engine's own stream; waits (Engine::wait)
void colselect_host(Engine &e, const double *x, long nrows, int ncols, long ld, const unsigned char *ok, int nranks,
                    const long *ranks, double *out);
// params[nsamples][npars] through the step's converter (step_convert_dev: no carry-over) in chunks; the temperature
// rows stay in HBM as one [nsamples][L] matrix, status == 0 is the mask; env[nq][L] the percentiles q of every layer
// (atm order), status[nsamples], *ngood.  No accepted sample: NaN rows.
void posterior_tp(Engine &e, const double *params, long nsamples, int npars, int nq, const double *q, double *env,
                  int *status, long *ngood);
// the order statistics behind the latest posterior_tp's envelope: ranks[2 nq] (lo then hi of every percent) and
// order[2 nq][L]; false when there is none (no call yet, or no accepted sample) or the shape is another
bool posterior_tp_order(const Engine &e, int nq, int nlayers, long *ranks, double *order);
// rows per chunk of posterior_tp (0: the default); the envelope does not depend on it
void posterior_set_chunk(Engine &e, long rows);
long posterior_chunk(const Engine &e);   // the rows per chunk in force (the default where none is set)
// rows per workgroup of the selection (0: kQuantSlabRows), for tests: the result does not depend on it
void colselect_set_slab(Engine &e, long rows);
long colselect_slab(const Engine &e);
void quant_release(Engine &e);

}  // namespace bartrt
