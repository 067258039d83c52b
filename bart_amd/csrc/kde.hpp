// Gaussian kernel density estimates of selected columns of a row-major matrix in HBM on a grid per column (kde.hip;
// the rule is kde_core.hpp's).  No engine: the calls own their scratch and run on the current device, one call at a
// time under scratch.hpp's reuse rule.
#pragma once
#include <hip/hip_runtime.h>

#include "devbuf.hpp"
#include "kde_core.hpp"

namespace bartrt {

constexpr long kKdeChunkBytes = 64l << 20;       // the host forms' upload chunk, and the most a round's partials take

// d_x[nrows][ld], d_ok[nrows] or null, cols[nsel] and grid[nsel][ngrid] HOST arrays, rule kde::kScott / kSilverman /
// kFactor (then factor > 0) -> d_pdf[nsel][ngrid], d_stat[nsel][4] (n, mean, std, h), d_nonfinite[nsel].  Device
// memory, asynchronous on st.  The arguments are the caller's to check (capi.hip).
void kde_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols, int ngrid,
             const double *grid, int rule, double factor, double *d_pdf, double *d_stat, unsigned long long *d_nonfinite,
             hipStream_t st);
// the same from and to host memory: the matrix goes up twice in row chunks that are whole tiles (kde_set_chunk; by
// default kKdeChunkBytes' worth or one tile, whichever is larger: a tile of ld > 4096 columns exceeds 64 MiB), first
// for the moments, then for the sums; waits
void kde_host(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols, int ngrid,
              const double *grid, int rule, double factor, double *pdf, double *stat, unsigned long long *nonfinite);
// rows per upload chunk of the host form and per round of either form, rounded up to whole tiles (0: kKdeChunkBytes'
// worth, one tile at least), for tests: no result depends on it
void kde_set_chunk(long rows);
long kde_chunk();

}  // namespace bartrt
