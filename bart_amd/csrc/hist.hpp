// Marginal and pairwise histograms of selected columns of a row-major matrix in HBM, and their range (hist.hip; the
// rule is hist_core.hpp's).  No engine: the calls own their scratch and run on the current device.  It serves one
// call at a time: a call comes after the previous one's device work before it reuses the scratch (scratch.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "devbuf.hpp"
#include "hist_core.hpp"

namespace bartrt {

// the rows one workgroup owns.  Measured on [1e6, 9] and [1e7, 9] at 20 bins (tools/marginals_bench.py --slab; range +
// counts, device form): 16384 rows 1.41 / 4.06 ms, 8192 0.82 / 2.57, 4096 0.52 / 2.04, 2048 0.45 / 1.99, 1024 0.48 / 2.33
// -- a workgroup walks its slab serially, so large slabs leave most of the card idle at 1e6 rows (MEASUREMENTS.md)
constexpr long kHistSlabRows = 2048;
constexpr long kHistMaxSlabRows = 1l << 24;      // (LDS counts are 32-bit)
constexpr long kHistMaxRows = 0x7fffffffl;
constexpr long kHistChunkBytes = 64l << 20;      // the host forms' upload chunk, and the bin-index scratch

// d_x[nrows][ld], d_ok[nrows] or null, cols[nsel] and edges[nsel][nbins + 1] HOST arrays -> d_h1[nsel][nbins],
// d_out[nsel][3] (below, above, NaN) and, d_h2 not null, d_h2[npairs][nbins][nbins] (pairs a < b of selection
// indices, a-major, the first bin index a's).  Device memory, zeroed here, asynchronous on st.  The arguments are the
// caller's to check (capi.hip).
void marginals_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols, int nbins,
                   const double *edges, unsigned long long *d_h1, unsigned long long *d_out, unsigned long long *d_h2,
                   hipStream_t st);
// the same from and to host memory: the matrix goes up in row chunks (marginals_set_chunk), the counts add up on the
// device; waits
void marginals_host(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols, int nbins,
                    const double *edges, unsigned long long *h1, unsigned long long *out, unsigned long long *h2);
// d_lohi[nsel][2] the smallest and largest finite value of every selected column, d_nfinite[nsel] their number
void marginals_range_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols,
                         double *d_lohi, unsigned long long *d_nfinite, hipStream_t st);
void marginals_range_host(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols,
                          double *lohi, unsigned long long *nfinite);
// rows per workgroup (0: kHistSlabRows) and rows per upload chunk of the host forms (0: kHistChunkBytes' worth), for
// tests: no result depends on either
void marginals_set_slab(long rows);
long marginals_slab();
void marginals_set_chunk(long rows);
long marginals_chunk();

}  // namespace bartrt
