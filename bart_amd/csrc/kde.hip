// Gaussian kernel density estimates of selected columns of a row-major matrix on a grid per column (kde.hpp).  The
// rule -- which rows count, the order of the moments and of the sums, the bandwidth, the normalisation -- is
// kde_core.hpp's; here are the kernels that run it over a matrix in HBM, their scratch and the host drivers.
//
// MOMENTS.  kde_leaf runs one lane per (leaf, column), kde_merge one per (tile, column) over the tile's leaves, kde_fold
// one per column over the tiles of a round in ascending order into the column's running quad: the shape of mcmc_gr_leaf
// and mcmc_gr_merge with one level more, so that the serial part walks tiles, not leaves.  kde_stat makes n, mean, std
// and h of it.
//
// SUMS.  The work is nrows x ngrid exponentials per column and nothing else, so LANES ARE GRID POINTS: a workgroup of
// kde_sum owns (a tile, a column, kSumThreads neighbouring grid points), stages the tile's values of that column in LDS
// once (NaN for a row that does not count) and every lane walks them in row order with exp_rt -- all lanes read the
// same LDS address in the same step, a broadcast without a bank conflict, and no lane waits for another: no reduction
// across lanes, no atomics.  Each lane leaves its tile's sum in part[tile of the round][column][grid point]; kde_add,
// one lane per (column, grid point), adds a round's tile sums in ascending order to the running sum, and kde_finish
// normalises.  Had lanes been rows, every grid point would have needed a reduction over lanes whose order is a launch
// shape.
//
// ROUNDS.  The partials of all tiles of 2^31 - 1 rows do not fit a scratch, so the tiles are taken in rounds of as
// many as kKdeChunkBytes hold (or kde_set_chunk allows).  Both folds continue a running value in ascending order, so a
// round boundary is no boundary of the arithmetic: the rounds are invisible in the result, and so are the host form's
// upload chunks, which are whole tiles.
#include "kde.hpp"

#include <cstring>

#include "kernels.hpp"
#include "scratch.hpp"

namespace bartrt {

namespace {

static_assert(kde::kArgMin == kExpMin, "the density drops what exp_rt's range ends at");
static_assert(hist::kMaxSel <= 64, "one lane per column in kde_start, kde_fold and kde_stat");

constexpr int kThreads = 256;
constexpr int kSumThreads = 128;      // grid points of one workgroup of kde_sum: two waves share a staged tile
constexpr int kColLanes = 64;

using u64 = unsigned long long;

struct ExpRt {
  __device__ double operator()(double a) const { return exp_rt(a); }
};

__global__ void kde_start(const double *__restrict__ x, int nsel, const int *__restrict__ cols, double *__restrict__ ref,
                          double *__restrict__ run) {
  const int s = threadIdx.x;
  if (s >= nsel) return;
  ref[s] = kde::reference(x, cols[s]);
  kde::clear_quad(run + (size_t)s * kde::kQuad);
}

// leaf[nleaves][nsel][4] of the nrows rows at x
__global__ __launch_bounds__(kThreads) void kde_leaf(const double *__restrict__ x, long nrows, long ld,
                                                     const unsigned char *__restrict__ ok, int nsel,
                                                     const int *__restrict__ cols, const double *__restrict__ ref,
                                                     double *__restrict__ leaf) {
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= kde::leaves(nrows) * nsel) return;
  const int s = (int)(idx % nsel);
  const long r0 = idx / nsel * kde::kMomentRows, r1 = r0 + kde::kMomentRows < nrows ? r0 + kde::kMomentRows : nrows;
  kde::leaf(x, ld, ok, r0, r1, cols[s], ref[s], leaf + (size_t)idx * kde::kQuad);
}

// tile[ntiles][nsel][4]: each tile's leaves merged in ascending order
__global__ __launch_bounds__(kThreads) void kde_merge(const double *__restrict__ leaf, long nleaves, int nsel, long ntiles,
                                                      double *__restrict__ tile) {
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= ntiles * nsel) return;
  const int s = (int)(idx % nsel);
  const long l0 = idx / nsel * kde::kLeavesPerTile, l1 = l0 + kde::kLeavesPerTile < nleaves ? l0 + kde::kLeavesPerTile : nleaves;
  kde::merge_leaves(leaf + (size_t)s * kde::kQuad, (size_t)nsel * kde::kQuad, l0, l1, tile + (size_t)idx * kde::kQuad);
}

// the round's tiles merged in ascending order into the columns' running quads
__global__ void kde_fold(const double *__restrict__ tile, long ntiles, int nsel, double *__restrict__ run) {
  const int s = threadIdx.x;
  if (s >= nsel) return;
  double q[kde::kQuad];
  for (int i = 0; i < kde::kQuad; i++) q[i] = run[(size_t)s * kde::kQuad + i];
  for (long k = 0; k < ntiles; k++) kde::merge_into(q, tile + ((size_t)k * nsel + s) * kde::kQuad);
  for (int i = 0; i < kde::kQuad; i++) run[(size_t)s * kde::kQuad + i] = q[i];
}

__global__ void kde_stat(const double *__restrict__ run, const double *__restrict__ ref, int nsel, int rule, double factor,
                         double *__restrict__ stat, u64 *__restrict__ nonfinite) {
  const int s = threadIdx.x;
  if (s >= nsel) return;
  kde::finish_moments(run + (size_t)s * kde::kQuad, ref[s], rule, factor, stat + (size_t)s * 4);
  nonfinite[s] = (u64)run[(size_t)s * kde::kQuad + 3];
}

// part[tiles of the round][nsel][ngrid]: workgroup (tile, column, block of grid points)
__global__ __launch_bounds__(kSumThreads) void kde_sum(const double *__restrict__ x, long nrows, long ld,
                                                       const unsigned char *__restrict__ ok, int nsel,
                                                       const int *__restrict__ cols, int ngrid,
                                                       const double *__restrict__ grid, const double *__restrict__ stat,
                                                       double *__restrict__ part) {
  __shared__ double v[kde::kKdeTileRows];
  const int t = threadIdx.x, s = blockIdx.y;
  const long k = blockIdx.x, r0 = k * kde::kKdeTileRows;
  const int n = (int)(nrows - r0 < kde::kKdeTileRows ? nrows - r0 : kde::kKdeTileRows);
  const int j = blockIdx.z * kSumThreads + t;
  double *out = part + ((size_t)k * nsel + s) * ngrid;
  const double h = stat[(size_t)s * 4 + 3];
  if (!(h == h)) {                         // a degenerate column (uniform in the workgroup): kde_finish writes NaN
    if (j < ngrid) out[j] = 0.0;
    return;
  }
  const long col = cols[s];
  for (int i = t; i < n; i += kSumThreads) v[i] = kde::staged(x, ld, ok, r0 + i, col);
  __syncthreads();
  if (j >= ngrid) return;
  out[j] = kde::tile_sum(v, n, grid[(size_t)s * ngrid + j], 1.0 / h, ExpRt());
}

// acc[nq] continued by the round's tile sums in ascending order
__global__ __launch_bounds__(kThreads) void kde_add(const double *__restrict__ part, long ntiles, int nq,
                                                    double *__restrict__ acc) {
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= nq) return;
  double a = acc[q];
  for (long k = 0; k < ntiles; k++) a = a + part[(size_t)k * nq + q];
  acc[q] = a;
}

__global__ __launch_bounds__(kThreads) void kde_finish(const double *__restrict__ acc, const double *__restrict__ stat,
                                                       int ngrid, int nq, double *__restrict__ pdf) {
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= nq) return;
  pdf[q] = kde::normalised(acc[q], stat + (size_t)(q / ngrid) * 4);
}

// The calls' scratch (scratch.hpp: the reuse rule), a sibling of hist.hip's: no engine, the device that was current
// when it was made.  chunk_rows is kde_set_chunk's; slab_rows is not used.
struct KdeState : Scratch {
  PinBuf<double> h_grid;
  PinBuf<int> h_cols;
  DevBuf<int> cols;
  DevBuf<double> grid, ref, run, leaf, tile, part, acc, stat, pdf;
  DevBuf<u64> nonfinite;
};

KdeState *g_state = new KdeState;       // (never freed at exit: no HIP call from a static destructor)

// the state, ready for a new call on the current device: the host waits for the previous call, whose copies read the
// pinned staging memory this one rewrites
KdeState &begin(int nsel, int ngrid, const int *cols, const double *grid, hipStream_t st) {
  KdeState &h = on_current_device(g_state);
  h.wait();
  const size_t ng = (size_t)nsel * ngrid;
  h.h_cols.reserve(hist::kMaxSel);
  h.cols.reserve(hist::kMaxSel);
  h.h_grid.reserve(ng);
  h.grid.reserve(ng);
  h.ref.reserve(hist::kMaxSel);
  h.run.reserve((size_t)hist::kMaxSel * kde::kQuad);
  h.acc.reserve(ng);
  std::memcpy(h.h_cols.get(), cols, sizeof(int) * nsel);
  std::memcpy(h.h_grid.get(), grid, sizeof(double) * ng);
  HIPCHK(hipMemcpyAsync(h.cols, h.h_cols, sizeof(int) * nsel, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h.grid, h.h_grid, sizeof(double) * ng, hipMemcpyHostToDevice, st));
  return h;
}

long whole_tiles(long rows) { return kde::tiles(rows) * kde::kKdeTileRows; }

// tiles of one round: what kKdeChunkBytes hold of the larger of the two passes' partials, kde_set_chunk's at most
long round_tiles(const KdeState &h, int nsel, int ngrid) {
  const long moments = (long)sizeof(double) * kde::kQuad * nsel * (kde::kLeavesPerTile + 1);
  const long sums = (long)sizeof(double) * nsel * ngrid;
  long t = std::max<long>(1, kKdeChunkBytes / std::max(moments, sums));
  if (h.chunk_rows > 0) t = std::min(t, kde::tiles(h.chunk_rows));
  return t;
}

unsigned blocks(long lanes) { return (unsigned)((lanes + kThreads - 1) / kThreads); }

void start(KdeState &h, const double *d_x, int nsel, hipStream_t st) {
  hipLaunchKernelGGL(kde_start, dim3(1), dim3(kColLanes), 0, st, d_x, nsel, h.cols.get(), h.ref.get(), h.run.get());
  HIPCHK(hipGetLastError());
}

// the running quads continued by d_x's nrows rows, which begin at a tile's first row
void moments_pass(KdeState &h, const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, int ngrid,
                  hipStream_t st) {
  const long rows = round_tiles(h, nsel, ngrid) * kde::kKdeTileRows;
  h.leaf.reserve((size_t)kde::leaves(std::min(rows, whole_tiles(nrows))) * nsel * kde::kQuad);
  h.tile.reserve((size_t)kde::tiles(std::min(rows, nrows)) * nsel * kde::kQuad);
  for (long off = 0; off < nrows; off += rows) {
    const long n = std::min(rows, nrows - off), nl = kde::leaves(n), nt = kde::tiles(n);
    hipLaunchKernelGGL(kde_leaf, dim3(blocks(nl * nsel)), dim3(kThreads), 0, st, d_x + (size_t)off * ld, n, ld,
                       d_ok ? d_ok + off : nullptr, nsel, h.cols.get(), h.ref.get(), h.leaf.get());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(kde_merge, dim3(blocks(nt * nsel)), dim3(kThreads), 0, st, h.leaf.get(), nl, nsel, nt, h.tile.get());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(kde_fold, dim3(1), dim3(kColLanes), 0, st, h.tile.get(), nt, nsel, h.run.get());
    HIPCHK(hipGetLastError());
  }
}

void stat_of(KdeState &h, int nsel, int ngrid, int rule, double factor, double *d_stat, u64 *d_nonfinite, hipStream_t st) {
  hipLaunchKernelGGL(kde_stat, dim3(1), dim3(kColLanes), 0, st, h.run.get(), h.ref.get(), nsel, rule, factor, d_stat,
                     d_nonfinite);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(h.acc, 0, sizeof(double) * nsel * ngrid, st));     // (+0.0)
}

// the running sums continued by d_x's nrows rows, which begin at a tile's first row
void sums_pass(KdeState &h, const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, int ngrid,
               const double *d_stat, hipStream_t st) {
  const long rows = round_tiles(h, nsel, ngrid) * kde::kKdeTileRows;
  const int nq = nsel * ngrid;
  h.part.reserve((size_t)kde::tiles(std::min(rows, nrows)) * nq);
  for (long off = 0; off < nrows; off += rows) {
    const long n = std::min(rows, nrows - off), nt = kde::tiles(n);
    hipLaunchKernelGGL(kde_sum, dim3((unsigned)nt, (unsigned)nsel, (unsigned)((ngrid + kSumThreads - 1) / kSumThreads)),
                       dim3(kSumThreads), 0, st, d_x + (size_t)off * ld, n, ld, d_ok ? d_ok + off : nullptr, nsel,
                       h.cols.get(), ngrid, h.grid.get(), d_stat, h.part.get());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(kde_add, dim3(blocks(nq)), dim3(kThreads), 0, st, h.part.get(), nt, nq, h.acc.get());
    HIPCHK(hipGetLastError());
  }
}

void finish(KdeState &h, int nsel, int ngrid, const double *d_stat, double *d_pdf, hipStream_t st) {
  const int nq = nsel * ngrid;
  hipLaunchKernelGGL(kde_finish, dim3(blocks(nq)), dim3(kThreads), 0, st, h.acc.get(), d_stat, ngrid, nq, d_pdf);
  HIPCHK(hipGetLastError());
}

}  // namespace

void kde_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols, int ngrid,
             const double *grid, int rule, double factor, double *d_pdf, double *d_stat, u64 *d_nonfinite, hipStream_t st) {
  KdeState &h = begin(nsel, ngrid, cols, grid, st);
  start(h, d_x, nsel, st);
  moments_pass(h, d_x, nrows, ld, d_ok, nsel, ngrid, st);
  stat_of(h, nsel, ngrid, rule, factor, d_stat, d_nonfinite, st);
  sums_pass(h, d_x, nrows, ld, d_ok, nsel, ngrid, d_stat, st);
  finish(h, nsel, ngrid, d_stat, d_pdf, st);
  h.record(st);
}

void kde_host(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols, int ngrid,
              const double *grid, int rule, double factor, double *pdf, double *stat, u64 *nonfinite) {
  hipStream_t st = nullptr;
  KdeState &h = begin(nsel, ngrid, cols, grid, st);
  const size_t nq = (size_t)nsel * ngrid;
  h.stat.reserve((size_t)nsel * 4);
  h.nonfinite.reserve((size_t)nsel);
  h.pdf.reserve(nq);
  long width = 0;
  for (int s = 0; s < nsel; s++) width = std::max<long>(width, cols[s] + 1);
  // whole tiles per chunk: a chunk's first row is a tile's first row
  const long fit = std::max<long>(1, kKdeChunkBytes / (long)(sizeof(double) * ld) / kde::kKdeTileRows) * kde::kKdeTileRows;
  const long rows = std::min(whole_tiles(nrows), h.chunk_rows > 0 ? whole_tiles(h.chunk_rows) : fit);
  bool first = true;
  h.upload_chunks(x, nrows, ld, width, ok, rows, st, [&](const double *d_x, long n, const unsigned char *d_ok) {
    if (first) start(h, d_x, nsel, st);
    first = false;
    moments_pass(h, d_x, n, ld, d_ok, nsel, ngrid, st);
  });
  stat_of(h, nsel, ngrid, rule, factor, h.stat, h.nonfinite, st);
  h.upload_chunks(x, nrows, ld, width, ok, rows, st, [&](const double *d_x, long n, const unsigned char *d_ok) {
    sums_pass(h, d_x, n, ld, d_ok, nsel, ngrid, h.stat, st);
  });
  finish(h, nsel, ngrid, h.stat, h.pdf, st);
  HIPCHK(hipMemcpyAsync(pdf, h.pdf, sizeof(double) * nq, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(stat, h.stat, sizeof(double) * nsel * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(nonfinite, h.nonfinite, sizeof(u64) * nsel, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
}

void kde_set_chunk(long rows) { Scratch::set_rows(g_state->chunk_rows, "kde_set_chunk", rows); }
long kde_chunk() { return g_state->chunk_rows; }

}  // namespace bartrt
