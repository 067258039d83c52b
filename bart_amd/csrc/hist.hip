// Marginal and pairwise histograms of selected columns of a row-major matrix, and their range (hist.hpp).  The rule --
// which bin a value falls in, what counts in a pair, the keys of the range -- is hist_core.hpp's; here are the kernels
// that run it over a matrix in HBM, their scratch and the host drivers.
//
// TWO KERNELS.  Every matrix element is classified once, by hist_bin.  A workgroup owns a slab of rows and a tile of
// the selected columns; thread t reads column t % tile of row t / tile (+ a multiple of the rows a pass covers), so a
// wave's load is the neighbouring selected columns of a few consecutive rows of the matrix as it lies.  The tile's
// edges are staged in LDS and searched there (hist::classify).  The thread adds to its column's 1-D histogram in LDS
// and, when pairs are wanted, leaves the bin as a 16-bit index (hist::kNotCounted for a value out of range, a NaN or
// a masked row) in a column-major scratch [nsel][rows]; the indices of a pass go through LDS so that each column's run
// is written in one piece.  hist_pairs owns (a tile of pairs, a slab of rows): lanes along rows, it reads the two
// index columns of a pair (coalesced 2-byte loads) and adds to the pair's histogram in LDS, as many pair histograms as
// 64 kB hold.  Slab partials are added to the zeroed global histograms with 64-bit integer atomics, zero cells skipped.
//
// CONTENTION.  Lanes of a wave are consecutive rows of ONE pair in hist_pairs, so a narrow posterior sends all 64 to
// one LDS word.  The hardware serialises that correctly; to keep it from costing 64 turns, a wave whose live lanes all
// name the same cell adds their number once (count_cell).  Any other pattern goes through plain LDS atomics.
//
// ORDER.  Integer atomics only: the counts depend on no slab size, tile size, chunk or schedule.
#include "hist.hpp"

#include <cstring>

#include "scratch.hpp"

namespace bartrt {

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerPass = 4;                    // rows a thread of hist_bin takes between two barriers
constexpr size_t kBinLdsBytes = 48 * 1024;         // edges + histograms of hist_bin's column tile
constexpr size_t kPairLdsBytes = 64 * 1024;        // hist_pairs' histograms: the default limit, no static LDS beside it
static_assert(sizeof(unsigned) * hist::kMaxPairBins * hist::kMaxPairBins <= kPairLdsBytes, "one pair histogram fits");
static_assert((hist::kMaxBins + 1) * sizeof(double) + hist::kMaxBins * sizeof(unsigned) + 3 * sizeof(unsigned) <= kBinLdsBytes,
              "one column's edges and histogram fit");

using u64 = unsigned long long;

// what one column of hist_bin's tile takes in LDS
size_t bin_lds_per_col(int nbins) { return (size_t)(nbins + 1) * sizeof(double) + (size_t)(nbins + 3) * sizeof(unsigned); }

__global__ __launch_bounds__(kThreads) void hist_bin(const double *__restrict__ x, long nrows, long ld,
                                                     const unsigned char *__restrict__ ok, int nsel,
                                                     const int *__restrict__ cols, int nbins,
                                                     const double *__restrict__ edges, int tile_cols, long slab_rows,
                                                     unsigned short *__restrict__ idx, long idx_ld, u64 *__restrict__ h1,
                                                     u64 *__restrict__ out) {
  extern __shared__ double lds_bin[];      // edges [tc][nbins + 1], then counts [tc][nbins], then outside [tc][3]
  __shared__ unsigned short lds_code[kThreads * kRowsPerPass];   // [tc][G kRowsPerPass]: a pass's indices
  const int t = threadIdx.x;
  const int s0 = blockIdx.y * tile_cols;
  const int tc = nsel - s0 < tile_cols ? nsel - s0 : tile_cols;
  double *le = lds_bin;
  unsigned *lh = reinterpret_cast<unsigned *>(le + (size_t)tc * (nbins + 1));
  unsigned *lo = lh + (size_t)tc * nbins;
  for (int i = t; i < tc * (nbins + 1); i += kThreads) le[i] = edges[(size_t)s0 * (nbins + 1) + i];
  for (int i = t; i < tc * (nbins + 3); i += kThreads) lh[i] = 0u;
  __syncthreads();
  const long row0 = (long)blockIdx.x * slab_rows;
  const long row1 = row0 + slab_rows < nrows ? row0 + slab_rows : nrows;
  const int G = kThreads / tc;             // rows side by side
  const int span = G * kRowsPerPass;       // rows of a pass
  const bool mine = t < G * tc;
  const int sl = t % tc, r = t / tc;
  const double *e = le + (size_t)sl * (nbins + 1);
  const double scale = hist::guess_scale(e, nbins);
  const long col = mine ? cols[s0 + sl] : 0;
  for (long base = row0; base < row1; base += span) {
    double v[kRowsPerPass];
    bool use[kRowsPerPass];
#pragma unroll
    for (int k = 0; k < kRowsPerPass; k++) {
      const long row = base + r + (long)k * G;
      use[k] = mine && row < row1 && (!ok || ok[row]);
      v[k] = use[k] ? x[(size_t)row * ld + col] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kRowsPerPass; k++) {
      unsigned short code = hist::kNotCounted;
      if (use[k]) {
        const int b = hist::classify(v[k], e, nbins, scale);
        if (b >= 0) {
          atomicAdd(&lh[sl * nbins + b], 1u);
          code = (unsigned short)b;
        } else {
          atomicAdd(&lo[sl * 3 + (-1 - b)], 1u);
        }
      }
      if (idx && mine) lds_code[sl * span + r + k * G] = code;
    }
    if (idx) {       // (uniform)
      __syncthreads();
      for (int i = t; i < tc * span; i += kThreads) {
        const int s = i / span, rr = i % span;
        if (base + rr < row1) idx[(size_t)(s0 + s) * idx_ld + base + rr] = lds_code[i];
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int i = t; i < tc * nbins; i += kThreads)
    if (const unsigned c = lh[i]) atomicAdd(&h1[(size_t)s0 * nbins + i], (u64)c);
  for (int i = t; i < tc * 3; i += kThreads)
    if (const unsigned c = lo[i]) atomicAdd(&out[(size_t)s0 * 3 + i], (u64)c);
}

// one more in cell `cell` of h for every lane with live set; a wave whose live lanes agree on the cell adds once
__device__ inline void count_cell(unsigned *h, int cell, bool live) {
  if (!live) return;
  const int lead = __builtin_amdgcn_readfirstlane(cell);
  const u64 same = __ballot(cell == lead), all = __ballot(1);
  if (same == all) {
    if ((int)(threadIdx.x % warpSize) == __ffsll((long long)all) - 1) atomicAdd(&h[lead], (unsigned)__popcll(all));
  } else {
    atomicAdd(&h[cell], 1u);
  }
}

__global__ __launch_bounds__(kThreads) void hist_pairs(const unsigned short *__restrict__ idx, long idx_ld, long nrows,
                                                       int nsel, int nbins, long npairs, int tile_pairs, long slab_rows,
                                                       u64 *__restrict__ h2) {
  extern __shared__ unsigned lds_pair[];   // [pairs of the tile][nbins][nbins]
  const int t = threadIdx.x;
  const long p0 = (long)blockIdx.y * tile_pairs;
  const int np = (int)(npairs - p0 < tile_pairs ? npairs - p0 : tile_pairs);
  const int cells = nbins * nbins;
  for (int i = t; i < np * cells; i += kThreads) lds_pair[i] = 0u;
  __syncthreads();
  // the pair p0 = (a0, b0) of the a-major list over a < b
  int a0 = 0;
  long rem = p0;
  while (rem >= nsel - 1 - a0) {
    rem -= nsel - 1 - a0;
    a0++;
  }
  const int b0 = a0 + 1 + (int)rem;
  const long row0 = (long)blockIdx.x * slab_rows;
  const long row1 = row0 + slab_rows < nrows ? row0 + slab_rows : nrows;
  for (long base = row0; base < row1; base += kThreads) {
    const long row = base + t;
    const bool has = row < row1;
    int a = a0, b = b0;
    unsigned ia = has ? idx[(size_t)a * idx_ld + row] : hist::kNotCounted;
    for (int p = 0; p < np; p++) {
      const unsigned ib = has ? idx[(size_t)b * idx_ld + row] : hist::kNotCounted;
      const bool live = ia != hist::kNotCounted && ib != hist::kNotCounted;
      count_cell(lds_pair + (size_t)p * cells, live ? (int)(ia * nbins + ib) : 0, live);
      if (++b == nsel && p + 1 < np) {
        a++;
        b = a + 1;
        ia = has ? idx[(size_t)a * idx_ld + row] : hist::kNotCounted;
      }
    }
  }
  __syncthreads();
  for (int i = t; i < np * cells; i += kThreads)
    if (const unsigned c = lds_pair[i]) atomicAdd(&h2[(size_t)p0 * cells + i], (u64)c);
}

// keys[nsel][3]: the smallest key, the largest key and the number of the finite values
__global__ void hist_range_start(u64 *keys, int nsel) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsel) return;
  const hist::Range g;
  keys[3 * s] = g.lo;
  keys[3 * s + 1] = g.hi;
  keys[3 * s + 2] = g.n;
}

__global__ __launch_bounds__(kThreads) void hist_range(const double *__restrict__ x, long nrows, long ld,
                                                       const unsigned char *__restrict__ ok, int nsel,
                                                       const int *__restrict__ cols, long slab_rows, u64 *__restrict__ keys) {
  __shared__ u64 lk[hist::kMaxSel * 3];
  const int t = threadIdx.x;
  if (t < nsel) {
    const hist::Range g;
    lk[3 * t] = g.lo;
    lk[3 * t + 1] = g.hi;
    lk[3 * t + 2] = g.n;
  }
  __syncthreads();
  const long row0 = (long)blockIdx.x * slab_rows;
  const long row1 = row0 + slab_rows < nrows ? row0 + slab_rows : nrows;
  const int G = kThreads / nsel;
  const int s = t % nsel, r = t / nsel;
  if (t < G * nsel) {
    hist::Range g;
    const long col = cols[s];
    for (long row = row0 + r; row < row1; row += G)
      if (!ok || ok[row]) hist::range_add(g, x[(size_t)row * ld + col]);
    if (g.n) {
      atomicMin(&lk[3 * s], (u64)g.lo);
      atomicMax(&lk[3 * s + 1], (u64)g.hi);
      atomicAdd(&lk[3 * s + 2], (u64)g.n);
    }
  }
  __syncthreads();
  if (t < nsel && lk[3 * t + 2]) {
    atomicMin(&keys[3 * t], lk[3 * t]);
    atomicMax(&keys[3 * t + 1], lk[3 * t + 1]);
    atomicAdd(&keys[3 * t + 2], lk[3 * t + 2]);
  }
}

__global__ void hist_range_finish(const u64 *__restrict__ keys, int nsel, double *__restrict__ lohi, u64 *__restrict__ nfinite) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsel) return;
  const u64 n = keys[3 * s + 2];
  lohi[2 * s] = hist::range_value(keys[3 * s], n);
  lohi[2 * s + 1] = hist::range_value(keys[3 * s + 1], n);
  nfinite[s] = n;
}

// The calls' scratch (scratch.hpp: the reuse rule).  It belongs to no engine; it lives on the device that was current
// when it was made, and a call on another device starts over.
struct HistState : Scratch {
  PinBuf<double> h_edges;
  PinBuf<int> h_cols;
  DevBuf<double> edges, lohi;
  DevBuf<int> cols;
  DevBuf<unsigned short> idx;
  DevBuf<u64> keys, h1, out, h2, nfinite;
};

HistState *g_state = new HistState;     // (never freed at exit: no HIP call from a static destructor)

// the state, ready for a new call on the current device.  The host waits for the previous call: every call rewrites
// the pinned staging memory that call's copies read
HistState &begin() {
  HistState &h = on_current_device(g_state);
  h.wait();
  return h;
}

long slab_of(const HistState &h) { return h.slab_rows > 0 ? h.slab_rows : kHistSlabRows; }

// rows of one launch pair: what kHistChunkBytes hold of 16-bit indices, in whole slabs
long launch_rows(const HistState &h, int nsel) {
  const long slab = slab_of(h);
  const long fit = kHistChunkBytes / (long)(sizeof(unsigned short) * nsel);
  return fit / slab >= 1 ? fit / slab * slab : slab;
}

void stage_cols(HistState &h, int nsel, const int *cols, hipStream_t st) {
  h.h_cols.reserve(hist::kMaxSel);
  h.cols.reserve(hist::kMaxSel);
  std::memcpy(h.h_cols.get(), cols, sizeof(int) * nsel);
  HIPCHK(hipMemcpyAsync(h.cols, h.h_cols, sizeof(int) * nsel, hipMemcpyHostToDevice, st));
}

void stage_edges(HistState &h, int nsel, int nbins, const double *edges, hipStream_t st) {
  const size_t n = (size_t)nsel * (nbins + 1);
  h.h_edges.reserve(n);
  h.edges.reserve(n);
  std::memcpy(h.h_edges.get(), edges, sizeof(double) * n);
  HIPCHK(hipMemcpyAsync(h.edges, h.h_edges, sizeof(double) * n, hipMemcpyHostToDevice, st));
}

// the counts of d_x's nrows rows ADDED to d_h1, d_out and (not null) d_h2; cols and edges are staged
void accumulate(HistState &h, const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, int nbins,
                u64 *d_h1, u64 *d_out, u64 *d_h2, hipStream_t st) {
  const long slab = slab_of(h), rows = std::min(nrows, launch_rows(h, nsel));
  const long npairs = (long)nsel * (nsel - 1) / 2;
  const bool pairs = d_h2 && npairs > 0;
  if (pairs) h.idx.reserve((size_t)nsel * rows);
  const int tile_cols = (int)std::max<size_t>(1, std::min<size_t>(nsel, kBinLdsBytes / bin_lds_per_col(nbins)));
  const size_t bin_lds = (size_t)tile_cols * bin_lds_per_col(nbins);
  const size_t cell_bytes = sizeof(unsigned) * nbins * nbins;
  const int tile_pairs = pairs ? (int)std::min<long>(npairs, (long)(kPairLdsBytes / cell_bytes)) : 0;
  for (long off = 0; off < nrows; off += rows) {
    const long n = std::min(rows, nrows - off);
    const unsigned nslabs = (unsigned)((n + slab - 1) / slab);
    hipLaunchKernelGGL(hist_bin, dim3(nslabs, (unsigned)((nsel + tile_cols - 1) / tile_cols)), dim3(kThreads), bin_lds, st,
                       d_x + (size_t)off * ld, n, ld, d_ok ? d_ok + off : nullptr, nsel, h.cols.get(), nbins,
                       h.edges.get(), tile_cols, slab, pairs ? h.idx.get() : nullptr, rows, d_h1, d_out);
    HIPCHK(hipGetLastError());
    if (!pairs) continue;
    hipLaunchKernelGGL(hist_pairs, dim3(nslabs, (unsigned)((npairs + tile_pairs - 1) / tile_pairs)), dim3(kThreads),
                       (size_t)tile_pairs * cell_bytes, st, h.idx.get(), rows, n, nsel, nbins, npairs, tile_pairs, slab, d_h2);
    HIPCHK(hipGetLastError());
  }
}

void zero_counts(int nsel, int nbins, u64 *d_h1, u64 *d_out, u64 *d_h2, hipStream_t st) {
  const size_t npairs = (size_t)nsel * (nsel - 1) / 2;
  HIPCHK(hipMemsetAsync(d_h1, 0, sizeof(u64) * nsel * nbins, st));
  HIPCHK(hipMemsetAsync(d_out, 0, sizeof(u64) * nsel * 3, st));
  if (d_h2 && npairs) HIPCHK(hipMemsetAsync(d_h2, 0, sizeof(u64) * npairs * nbins * nbins, st));
}

void range_accumulate(HistState &h, const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel,
                      hipStream_t st) {
  const long slab = slab_of(h), rows = std::min(nrows, launch_rows(h, nsel));
  for (long off = 0; off < nrows; off += rows) {
    const long n = std::min(rows, nrows - off);
    hipLaunchKernelGGL(hist_range, dim3((unsigned)((n + slab - 1) / slab)), dim3(kThreads), 0, st, d_x + (size_t)off * ld, n,
                       ld, d_ok ? d_ok + off : nullptr, nsel, h.cols.get(), slab, h.keys.get());
    HIPCHK(hipGetLastError());
  }
}

void range_start(HistState &h, int nsel, const int *cols, hipStream_t st) {
  stage_cols(h, nsel, cols, st);
  h.keys.reserve((size_t)hist::kMaxSel * 3);
  hipLaunchKernelGGL(hist_range_start, dim3(1), dim3(hist::kMaxSel), 0, st, h.keys.get(), nsel);
  HIPCHK(hipGetLastError());
}

void range_finish(HistState &h, int nsel, double *d_lohi, u64 *d_nfinite, hipStream_t st) {
  hipLaunchKernelGGL(hist_range_finish, dim3(1), dim3(hist::kMaxSel), 0, st, h.keys.get(), nsel, d_lohi, d_nfinite);
  HIPCHK(hipGetLastError());
}

// the host forms' loop: row chunks (marginals_set_chunk) of the matrix up to its last selected column, through `each`
template <class F>
void upload_chunks(HistState &h, const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols,
                   hipStream_t st, F &&each) {
  long width = 0;
  for (int s = 0; s < nsel; s++) width = std::max<long>(width, cols[s] + 1);
  const long fit = std::max<long>(1, kHistChunkBytes / (long)(sizeof(double) * ld));
  h.upload_chunks(x, nrows, ld, width, ok, std::min(nrows, h.chunk_rows > 0 ? h.chunk_rows : fit), st, each);
}

}  // namespace

void marginals_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols, int nbins,
                   const double *edges, u64 *d_h1, u64 *d_out, u64 *d_h2, hipStream_t st) {
  HistState &h = begin();
  stage_cols(h, nsel, cols, st);
  stage_edges(h, nsel, nbins, edges, st);
  zero_counts(nsel, nbins, d_h1, d_out, d_h2, st);
  accumulate(h, d_x, nrows, ld, d_ok, nsel, nbins, d_h1, d_out, d_h2, st);
  h.record(st);
}

void marginals_host(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols, int nbins,
                    const double *edges, u64 *h1, u64 *out, u64 *h2) {
  HistState &h = begin();
  hipStream_t st = nullptr;
  const size_t n1 = (size_t)nsel * nbins, n2 = (size_t)nsel * (nsel - 1) / 2 * nbins * nbins;
  const bool pairs = h2 && n2;
  h.h1.reserve(n1);
  h.out.reserve((size_t)nsel * 3);
  if (pairs) h.h2.reserve(n2);
  u64 *d_h2 = pairs ? h.h2.get() : nullptr;
  stage_cols(h, nsel, cols, st);
  stage_edges(h, nsel, nbins, edges, st);
  zero_counts(nsel, nbins, h.h1, h.out, d_h2, st);
  upload_chunks(h, x, nrows, ld, ok, nsel, cols, st, [&](const double *d_x, long n, const unsigned char *d_ok) {
    accumulate(h, d_x, n, ld, d_ok, nsel, nbins, h.h1, h.out, d_h2, st);
  });
  HIPCHK(hipMemcpyAsync(h1, h.h1, sizeof(u64) * n1, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(out, h.out, sizeof(u64) * nsel * 3, hipMemcpyDeviceToHost, st));
  if (pairs) HIPCHK(hipMemcpyAsync(h2, h.h2, sizeof(u64) * n2, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
}

void marginals_range_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols,
                         double *d_lohi, u64 *d_nfinite, hipStream_t st) {
  HistState &h = begin();
  range_start(h, nsel, cols, st);
  range_accumulate(h, d_x, nrows, ld, d_ok, nsel, st);
  range_finish(h, nsel, d_lohi, d_nfinite, st);
  h.record(st);
}

void marginals_range_host(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols,
                          double *lohi, u64 *nfinite) {
  HistState &h = begin();
  hipStream_t st = nullptr;
  h.lohi.reserve((size_t)nsel * 2);
  h.nfinite.reserve((size_t)nsel);
  range_start(h, nsel, cols, st);
  upload_chunks(h, x, nrows, ld, ok, nsel, cols, st, [&](const double *d_x, long n, const unsigned char *d_ok) {
    range_accumulate(h, d_x, n, ld, d_ok, nsel, st);
  });
  range_finish(h, nsel, h.lohi, h.nfinite, st);
  HIPCHK(hipMemcpyAsync(lohi, h.lohi, sizeof(double) * nsel * 2, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(nfinite, h.nfinite, sizeof(u64) * nsel, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
}

void marginals_set_slab(long rows) { Scratch::set_rows(g_state->slab_rows, "marginals_set_slab", rows, kHistMaxSlabRows); }
long marginals_slab() { return slab_of(*g_state); }

void marginals_set_chunk(long rows) { Scratch::set_rows(g_state->chunk_rows, "marginals_set_chunk", rows); }
long marginals_chunk() { return g_state->chunk_rows; }

}  // namespace bartrt
