// Column-wise multi-rank selection on a row-major matrix, and the posterior T(p) envelope (quant.hpp).  The
// arithmetic -- keys, digits, the histogram walk, the percentile rule -- is quant_core.hpp's; here are the two kernels
// that run it over a matrix in HBM, their scratch and the host drivers.
//
// LAYOUT.  The matrix is read as it lies, row-major, lanes along columns: a wave reads 64 neighbouring columns of one
// row in one coalesced load (512 bytes), the four waves of a workgroup take every fourth row of the workgroup's slab.
// No transposed copy is made: it would double the memory of a matrix that is already the largest thing in HBM (a
// posterior of 1e6 x 100 doubles is 800 MB, the contribution-function matrix nfilters times that), and the mask test
// it saves is one byte per row, broadcast to the wave.  With lanes along columns every lane of a wave counts into its
// own column's histogram, and the histograms lie in LDS as [rank][digit][column]: the 64 lanes of one atomic add hit
// 64 consecutive words, so no two lanes of a wave share an address or a bank.  That layout is also why the digit is 4
// bits wide and not 8: 16 ranks x 16 digits x 64 columns of 32-bit counts are 64 kB of LDS, which is the default
// limit and leaves room for two workgroups per CU; 256 digits would need 1 MB, or a column tile of four lanes and
// 32-byte reads.  Sixteen passes of coalesced reads it is.
//
// SHARED PASSES.  All ranks of a column share each pass.  Ranks whose prefixes are still equal (all of them in pass 0,
// and as long as the order statistics asked for agree in their leading digits) count into ONE histogram, the one of
// the first such rank, their leader: an element is tested against the leaders' prefixes only.
//
// MERGE.  A column longer than one slab is split across workgroups; each adds its non-zero LDS counts to the global
// histogram [rank][digit][column] with integer atomics.  quant_walk, one lane per column, walks every rank's leader
// histogram (quant::walk), appends the digit, names the next pass's leaders and zeroes the histogram again.
#include "quant.hpp"

#include <limits>
#include <vector>

#include "scratch.hpp"
#include "step.hpp"

namespace bartrt {

namespace {

constexpr int kCountThreads = 256;
constexpr int kCountWaves = kCountThreads / kQuantTileCols;
constexpr int kRowUnroll = 4;
static_assert(kQuantTileCols == 64, "one wave spans a column tile");
static_assert(sizeof(unsigned) * quant::kMaxRanks * quant::kBins * kQuantTileCols <= 64 * 1024, "the histograms fit the default LDS limit");

struct RankList {
  long k[quant::kMaxRanks];
};

// the state of a selection: per (rank, column) the prefix found so far, the rank inside it and the rank's leader; per
// column the ranks still alive (bit r) and the leaders among them (bit r)
struct SelState {
  unsigned long long *prefix;   // [nranks][ncols]
  long *krem;                   // [nranks][ncols]
  unsigned char *leader;        // [nranks][ncols]
  unsigned *alive, *active;     // [ncols]
  unsigned *hist;               // [nranks][kBins][ncols], zero between passes
};

__global__ void quant_start(SelState s, int ncols, int nranks, RankList ranks) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= ncols) return;
  for (int r = 0; r < nranks; r++) {
    const size_t q = (size_t)r * ncols + col;
    s.prefix[q] = 0;
    s.krem[q] = ranks.k[r];
    s.leader[q] = 0;
  }
  s.alive[col] = nranks >= 32 ? ~0u : (1u << nranks) - 1u;
  s.active[col] = 1u;
}

// pass `pass` of the selection: the digit counts of the slab's rows that count, per leader
__global__ __launch_bounds__(kCountThreads) void quant_count(const double *__restrict__ x, long nrows, int ncols, long ld,
                                                             const unsigned char *__restrict__ ok, int nranks, int pass,
                                                             long slab_rows, SelState s) {
  extern __shared__ unsigned lds_hist[];   // [nranks][kBins][kQuantTileCols]
  const int lane = threadIdx.x % kQuantTileCols, wave = threadIdx.x / kQuantTileCols;
  const int col0 = blockIdx.y * kQuantTileCols, col = col0 + lane;
  const long row0 = (long)blockIdx.x * slab_rows;
  const long row1 = row0 + slab_rows < nrows ? row0 + slab_rows : nrows;
  const int nhist = nranks * quant::kBins * kQuantTileCols;
  for (int i = threadIdx.x; i < nhist; i += kCountThreads) lds_hist[i] = 0;
  __syncthreads();
  const bool has = col < ncols;
  const unsigned act = has ? s.active[col] : 0u;
  unsigned long long want[quant::kMaxRanks];
#pragma unroll
  for (int r = 0; r < quant::kMaxRanks; r++)
    want[r] = (has && r < nranks) ? quant::above(s.prefix[(size_t)r * ncols + col], pass) : 0ull;
  if (act) {
    for (long base = row0 + wave; base < row1; base += (long)kCountWaves * kRowUnroll) {
      unsigned long long key[kRowUnroll];
      bool use[kRowUnroll];
#pragma unroll
      for (int u = 0; u < kRowUnroll; u++) {
        const long row = base + (long)u * kCountWaves;
        use[u] = row < row1 && (!ok || ok[row]);
        key[u] = use[u] ? quant::key_of(x[(size_t)row * ld + col]) : 0ull;
      }
#pragma unroll
      for (int u = 0; u < kRowUnroll; u++) {
        if (!use[u]) continue;
        const unsigned long long hi = quant::above(key[u], pass);
        const int d = quant::digit(key[u], pass);
#pragma unroll
        for (int r = 0; r < quant::kMaxRanks; r++)
          if (((act >> r) & 1u) && hi == want[r]) atomicAdd(&lds_hist[(r * quant::kBins + d) * kQuantTileCols + lane], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nhist; i += kCountThreads) {
    const unsigned v = lds_hist[i];
    const int c = col0 + i % kQuantTileCols;
    if (v && c < ncols) atomicAdd(&s.hist[(size_t)(i / kQuantTileCols) * ncols + c], v);
  }
}

// after pass `pass`'s counts: every rank's next digit, the next leaders, the histograms zeroed; after the last pass
// the answers out[nranks][ncols]
__global__ void quant_walk(SelState s, int ncols, int nranks, int pass, double *__restrict__ out) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= ncols) return;
  unsigned alive = s.alive[col];
  const unsigned act = s.active[col];
  for (int r = 0; r < nranks; r++) {
    if (!((alive >> r) & 1u)) continue;
    const size_t q = (size_t)r * ncols + col;
    long k = s.krem[q];
    const int d = quant::walk(s.hist + (size_t)s.leader[q] * quant::kBins * ncols + col, (size_t)ncols, &k);
    if (d < 0) {
      alive &= ~(1u << r);
      continue;
    }
    s.prefix[q] = quant::append(s.prefix[q], pass, d);
    s.krem[q] = k;
  }
  for (int r = 0; r < nranks; r++)
    if ((act >> r) & 1u)
      for (int d = 0; d < quant::kBins; d++) s.hist[(size_t)(r * quant::kBins + d) * ncols + col] = 0u;
  unsigned next = 0;
  for (int r = 0; r < nranks; r++) {
    if (!((alive >> r) & 1u)) continue;
    const size_t q = (size_t)r * ncols + col;
    const unsigned long long mine = s.prefix[q];
    int lead = r;
    for (int o = 0; o < r; o++)
      if (((next >> o) & 1u) && s.prefix[(size_t)o * ncols + col] == mine) {
        lead = o;
        break;
      }
    s.leader[q] = (unsigned char)lead;
    if (lead == r) next |= 1u << r;
  }
  s.alive[col] = alive;
  s.active[col] = next;
  if (pass == quant::kPasses - 1)
    for (int r = 0; r < nranks; r++) {
      const size_t q = (size_t)r * ncols + col;
      out[q] = ((alive >> r) & 1u) ? quant::value_of(s.prefix[q]) : quant::double_of(quant::kExp | (quant::kExp >> 1));
    }
}

__global__ void quant_mask_of_status(const int *__restrict__ status, long n, unsigned char *__restrict__ ok) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ok[i] = status[i] == 0;
}

}  // namespace

// the engine's scratch of the selection and of the posterior envelope (scratch.hpp: the reuse rule, the settings)
struct QuantState : Scratch {
  DevBuf<unsigned long long> prefix;
  DevBuf<long> krem;
  DevBuf<unsigned char> leader;
  DevBuf<unsigned> alive, active, hist;
  DevBuf<double> out;    // host form of the selection
  // posterior_tp
  DevBuf<double> params, prof, temp, order;
  DevBuf<int> status;
  DevBuf<unsigned char> good;
  std::vector<long> last_ranks;
  std::vector<double> last_order;
  int last_nq = 0, last_L = 0;
};

namespace {

constexpr long kDefaultChunk = 4096;

QuantState &state_of(Engine &e) {
  if (!e.quant) e.quant = new QuantState;
  return *e.quant;
}

}  // namespace

void quant_release(Engine &e) {
  delete e.quant;
  e.quant = nullptr;
}

void colselect_dev(Engine &e, const double *d_x, long nrows, int ncols, long ld, const unsigned char *d_ok, int nranks,
                   const long *ranks, double *d_out, hipStream_t st, long slab_rows) {
  if (ncols <= 0) return;
  QuantState &q = state_of(e);
  if (slab_rows <= 0) slab_rows = q.slab_rows > 0 ? q.slab_rows : kQuantSlabRows;
  const size_t cells = (size_t)nranks * ncols;
  q.room(q.prefix, cells);
  q.room(q.krem, cells);
  q.room(q.leader, cells);
  q.room(q.alive, (size_t)ncols);
  q.room(q.active, (size_t)ncols);
  q.room(q.hist, cells * quant::kBins);
  q.after_previous(st);
  SelState s{q.prefix, q.krem, q.leader, q.alive, q.active, q.hist};
  RankList rl{};
  for (int r = 0; r < nranks; r++) rl.k[r] = ranks[r];
  const int lanes = 64;
  const dim3 per_col((ncols + lanes - 1) / lanes);
  HIPCHK(hipMemsetAsync(q.hist, 0, sizeof(unsigned) * cells * quant::kBins, st));
  hipLaunchKernelGGL(quant_start, per_col, dim3(lanes), 0, st, s, ncols, nranks, rl);
  HIPCHK(hipGetLastError());
  const dim3 grid((unsigned)((nrows + slab_rows - 1) / slab_rows), (unsigned)((ncols + kQuantTileCols - 1) / kQuantTileCols));
  const size_t sh = sizeof(unsigned) * nranks * quant::kBins * kQuantTileCols;
  for (int pass = 0; pass < quant::kPasses; pass++) {
    hipLaunchKernelGGL(quant_count, grid, dim3(kCountThreads), sh, st, d_x, nrows, ncols, ld, d_ok, nranks, pass,
                       slab_rows, s);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(quant_walk, per_col, dim3(lanes), 0, st, s, ncols, nranks, pass, d_out);
    HIPCHK(hipGetLastError());
  }
  q.record(st);
}

void colselect_host(Engine &e, const double *x, long nrows, int ncols, long ld, const unsigned char *ok, int nranks,
                    const long *ranks, double *out) {
  QuantState &q = state_of(e);
  hipStream_t st = e.stream;
  const size_t nout = (size_t)nranks * ncols;
  q.room(q.out, nout);
  // one chunk of all rows: the selection makes 16 passes over the matrix and needs it resident.  (The staging and
  // q.out are this function's alone, and it ends in a full wait: no earlier call can still be using them.)
  q.upload_chunks(x, nrows, ld, ncols, ok, nrows, st, [&](const double *d_x, long, const unsigned char *d_ok) {
    colselect_dev(e, d_x, nrows, ncols, ld, d_ok, nranks, ranks, q.out, st);
  });
  HIPCHK(hipMemcpyAsync(out, q.out, sizeof(double) * nout, hipMemcpyDeviceToHost, st));
  e.wait(st);
}

void posterior_set_chunk(Engine &e, long rows) { Scratch::set_rows(state_of(e).chunk_rows, "posterior_set_chunk", rows); }

long posterior_chunk(const Engine &e) { return e.quant && e.quant->chunk_rows > 0 ? e.quant->chunk_rows : kDefaultChunk; }

void posterior_tp(Engine &e, const double *params, long nsamples, int npars, int nq, const double *pct, double *env,
                  int *status, long *ngood) {
  QuantState &q = state_of(e);
  hipStream_t st = e.stream;
  const int L = e.L;
  const size_t nprof = (size_t)(e.S + 1) * L;
  const long chunk = std::min(nsamples, posterior_chunk(e));
  q.room(q.params, (size_t)chunk * npars);
  q.room(q.prof, (size_t)chunk * nprof);
  q.room(q.temp, (size_t)nsamples * L);
  q.room(q.status, (size_t)nsamples);
  q.room(q.good, (size_t)nsamples);
  q.room(q.order, (size_t)2 * nq * L);
  q.last_nq = 0;
  for (long off = 0; off < nsamples; off += chunk) {
    const int n = (int)std::min(chunk, nsamples - off);
    HIPCHK(hipMemcpyAsync(q.params, params + (size_t)off * npars, sizeof(double) * n * npars, hipMemcpyHostToDevice, st));
    step_convert_dev(e, q.params, n, npars, q.prof, q.status + off, nullptr, st);
    // the temperature is the first L values of a profile
    HIPCHK(hipMemcpy2DAsync(q.temp + (size_t)off * L, sizeof(double) * L, q.prof, sizeof(double) * nprof,
                            sizeof(double) * L, (size_t)n, hipMemcpyDeviceToDevice, st));
  }
  hipLaunchKernelGGL(quant_mask_of_status, dim3((unsigned)((nsamples + 255) / 256)), dim3(256), 0, st, q.status.get(),
                     nsamples, q.good.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(status, q.status, sizeof(int) * nsamples, hipMemcpyDeviceToHost, st));
  e.wait(st);
  long good = 0;
  for (long i = 0; i < nsamples; i++) good += status[i] == 0;
  *ngood = good;
  if (good == 0) {
    for (size_t i = 0; i < (size_t)nq * L; i++) env[i] = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  std::vector<long> ranks((size_t)2 * nq);
  std::vector<double> w((size_t)nq);
  for (int i = 0; i < nq; i++) quant::percentile_rule(good, pct[i], &ranks[2 * i], &ranks[2 * i + 1], &w[i]);
  colselect_dev(e, q.temp, nsamples, L, L, q.good, 2 * nq, ranks.data(), q.order, st);
  q.last_order.resize((size_t)2 * nq * L);
  HIPCHK(hipMemcpyAsync(q.last_order.data(), q.order, sizeof(double) * 2 * nq * L, hipMemcpyDeviceToHost, st));
  e.wait(st);
  for (int i = 0; i < nq; i++)
    for (int l = 0; l < L; l++)
      env[(size_t)i * L + l] = quant::interpolate(q.last_order[(size_t)(2 * i) * L + l], q.last_order[(size_t)(2 * i + 1) * L + l], w[i]);
  q.last_ranks = ranks;
  q.last_nq = nq;
  q.last_L = L;
}

bool posterior_tp_order(const Engine &e, int nq, int nlayers, long *ranks, double *order) {
  const QuantState *q = e.quant;
  if (!q || q->last_nq == 0 || q->last_nq != nq || q->last_L != nlayers) return false;
  std::copy(q->last_ranks.begin(), q->last_ranks.end(), ranks);
  std::copy(q->last_order.begin(), q->last_order.end(), order);
  return true;
}

long colselect_slab(const Engine &e) { return e.quant && e.quant->slab_rows > 0 ? e.quant->slab_rows : kQuantSlabRows; }

void colselect_set_slab(Engine &e, long rows) { Scratch::set_rows(state_of(e).slab_rows, "colselect_set_slab", rows); }

}  // namespace bartrt
