// Native driver loop of a retrieval: differential-evolution MCMC (ter Braak
// 2006; the reference's `walk = demc`) and its snooker variant (ter Braak &
// Vrugt 2008; `walk = snooker`) over all chains per iteration, one batched model
// call (step_run_host) per iteration.  Same moves, bounds and rejection rules as
// bart_amd/sampler.py (the keys of the reference's [MCMC] section,
// examples/demo/BART_eclipse.cfg:43-102); the random streams differ, so the two
// agree statistically, not draw for draw.  Host code: an iteration is a few
// hundred flops around three kernel launches, and in Python its bookkeeping
// costs as much as the launches.
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine.hpp"
#include "ess_core.hpp"
#include "gr_core.hpp"
#include "mcmc_core.hpp"
#include "retrieval_host.hpp"
#include "step.hpp"

namespace bartrt {

void mcmc_run(Engine &e, const RetrievalProblem &problem, int nch, long nsteps, const double *params, int snooker,
              unsigned long long seed, double *chain, double *chisq, long *naccept_out, long *nbad) {
  // (its own refusals, with their own error class, and its own chi-square: this loop is kept as it was)
  const int npars = problem.npars, ndata = problem.ndata;
  const double *pmin = problem.pmin, *pmax = problem.pmax, *stepsize = problem.stepsize;
  const double *data = problem.data, *uncert = problem.uncert;
  if (!e.step) throw IoError{"mcmc_run: call step_setup first"};
  if (nch < 1 || npars < 1 || nsteps < 1) throw IoError{"mcmc_run: bad sizes"};
  if (ndata != e.step->nfilters) throw IoError{"mcmc_run: data length must equal the number of filters"};
  std::vector<int> free_;
  for (int j = 0; j < npars; j++) {
    if (stepsize[j] < 0)
      throw IoError{"mcmc_run: stepsize < 0 (a shared parameter in MC3's convention) is not supported"};
    if (stepsize[j] > 0) free_.push_back(j);
  }
  const int nfree = (int)free_.size();
  std::mt19937_64 rng(seed);
  std::normal_distribution<double> normal(0.0, 1.0);
  std::uniform_real_distribution<double> unif(0.0, 1.0);
  const double inf = std::numeric_limits<double>::infinity();

  std::vector<double> band((size_t)nch * ndata), packed((size_t)nch * npars);
  std::vector<int> rows(nch), status(nch);
  if (nbad) std::fill(nbad, nbad + 4, 0L);
  // chi-square of the rows of p flagged in `use` (others: inf); a row of -1 is
  // the worker's rejection sentinel
  auto chisq_of = [&](const std::vector<double> &p, const std::vector<char> &use, std::vector<double> &out) {
    int m = 0;
    for (int i = 0; i < nch; i++) {
      out[i] = inf;
      if (!use[i]) continue;
      std::copy(p.begin() + (size_t)i * npars, p.begin() + (size_t)(i + 1) * npars,
                packed.begin() + (size_t)m * npars);
      rows[m++] = i;
    }
    if (m == 0) return;
    step_run_host(e, packed.data(), m, npars, band.data(), status.data());
    if (nbad)
      for (int k = 0; k < m; k++)
        if (status[k] >= 1 && status[k] <= 3) nbad[status[k]]++;
    for (int k = 0; k < m; k++) {
      const double *b = band.data() + (size_t)k * ndata;
      bool sentinel = true;
      double c = 0.0;
      for (int f = 0; f < ndata; f++) {
        sentinel = sentinel && b[f] == -1.0;
        const double r = (b[f] - data[f]) / uncert[f];
        c += r * r;
      }
      out[rows[k]] = sentinel ? inf : c;
    }
  };
  // the box applies to the free parameters; a fixed one keeps its configured value
  auto clip = [&](std::vector<double> &p) {
    for (int i = 0; i < nch; i++)
      for (int j : free_) {
        double &v = p[(size_t)i * npars + j];
        v = std::min(std::max(v, pmin[j]), pmax[j]);
      }
  };

  // start: the configured point jittered by the stepsizes, inside the box
  std::vector<double> x((size_t)nch * npars), prop((size_t)nch * npars), c(nch), cp(nch);
  std::vector<char> all(nch, 1), inside(nch);
  for (int i = 0; i < nch; i++)
    for (int j = 0; j < npars; j++)
      x[(size_t)i * npars + j] = params[j] + (i > 0 && stepsize[j] > 0 ? stepsize[j] * normal(rng) : 0.0);
  clip(x);
  chisq_of(x, all, c);
  for (int round = 0; round < 20; round++) {  // re-draw chains that start on a rejected model
    bool any_bad = false;
    for (int i = 0; i < nch; i++)
      if (!std::isfinite(c[i])) {
        any_bad = true;
        for (int j = 0; j < npars; j++)
          x[(size_t)i * npars + j] = params[j] + (stepsize[j] > 0 ? 0.1 * stepsize[j] * normal(rng) : 0.0);
      }
    if (!any_bad) break;
    clip(x);
    chisq_of(x, all, c);
  }
  if (std::none_of(c.begin(), c.end(), [](double v) { return std::isfinite(v); }))
    throw IoError{"mcmc_run: no chain starts on a physical model: check params/pmin/pmax"};

  auto other = [&](int i, int a, int b) {  // uniform over the chains other than i, a, b (a, b < 0: unused)
    int ex[3] = {i, a, b}, k = 1 + (a >= 0) + (b >= 0);
    std::sort(ex, ex + 3);                 // unused entries (-1) sort first
    int draw = (int)(unif(rng) * (nch - k));
    if (draw >= nch - k) draw = nch - k - 1;
    for (int q = 3 - k; q < 3; q++) draw += draw >= ex[q];
    return draw;
  };
  const double gamma0 = 2.38 / std::sqrt(2.0 * std::max(nfree, 1));
  const bool do_snooker = snooker && nch > 3;
  long naccept = 0;
  std::vector<double> logjac(nch);
  for (long t = 0; t < nsteps; t++) {
    prop = x;
    for (int i = 0; i < nch; i++) {
      const int r1 = nch > 1 ? other(i, -1, -1) : i;
      const int r2 = nch > 2 ? other(i, r1, -1) : r1;
      double *pi = prop.data() + (size_t)i * npars;
      const double *xi = x.data() + (size_t)i * npars;
      const double *x1 = x.data() + (size_t)r1 * npars, *x2 = x.data() + (size_t)r2 * npars;
      logjac[i] = 0.0;
      if (do_snooker && t % 10 != 0) {
        // snooker update: move along the line through a third chain
        const int z = other(i, r1, r2);
        const double *xz = x.data() + (size_t)z * npars;
        double nd = 0.0, proj = 0.0;
        for (int j : free_) nd += (xi[j] - xz[j]) * (xi[j] - xz[j]);
        nd = std::sqrt(nd);
        if (nd == 0.0) nd = 1.0;
        for (int j : free_) proj += (x1[j] - x2[j]) * (xi[j] - xz[j]) / nd;
        const double g = 1.2 + unif(rng);
        double ndn = 0.0;
        for (int j : free_) {
          pi[j] = xi[j] + g * proj * (xi[j] - xz[j]) / nd;
          ndn += (pi[j] - xz[j]) * (pi[j] - xz[j]);
        }
        logjac[i] = (nfree - 1) * (std::log(std::max(std::sqrt(ndn), 1e-300)) - std::log(nd));
      } else {
        const double gam = t % 10 == 0 ? 1.0 : gamma0;
        for (int j : free_) pi[j] = xi[j] + gam * (x1[j] - x2[j]) + 1e-3 * stepsize[j] * normal(rng);
      }
      inside[i] = 1;
      for (int j : free_) inside[i] = inside[i] && pi[j] >= pmin[j] && pi[j] <= pmax[j];
    }
    chisq_of(prop, inside, cp);
    for (int i = 0; i < nch; i++) {
      const double loga = -0.5 * (cp[i] - c[i]) + logjac[i];
      if (std::isfinite(cp[i]) && std::log(unif(rng)) < loga) {
        std::copy(prop.begin() + (size_t)i * npars, prop.begin() + (size_t)(i + 1) * npars,
                  x.begin() + (size_t)i * npars);
        c[i] = cp[i];
        naccept++;
      }
      std::copy(x.begin() + (size_t)i * npars, x.begin() + (size_t)(i + 1) * npars,
                chain + ((size_t)i * nsteps + t) * npars);
      chisq[(size_t)i * nsteps + t] = c[i];
    }
  }
  if (naccept_out) *naccept_out = naccept;
}

// ---- the resident loop ---------------------------------------------------------------------------------------------
// The same sampler with the population in HBM and no host wait inside an iteration.  Its arithmetic and its random
// draws are mcmc_core.hpp's: a counter-based generator, so a chain can be restated draw for draw anywhere (the
// streams of mcmc_run above and of bart_amd/sampler.py remain their own).  Shared parameters (stepsize < 0),
// Gaussian priors, thinning and the per-sample band fluxes are served here and only here.
namespace {

// One workgroup, chain i on lane i.  Launch t finishes iteration t - 1 on the band fluxes and statuses the step left
// (decision, new state, output rows, per-lane counters), then -- every chain's new point in place -- proposes
// iteration t into the rows the next step reads.  snap (host-mapped, optional): the lanes' accept counts so far.
__global__ __launch_bounds__(mcmc::kMaxChains) void mcmc_advance(mcmc::State s, long t, int finish_prev,
                                                                 int propose_next, long *snap) {
  const int i = threadIdx.x;
  if (finish_prev && i < s.nch) {
    mcmc::finish(s, t - 1, i);
    if (snap) snap[i] = s.counts[(size_t)i * 4];
  }
  __syncthreads();
  if (propose_next && i < s.nch) mcmc::propose(s, t, i);
}

// The same launch for several independent retrievals (mcmc_core.hpp: GROUPS): workgroup g reads group g's State from
// device memory -- a uniform address, so the wave holds it in scalar registers as it holds mcmc_advance's argument --
// and lane i is chain i of that group.  No lane reads or writes a row of another group.  snap: [ngroups][nch].
__global__ __launch_bounds__(mcmc::kMaxChains) void mcmc_advance_groups(const mcmc::State *groups, long t,
                                                                        int finish_prev, int propose_next, long *snap) {
  const mcmc::State s = groups[blockIdx.x];
  const int i = threadIdx.x;
  if (finish_prev && i < s.nch) {
    mcmc::finish(s, t - 1, i);
    if (snap) snap[(size_t)blockIdx.x * s.nch + i] = s.counts[(size_t)i * 4];
  }
  __syncthreads();
  if (propose_next && i < s.nch) mcmc::propose(s, t, i);
}

__global__ void mcmc_draws_kernel(unsigned long long seed, unsigned long long t, int nch, int npars, double *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nch) mcmc::draws_row(seed, t, nch, i, npars, out + (size_t)i * (mcmc::kDrawsHead + npars));
}

// ---- the Gelman-Rubin statistic of the chain in device memory (gr_core.hpp states every sum and its order) -----------
// Leaf stage: one lane per (chain, tile, parameter), the parameter fastest, so the lanes of a wave read whole rows.
// leafs[nch][ntiles][npars][3]; the lanes of parameters that are not free write nothing.
__global__ __launch_bounds__(256) void mcmc_gr_leaf(const double *chain, int nch, long nkept, int npars,
                                                    const double *stepsize, long r0, long r1, double *leafs) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const long nt = gr::tiles(r0, r1);
  if (q >= (size_t)nch * nt * npars) return;
  const int j = (int)(q % npars);
  if (!(stepsize[j] > 0)) return;
  const size_t ik = q / npars;
  gr::leaf(chain, nkept, npars, r0, r1, (int)(ik / nt), (long)(ik % nt), j, leafs + q * 3);
}

// Merge stage: one lane per (chain, parameter), its tiles in ascending order.  triples[nch][npars][3].
__global__ __launch_bounds__(256) void mcmc_gr_merge(const double *leafs, int nch, long nt, int npars,
                                                     const double *stepsize, double *triples) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (size_t)nch * npars) return;
  const int j = (int)(q % npars);
  const size_t i = q / npars;
  double a[3] = {0.0, 0.0, 0.0};
  if (stepsize[j] > 0) {
    const double *t = leafs + (i * nt * npars + j) * 3;
    a[0] = t[0]; a[1] = t[1]; a[2] = t[2];
    for (long k = 1; k < nt; k++) gr::merge(a, t + (size_t)k * npars * 3);
  }
  for (int c = 0; c < 3; c++) triples[q * 3 + c] = a[c];
}

// Finisher: one workgroup, parameter j on lane j.  Writes the record the host reads (host-mapped, as mcmc_advance's
// snap): rec_d = psrf[npars] then the triples; rec_w = converged, then the four counters summed over the chains as
// they stand now (counts null: zeros).
__global__ __launch_bounds__(gr::kFinishLanes) void mcmc_gr_finish(const double *triples, int nch, int npars,
                                                                   const double *stepsize, double threshold,
                                                                   const long *counts, double *rec_d, long *rec_w) {
  __shared__ double psrf[kMaxPars];
  const int j = threadIdx.x;
  if (j < npars) {
    psrf[j] = stepsize[j] > 0 ? gr::psrf_of(triples + (size_t)j * 3, (size_t)npars * 3, nch) : 0.0;
    rec_d[j] = psrf[j];
  }
  for (size_t q = j; q < (size_t)nch * npars * 3; q += gr::kFinishLanes) rec_d[npars + q] = triples[q];
  __syncthreads();
  if (j == 0) rec_w[0] = gr::converged_of(psrf, stepsize, npars, threshold);
  if (j >= 1 && j <= 4) {
    long sum = 0;
    if (counts)
      for (int i = 0; i < nch; i++) sum += counts[(size_t)i * 4 + (j - 1)];
    rec_w[j] = sum;
  }
}

// The three launches of one test on `stream`, their scratch, and the host-mapped records: `slots` of them, each
// psrf[npars] + triples[nch][npars][3] doubles and kRecWords words.
struct GrTest {
  static constexpr int kRecWords = 5;
  int nch, npars;
  DevBuf<double> leafs, triples;
  PinBuf<double> rec_d;
  PinBuf<long> rec_w;
  double *rec_d_dev = nullptr;
  long *rec_w_dev = nullptr;

  size_t doubles() const { return (size_t)npars + (size_t)nch * npars * 3; }
  GrTest(int nch_, int npars_, long maxrows, int slots) : nch(nch_), npars(npars_) {
    leafs.reserve((size_t)nch * gr::tiles(0, maxrows) * npars * 3);
    triples.reserve((size_t)nch * npars * 3);
    rec_d.reserve(doubles() * slots);
    rec_w.reserve((size_t)kRecWords * slots);
    void *p = nullptr;
    HIPCHK(hipHostGetDevicePointer(&p, rec_d.get(), 0));
    rec_d_dev = static_cast<double *>(p);
    HIPCHK(hipHostGetDevicePointer(&p, rec_w.get(), 0));
    rec_w_dev = static_cast<long *>(p);
  }
  const double *psrf(int slot) const { return rec_d.get() + doubles() * slot; }
  const long *words(int slot) const { return rec_w.get() + (size_t)kRecWords * slot; }
  // rows [r0, r1) of the device chain[nch][nkept][npars]; gr::testable(nch, r0, r1) and r1 - r0 <= maxrows hold
  void enqueue(const double *chain, long nkept, const double *stepsize, long r0, long r1, double threshold,
               const long *counts, int slot, hipStream_t st) {
    const long nt = gr::tiles(r0, r1);
    const size_t lanes = (size_t)nch * nt * npars, pairs = (size_t)nch * npars;
    hipLaunchKernelGGL(mcmc_gr_leaf, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, chain, nch, nkept, npars,
                       stepsize, r0, r1, leafs.get());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(mcmc_gr_merge, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, leafs.get(), nch, nt,
                       npars, stepsize, triples.get());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(mcmc_gr_finish, dim3(1), dim3(gr::kFinishLanes), 0, st, triples.get(), nch, npars, stepsize,
                       gr::threshold_of(threshold), counts, rec_d_dev + doubles() * slot,
                       rec_w_dev + (size_t)kRecWords * slot);
    HIPCHK(hipGetLastError());
  }
};

// ---- the effective sample size of the chain in device memory (ess_core.hpp states every sum and its order) ----------
// The lagged sums S_k.  A workgroup owns one (chain i, free parameter, block b of ess::kLanes consecutive lags); lane l
// carries S_k of lag k = b kLanes + l in a register and adds to it in ascending row order, kLanes rows a step.  The
// differences x - m go through LDS: win_a holds those of the step's rows (every lane reads the same one), win_b a ring
// of two halves with those of the rows b kLanes further on -- the half the step before loaded as its "next" and the
// next one, loaded now -- in which lane l reads entry rr + l of row rr's partner.  A row >= r1 is never read: its
// entry is 0.0 and no lane adds it.  The means are the merge stage's (triples[nch][npars][3]); acf[nch][npars][K + 1]
// is written for the free parameters alone.  Grid: nch nfree ceil((K + 1) / kLanes) workgroups, the lag block fastest.
__global__ __launch_bounds__(ess::kLanes) void mcmc_ess_lags(const double *chain, int nch, long nkept, int npars,
                                                             const double *stepsize, const double *triples, long r0,
                                                             long r1, long K, int nfree, double *acf) {
  constexpr int L = ess::kLanes;
  __shared__ double win_a[L], win_b[2 * L];
  const int l = threadIdx.x;
  const long nblk = (K + L) / L;
  size_t w = blockIdx.x;
  const long b = (long)(w % nblk);
  w /= nblk;
  const int f = (int)(w % nfree), i = (int)(w / nfree);
  if (i >= nch) return;
  int j = 0;   // the f-th free parameter
  for (int seen = -1; j < npars; j++)
    if (stepsize[j] > 0 && ++seen == f) break;
  if (j >= npars) return;
  const double m = triples[((size_t)i * npars + j) * 3 + 1];
  const double *col = chain + (size_t)i * nkept * npars + j;
  const long k = b * L + l;        // this lane's lag
  const long lim = r1 - k;         // rows r < lim have a partner r + k
  const long first = r0 + b * L;   // the row of the ring's entry 0
  auto diff_at = [&](long row) { return row < r1 ? ess::diff(col[(size_t)row * npars], m) : 0.0; };
  double s = 0.0;
  win_b[l] = diff_at(first + l);
  const long nsteps = (r1 - first + L - 1) / L;   // rows r0 ... r1 - 1 - b kLanes: those with a partner at lag b kLanes
  for (long c = 0; c < nsteps; c++) {
    const long base = r0 + c * L;
    win_a[l] = diff_at(base + l);
    win_b[(int)((c + 1) & 1) * L + l] = diff_at(first + (c + 1) * L + l);
    __syncthreads();
    const int h = (int)(c & 1) * L + l;
    for (int rr = 0; rr < L; rr++) {
      const double t = ess::lag_add(s, win_a[rr], win_b[(h + rr) & (2 * L - 1)]);
      s = base + rr < lim ? t : s;
    }
    __syncthreads();
  }
  if (k <= K) acf[((size_t)i * npars + j) * (K + 1) + k] = s;
}

// Finisher: one workgroup.  A lane per (chain, parameter) for tau and the truncated flag, then parameter j on lane j
// for ess and lane 0 for `reached`.  Writes the record the host reads (host-mapped, as mcmc_gr_finish's): rec_d =
// ess[npars] then tau[nch][npars]; rec_w = reached, the four counters summed over the chains as they stand now
// (counts null: zeros), then truncated[nch][npars].  tau and trunc: the same in device memory, for the second stage.
constexpr int kEssFinishLanes = 256;
static_assert(kEssFinishLanes >= kMaxPars, "one lane per parameter");
__global__ __launch_bounds__(kEssFinishLanes) void mcmc_ess_finish(const double *acf, int nch, int npars,
                                                                   const double *stepsize, long n, long K,
                                                                   double target, const long *counts, double *tau,
                                                                   int *trunc, double *rec_d, long *rec_w) {
  __shared__ double e[kMaxPars];
  const int l = threadIdx.x;
  for (size_t q = l; q < (size_t)nch * npars; q += kEssFinishLanes) {
    int tr = 0;
    const double t = stepsize[q % npars] > 0 ? ess::tau_of(acf + q * (K + 1), K, &tr) : 0.0;
    tau[q] = t;
    trunc[q] = tr;
    rec_d[npars + q] = t;
    rec_w[5 + q] = tr;
  }
  __syncthreads();
  if (l < npars) {
    e[l] = stepsize[l] > 0 ? ess::ess_of(tau + l, (size_t)npars, nch, n) : 0.0;
    rec_d[l] = e[l];
  }
  __syncthreads();
  if (l == 0) rec_w[0] = ess::reached_of(e, trunc, stepsize, nch, npars, target);
  if (l >= 1 && l <= 4) {
    long sum = 0;
    if (counts)
      for (int i = 0; i < nch; i++) sum += counts[(size_t)i * 4 + (l - 1)];
    rec_w[l] = sum;
  }
}

// The launches of one ESS test on `stream` -- the Gelman-Rubin test's leaf and merge stages for the means, the lagged
// sums, the finisher -- their scratch, and the host-mapped records: `slots` of them, each ess[npars] + tau[nch][npars]
// doubles and 5 + nch npars words.
struct EssTest {
  int nch, npars, nfree;
  long maxlag;   // as ess::maxlag_of gives it
  DevBuf<double> leafs, triples, acf, tau;
  DevBuf<int> trunc;
  PinBuf<double> rec_d;
  PinBuf<long> rec_w;
  double *rec_d_dev = nullptr;
  long *rec_w_dev = nullptr;

  size_t doubles() const { return (size_t)npars + (size_t)nch * npars; }
  size_t words() const { return 5 + (size_t)nch * npars; }
  // stepsize: the host's copy (the launches read the device's)
  EssTest(int nch_, int npars_, const double *stepsize, long maxrows, long maxlag_, int slots)
      : nch(nch_), npars(npars_), nfree(0), maxlag(ess::maxlag_of(maxlag_)) {
    for (int j = 0; j < npars; j++) nfree += stepsize[j] > 0;
    leafs.reserve((size_t)nch * gr::tiles(0, maxrows) * npars * 3);
    triples.reserve((size_t)nch * npars * 3);
    acf.reserve((size_t)nch * npars * (ess::lags(maxlag, maxrows) + 1));
    tau.reserve((size_t)nch * npars);
    trunc.reserve((size_t)nch * npars);
    rec_d.reserve(doubles() * slots);
    rec_w.reserve(words() * slots);
    void *p = nullptr;
    HIPCHK(hipHostGetDevicePointer(&p, rec_d.get(), 0));
    rec_d_dev = static_cast<double *>(p);
    HIPCHK(hipHostGetDevicePointer(&p, rec_w.get(), 0));
    rec_w_dev = static_cast<long *>(p);
  }
  const double *stat(int slot) const { return rec_d.get() + doubles() * slot; }
  const long *word(int slot) const { return rec_w.get() + words() * slot; }
  // rows [r0, r1) of the device chain[nch][nkept][npars]; ess::testable(r0, r1) and r1 - r0 <= maxrows hold
  void enqueue(const double *chain, long nkept, const double *stepsize, long r0, long r1, double target,
               const long *counts, int slot, hipStream_t st) {
    const long nt = gr::tiles(r0, r1), n = r1 - r0, K = ess::lags(maxlag, n);
    const size_t lanes = (size_t)nch * nt * npars, pairs = (size_t)nch * npars;
    hipLaunchKernelGGL(mcmc_gr_leaf, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, chain, nch, nkept, npars,
                       stepsize, r0, r1, leafs.get());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(mcmc_gr_merge, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, leafs.get(), nch, nt,
                       npars, stepsize, triples.get());
    HIPCHK(hipGetLastError());
    if (nfree > 0) {
      const size_t groups = (size_t)nch * nfree * ((K + ess::kLanes) / ess::kLanes);
      hipLaunchKernelGGL(mcmc_ess_lags, dim3((unsigned)groups), dim3(ess::kLanes), 0, st, chain, nch, nkept, npars,
                         stepsize, triples.get(), r0, r1, K, nfree, acf.get());
      HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(mcmc_ess_finish, dim3(1), dim3(kEssFinishLanes), 0, st, acf.get(), nch, npars, stepsize, n, K,
                       target, counts, tau.get(), trunc.get(), rec_d_dev + doubles() * slot, rec_w_dev + words() * slot);
    HIPCHK(hipGetLastError());
  }
};

struct Events {
  hipEvent_t ev[2] = {nullptr, nullptr};
  Events() {
    for (hipEvent_t &e : ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  ~Events() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace

void mcmc_draws_probe(unsigned long long seed, unsigned long long t, int nchains, int npars, double *out) {
  if (nchains < 1 || nchains > (1 << 20) || npars < 1 || npars > mcmc::kMaxPars)
    throw std::invalid_argument("mcmc_draws: 1 <= nchains <= 2^20 and 1 <= npars <= 64");
  const size_t n = (size_t)nchains * (mcmc::kDrawsHead + npars);
  DevBuf<double> d;
  d.reserve(n);
  mcmc_draws_kernel<<<dim3((unsigned)((nchains + 255) / 256)), dim3(256)>>>(seed, t, nchains, npars, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, d, sizeof(double) * n, hipMemcpyDeviceToHost));
}

void mcmc_gr_probe(const double *chain, int nch, long nkept, int npars, const double *stepsize, long r0, long r1,
                   double threshold, double *psrf, double *triples, int *converged) {
  if (nch < 1 || nch > (1 << 20) || npars < 1 || npars > kMaxPars || nkept < 1)
    throw std::invalid_argument("bartrt_mcmc_gr: 1 <= nchains <= 2^20, 1 <= npars <= 64 and nkept >= 1");
  if (r0 < 0 || r1 < r0 || r1 > nkept || threshold < 0)
    throw std::invalid_argument("bartrt_mcmc_gr: 0 <= r0 <= r1 <= nkept and threshold >= 0");
  const size_t nt = (size_t)nch * npars * 3;
  std::fill(psrf, psrf + npars, 0.0);
  std::fill(triples, triples + nt, 0.0);
  *converged = 0;
  if (!gr::testable(nch, r0, r1)) return;   // no test: zeros
  DevBuf<double> d_chain, d_step;
  d_chain.upload(chain, (size_t)nch * nkept * npars);
  d_step.upload(stepsize, npars);
  GrTest test(nch, npars, r1 - r0, 1);
  test.enqueue(d_chain, nkept, d_step, r0, r1, threshold, nullptr, 0, nullptr);
  HIPCHK(hipDeviceSynchronize());
  std::copy(test.psrf(0), test.psrf(0) + npars, psrf);
  std::copy(test.psrf(0) + npars, test.psrf(0) + npars + nt, triples);
  *converged = (int)test.words(0)[0];
}

void mcmc_ess_probe(const double *chain, int nch, long nkept, int npars, const double *stepsize, long r0, long r1,
                    long maxlag, double target, double *tau, double *ess_out, int *truncated, double *acf,
                    int *reached) {
  if (nch < 1 || nch > (1 << 20) || npars < 1 || npars > kMaxPars || nkept < 1)
    throw std::invalid_argument("bartrt_mcmc_ess: 1 <= nchains <= 2^20, 1 <= npars <= 64 and nkept >= 1");
  if (r0 < 0 || r1 < r0 || r1 > nkept || !(target >= 0))
    throw std::invalid_argument("bartrt_mcmc_ess: 0 <= r0 <= r1 <= nkept and esstarget >= 0");
  if (maxlag < 0 || maxlag > ess::kMaxLag)
    throw std::invalid_argument("bartrt_mcmc_ess: maxlag = " + std::to_string(maxlag) + " is not within 0 (the default, " +
                                std::to_string(ess::kDefaultLag) + ") ... " + std::to_string(ess::kMaxLag));
  const size_t pairs = (size_t)nch * npars;
  const long K = ess::lags(ess::maxlag_of(maxlag), r1 - r0);
  std::fill(ess_out, ess_out + npars, 0.0);
  std::fill(tau, tau + pairs, 0.0);
  std::fill(truncated, truncated + pairs, 0);
  if (acf && K >= 0) std::fill(acf, acf + pairs * (K + 1), 0.0);
  *reached = 0;
  if (!ess::testable(r0, r1)) return;   // no test: zeros
  DevBuf<double> d_chain, d_step;
  d_chain.upload(chain, (size_t)nch * nkept * npars);
  d_step.upload(stepsize, npars);
  EssTest test(nch, npars, stepsize, r1 - r0, maxlag, 1);
  HIPCHK(hipMemset(test.acf, 0, sizeof(double) * pairs * (K + 1)));   // (the lags kernel writes the free parameters' alone)
  test.enqueue(d_chain, nkept, d_step, r0, r1, target, nullptr, 0, nullptr);
  HIPCHK(hipDeviceSynchronize());
  std::copy(test.stat(0), test.stat(0) + npars, ess_out);
  std::copy(test.stat(0) + npars, test.stat(0) + npars + pairs, tau);
  for (size_t q = 0; q < pairs; q++) truncated[q] = (int)test.word(0)[5 + q];
  if (acf) HIPCHK(hipMemcpy(acf, test.acf, sizeof(double) * pairs * (K + 1), hipMemcpyDeviceToHost));
  *reached = (int)test.word(0)[0];
}

namespace {

// The resident loop over G groups of nch chains each (mcmc_core.hpp: GROUPS); mcmc_run_resident is its G = 1 under its
// own name and through its own kernel (by_value: mcmc_advance on the one State; else mcmc_advance_groups on the array
// of them).  Outputs per group: naccept [G], nbad [G][4], converged_at [G] (each may be null).
void resident_loop(Engine &e, const std::string &who, int G, const McmcGroup *groups, int nch, long nsteps,
                   const McmcOpts &opts, bool by_value, double *chain, double *chisq, double *models, long *naccept_out,
                   long *nbad, int *converged_at) {
  const int npars = groups[0].p.npars, ndata = groups[0].p.ndata;
  if (npars < 1 || nsteps < 1) throw std::invalid_argument(who + ": bad sizes");
  if (npars > mcmc::kMaxPars) throw std::invalid_argument(who + ": too many parameters (at most 64)");
  if (opts.thin < 1 || opts.block < 1) throw std::invalid_argument(who + ": thin and block must be >= 1");
  if (opts.walk == mcmc::kWalkUnif)
    throw std::invalid_argument(who + ": walk = 3 (unif) is not a chain: bartrt_grid_run makes model grids");
  if (opts.walk != 0 && opts.walk != mcmc::kWalkMrw)
    throw std::invalid_argument(who + ": walk = " + std::to_string(opts.walk) +
                                " is not one of 0 (demc / snooker) and 2 (mrw)");
  const long first = opts.first, B = opts.block;
  for (int g = 0; g < G; g++)
    if (first < 0 || (first > 0) != (groups[g].start != nullptr))
      throw std::invalid_argument(who + ": first > 0 and start come together (a resumed run), or neither");
  if (first % opts.thin != 0)
    throw std::invalid_argument(who + ": first = " + std::to_string(first) + " is not a multiple of thin = " +
                                std::to_string(opts.thin) + ": a run resumes on a kept row");
  if (opts.grcheck < 0 || opts.burnin < 0 || opts.ngr < 0 || opts.grthreshold < 0)
    throw std::invalid_argument(who + ": burnin, grcheck, grthreshold and ngr must be >= 0");
  if (opts.grcheck > 0 && (opts.grcheck % B != 0 || B % opts.thin != 0))
    throw std::invalid_argument(who + ": grcheck = " + std::to_string(opts.grcheck) +
                                " must be a multiple of block = " + std::to_string(B) + ", and block of thin = " +
                                std::to_string(opts.thin) + ": every test falls on a block end that is a kept row");
  const bool ess_on = opts.esstarget > 0;
  if (!(opts.esstarget >= 0) || opts.maxlag < 0)
    throw std::invalid_argument(who + ": esstarget and maxlag must be >= 0");
  if (opts.maxlag > ess::kMaxLag)
    throw std::invalid_argument(who + ": maxlag = " + std::to_string(opts.maxlag) + " is more than " +
                                std::to_string(ess::kMaxLag) + " lags");
  if (ess_on && opts.grcheck == 0)
    throw std::invalid_argument(who + ": esstarget > 0 with grcheck = 0: the effective-sample-size tests run where "
                                      "the convergence tests run, every grcheck iterations");
  if (!ess_on && (opts.essexit || opts.essstat || opts.esstau))
    throw std::invalid_argument(who + ": essexit, essstat and esstau come with esstarget > 0");
  std::vector<Objective> objective;
  if (by_value) objective.push_back(check_retrieval(who, &e, groups[0].p));
  else {
    std::vector<Objective> stated;
    for (int g = 0; g < G; g++) stated.push_back(groups[g].p);
    objective = check_groups(who, G, nch, stated.data(),
                             [&](const std::string &name, const Objective &p) { return check_retrieval(name, &e, p); });
  }

  const long nkept = mcmc::kept_rows(nsteps, opts.thin);
  const size_t np = npars, nd = ndata, n = nch, N = (size_t)G * n;   // n: a group's chains, N: the rows of a launch
  // the start, on the host through step_run_host as mcmc_run makes it, then uploaded once
  std::vector<double> x(N * np), c(N), cur(N * nd);
  std::vector<int> status(N);
  std::vector<long> total(4 * (size_t)G, 0);   // per group: accepted proposals, models rejected with status 1, 2, 3
  mcmc::State h{};
  h.nch = nch; h.snooker = opts.snooker; h.nsteps = nsteps; h.thin = opts.thin;
  h.first = first;
  h.walk = opts.walk;
  h.x = x.data(); h.c = c.data(); h.cur = cur.data();
  std::vector<mcmc::State> hs;
  for (int g = 0; g < G; g++) hs.push_back(mcmc::group_state(h, g, objective[g], groups[g].seed));
  auto model = [&](const double *rows, int m, double *band, int *st) { step_run_host(e, rows, m, npars, band, st); };
  if (first > 0) {
    // a resumed run: the population is the last rows of the run before; c and cur come back from one model call on
    // them, as start_groups evaluates a round (the same bits: the model and chisq_of are the loop's own).  No draw is
    // made and nothing is counted: the run before counted these models when it proposed them.
    for (int g = 0; g < G; g++) std::copy(groups[g].start, groups[g].start + n * np, hs[g].x);
    model(h.x, (int)N, h.cur, status.data());
    for (int g = 0; g < G; g++)
      for (size_t i = 0; i < n; i++)
        hs[g].c[i] = status[g * n + i] == 0 ? mcmc::chisq_of(hs[g], hs[g].cur + i * nd, hs[g].x + i * np) : INFINITY;
  } else {
    std::vector<const double *> params;
    for (int g = 0; g < G; g++) params.push_back(groups[g].params);
    std::vector<char> ok(G);
    mcmc::start_groups(hs.data(), G, params.data(), model, status.data(), total.data(), ok.data());
    for (int g = 0; g < G; g++)
      if (!ok[g])
        throw IoError{who + (by_value ? "" : ": group " + std::to_string(g)) +
                      ": no chain starts on a physical model: check params/pmin/pmax"};
  }

  std::vector<std::unique_ptr<DeviceObjective>> consts;
  for (int g = 0; g < G; g++) consts.emplace_back(new DeviceObjective(objective[g]));
  DevBuf<double> d_pop, d_out;
  DevBuf<int> d_int;
  DevBuf<long> d_counts;
  // population: x c cur logjac prop band
  d_pop.reserve(N * np + N + N * nd + N + N * np + N * nd);
  d_int.reserve(2 * N);
  d_counts.reserve(4 * N);
  d_out.reserve(N * nkept * (np + 1 + (models ? nd : 0)));
  HIPCHK(hipMemset(d_pop, 0, sizeof(double) * d_pop.count()));
  HIPCHK(hipMemset(d_int, 0, sizeof(int) * 2 * N));
  HIPCHK(hipMemset(d_counts, 0, sizeof(long) * 4 * N));
  mcmc::State d = h;   // the heads of the common arrays; with one group, that group's State but for its problem
  double *q = d_pop;
  d.x = q; q += N * np;
  d.c = q; q += N;
  d.cur = q; q += N * nd;
  d.logjac = q; q += N;
  d.prop = q; q += N * np;
  double *d_band = q;
  d.band = d_band;
  d.inside = d_int;
  int *d_status = d_int + N;
  d.status = d_status;
  d.counts = d_counts;
  d.chain = d_out;
  d.chisq = d.chain + N * nkept * np;
  d.models = models ? d.chisq + N * nkept : nullptr;
  HIPCHK(hipMemcpy(d.x, x.data(), sizeof(double) * N * np, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.c, c.data(), sizeof(double) * N, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.cur, cur.data(), sizeof(double) * N * nd, hipMemcpyHostToDevice));
  std::vector<mcmc::State> ds;
  for (int g = 0; g < G; g++) ds.push_back(mcmc::group_state(d, g, consts[g]->d, groups[g].seed));
  DevBuf<mcmc::State> d_groups;
  if (!by_value) d_groups.upload(ds);

  // accept counts at the end of a block, one slot per block in flight
  PinBuf<long> snap;
  snap.reserve(2 * N);
  void *snap_dev = nullptr;
  HIPCHK(hipHostGetDevicePointer(&snap_dev, snap.get(), 0));
  Events events;
  const long nblocks = (nsteps + B - 1) / B;
  const unsigned threads = (unsigned)((nch + 63) / 64 * 64);
  // t counts this call's iterations; the kernel is given the global one
  auto launch = [&](long t, long *snap_slot) {
    if (by_value)
      hipLaunchKernelGGL(mcmc_advance, dim3(1), dim3(threads), 0, e.stream, ds[0], first + t, (int)(t > 0),
                         (int)(t < nsteps), snap_slot);
    else
      hipLaunchKernelGGL(mcmc_advance_groups, dim3((unsigned)G), dim3(threads), 0, e.stream, d_groups.get(), first + t,
                         (int)(t > 0), (int)(t < nsteps), snap_slot);
    HIPCHK(hipGetLastError());
    if (t < nsteps) step_run_dev(e, d.prop, (int)N, npars, d_band, d_status, nullptr, e.stream, nullptr);
  };
  // Convergence tests: after block b, behind it on the stream, where its end T (iterations of this call) is a
  // multiple of grcheck or the last one and the rows past the burn-in are enough for a test.  The rows of this call
  // alone enter: kept row q is global iteration first + (q + 1) thin - 1, so the first one at or past burnin is
  // (burnin - first) / thin.  Every group is tested on its own slice of the chain by launches of its own (one scratch,
  // reused in stream order); one record per group and block in flight, read in finished(b).
  const long r0 = std::max(0L, opts.burnin - first) / opts.thin;
  auto test_rows = [&](long T) {   // the end of the row range of the test after T iterations, or 0: no test there
    if (opts.grcheck == 0 || (T % opts.grcheck != 0 && T != nsteps)) return 0L;
    const long r1 = mcmc::kept_rows(T, opts.thin);
    return gr::testable(nch, r0, r1) || (ess_on && ess::testable(r0, r1)) ? r1 : 0L;
  };
  std::unique_ptr<GrTest> tests;
  if (opts.grcheck > 0 && gr::testable(nch, r0, nkept)) tests.reset(new GrTest(nch, npars, nkept - r0, 2 * G));
  // Effective-sample-size tests (ess_core.hpp; the single call alone): at the same places, behind the same block, on
  // the same rows; one chain is enough for them, so with them a test is made wherever four rows lie past the burn-in
  // and the Gelman-Rubin record of a one-chain test is zeros.
  std::unique_ptr<EssTest> ess_tests;
  if (ess_on && ess::testable(r0, nkept))
    ess_tests.reset(new EssTest(nch, npars, groups[0].p.stepsize, nkept - r0, opts.maxlag, 2));
  bool tested[2] = {false, false};
  int ntests = 0;
  long stop = -1;   // grexit / essexit: the iterations the result holds
  std::vector<long> stop_counts(4 * (size_t)G, 0);   // and the groups' counters there
  if (converged_at) std::fill(converged_at, converged_at + G, -1);
  auto finished = [&](long b) {   // block b is done: wait for it, report, read its test; true: stop here
    HIPCHK(hipEventSynchronize(events.ev[b % 2]));
    const long T = std::min((b + 1) * B, nsteps);
    if (opts.progress) {
      long acc = 0;
      for (size_t i = 0; i < N; i++) acc += snap.get()[(size_t)(b % 2) * N + i];
      opts.progress(T, acc, opts.progress_user);
    }
    if (!tested[b % 2]) return false;
    const int k = ntests++;
    bool all = true;
    const bool gr_made = tests && gr::testable(nch, r0, mcmc::kept_rows(T, opts.thin));
    for (int g = 0; g < G; g++) {
      const int slot = (int)(b % 2) * G + g;
      if (k < opts.ngr && opts.grstat) {
        double *to = opts.grstat + ((size_t)k * G + g) * np;
        if (gr_made) std::copy(tests->psrf(slot), tests->psrf(slot) + np, to);
        else std::fill(to, to + np, 0.0);
      }
      const bool conv = gr_made && tests->words(slot)[0] != 0;
      if (conv && converged_at && converged_at[g] < 0) converged_at[g] = k;
      all = all && conv;
    }
    if (k < opts.ngr && opts.grwhen) opts.grwhen[k] = first + T;
    bool reached = false;
    if (ess_tests) {
      const int slot = (int)(b % 2);
      const double *rec = ess_tests->stat(slot);
      if (k < opts.ngr && opts.essstat) std::copy(rec, rec + np, opts.essstat + (size_t)k * np);
      if (k < opts.ngr && opts.esstau) std::copy(rec + np, rec + np + n * np, opts.esstau + (size_t)k * n * np);
      reached = ess_tests->word(slot)[0] != 0;
    }
    if (!(opts.grexit || opts.essexit) || (opts.grexit && !all) || (opts.essexit && !reached)) return false;
    stop = T;
    for (int g = 0; g < G; g++) {
      const long *w = ess_tests ? ess_tests->word((int)(b % 2)) : tests->words((int)(b % 2) * G + g);
      std::copy(w + 1, w + 5, stop_counts.begin() + 4 * (size_t)g);
    }
    return true;
  };
  launch(0, nullptr);
  long enqueued = 0;
  for (long b = 0; b < nblocks; b++, enqueued++) {
    if (b >= 2 && finished(b - 2)) break;   // at most two blocks in flight
    const long last = std::min((b + 1) * B, nsteps);
    for (long t = b * B + 1; t <= last; t++)
      launch(t, t == last ? static_cast<long *>(snap_dev) + (size_t)(b % 2) * N : nullptr);
    const long r1 = test_rows(last);
    tested[b % 2] = r1 > 0;
    if (r1 > 0 && gr::testable(nch, r0, r1))
      for (int g = 0; g < G; g++)
        tests->enqueue(ds[g].chain, nkept, consts[g]->d.stepsize, r0, r1, opts.grthreshold, ds[g].counts,
                       (int)(b % 2) * G + g, e.stream);
    if (r1 > 0 && ess_on)
      ess_tests->enqueue(ds[0].chain, nkept, consts[0]->d.stepsize, r0, r1, opts.esstarget, ds[0].counts, (int)(b % 2),
                         e.stream);
    HIPCHK(hipEventRecord(events.ev[b % 2], e.stream));
  }
  for (long b = std::max(0L, enqueued - 2); stop < 0 && b < enqueued; b++) finished(b);
  HIPCHK(hipStreamSynchronize(e.stream));   // (after a stop: the blocks in flight run out; their rows are not copied)

  // the rows of the iterations done, chain by chain: the caller's arrays past them are not written
  const long done = stop >= 0 ? stop : nsteps, kd = mcmc::kept_rows(done, opts.thin);
  auto fetch = [&](double *to, const double *from, size_t width) {
    if (kd == nkept) HIPCHK(hipMemcpy(to, from, sizeof(double) * N * nkept * width, hipMemcpyDeviceToHost));
    else HIPCHK(hipMemcpy2D(to, sizeof(double) * nkept * width, from, sizeof(double) * nkept * width,
                       sizeof(double) * kd * width, N, hipMemcpyDeviceToHost));
  };
  fetch(chain, d.chain, np);
  fetch(chisq, d.chisq, 1);
  if (models) fetch(models, d.models, nd);
  for (int g = 0; g < G; g++) {
    long *tg = total.data() + 4 * (size_t)g;
    if (stop >= 0)
      for (int s = 0; s < 4; s++) tg[s] += stop_counts[4 * (size_t)g + s];
    else
      add_counters(ds[g].counts, n, tg);
    if (naccept_out) naccept_out[g] = tg[0];
    if (nbad) {
      nbad[4 * (size_t)g] = 0;
      for (int s = 1; s < 4; s++) nbad[4 * (size_t)g + s] = tg[s];
    }
  }
  if (opts.ngr_out) *opts.ngr_out = ntests;
  if (opts.done) *opts.done = done;
}

}  // namespace

void mcmc_run_resident(Engine &e, const RetrievalProblem &p, int nch, long nsteps, const double *params,
                       const McmcOpts &opts, double *chain, double *chisq, double *models, long *naccept_out,
                       long *nbad) {
  if (!e.step) throw IoError{"mcmc_run_resident: call step_setup first"};
  if (nch < 1) throw std::invalid_argument("mcmc_run_resident: bad sizes");
  if (nch > mcmc::kMaxChains)
    throw std::invalid_argument("mcmc_run_resident: at most 1024 chains (one workgroup); more stay with mcmc_run");
  const McmcGroup one{p, params, opts.seed, opts.start};
  resident_loop(e, "mcmc_run_resident", 1, &one, nch, nsteps, opts, true, chain, chisq, models, naccept_out, nbad,
                nullptr);
}

void mcmc_run_resident_groups(Engine &e, int ngroups, const McmcGroup *groups, int nch, long nsteps,
                              const McmcOpts &opts, double *chain, double *chisq, double *models, long *naccept,
                              long *nbad, int *converged_at) {
  const std::string who = "mcmc_run_resident_groups";
  if (!e.step) throw IoError{who + ": call step_setup first"};
  if (ngroups < 1) throw std::invalid_argument(who + ": ngroups = " + std::to_string(ngroups) + ": at least one group");
  for (int g = 1; g < ngroups; g++)
    if (groups[g].p.npars != groups[0].p.npars || groups[g].p.ndata != groups[0].p.ndata)
      throw std::invalid_argument(who + ": every group has the same npars and ndata");
  if (opts.esstarget != 0 || opts.essexit || opts.maxlag != 0 || opts.essstat || opts.esstau)
    throw std::invalid_argument(who + ": esstarget, essexit, maxlag, essstat and esstau are not served here: the "
                                      "effective-sample-size tests are the single call's (bartrt_mcmc_run_resident)");
  resident_loop(e, who, ngroups, groups, nch, nsteps, opts, false, chain, chisq, models, naccept, nbad, converged_at);
}

}  // namespace bartrt
