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
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine.hpp"
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

__global__ void mcmc_draws_kernel(unsigned long long seed, unsigned long long t, int nch, int npars, double *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nch) mcmc::draws_row(seed, t, nch, i, npars, out + (size_t)i * (mcmc::kDrawsHead + npars));
}

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

void mcmc_run_resident(Engine &e, const RetrievalProblem &p, int nch, long nsteps, const double *params,
                       const McmcOpts &opts, double *chain, double *chisq, double *models, long *naccept_out,
                       long *nbad) {
  const int npars = p.npars, ndata = p.ndata;
  if (!e.step) throw IoError{"mcmc_run_resident: call step_setup first"};
  if (nch < 1 || npars < 1 || nsteps < 1) throw std::invalid_argument("mcmc_run_resident: bad sizes");
  if (nch > mcmc::kMaxChains)
    throw std::invalid_argument("mcmc_run_resident: at most 1024 chains (one workgroup); more stay with mcmc_run");
  if (npars > mcmc::kMaxPars) throw std::invalid_argument("mcmc_run_resident: too many parameters (at most 64)");
  if (opts.thin < 1 || opts.block < 1) throw std::invalid_argument("mcmc_run_resident: thin and block must be >= 1");
  const Objective objective = check_retrieval("mcmc_run_resident", &e, p);

  const long nkept = mcmc::kept_rows(nsteps, opts.thin);
  const size_t np = npars, nd = ndata, n = nch;
  // the start, on the host through step_run_host as mcmc_run makes it, then uploaded once
  std::vector<double> x(n * np), c(n), cur(n * nd);
  std::vector<int> status(n);
  long total[4] = {0, 0, 0, 0};   // accepted proposals, models rejected with status 1, 2, 3
  mcmc::State h{};
  static_cast<Objective &>(h) = objective;
  h.nch = nch; h.snooker = opts.snooker; h.seed = opts.seed; h.nsteps = nsteps; h.thin = opts.thin;
  h.x = x.data(); h.c = c.data(); h.cur = cur.data();
  auto model = [&](const double *rows, int m, double *band, int *st) { step_run_host(e, rows, m, npars, band, st); };
  if (!mcmc::start_population(h, params, model, status.data(), total))
    throw IoError{"mcmc_run_resident: no chain starts on a physical model: check params/pmin/pmax"};

  const DeviceObjective consts(objective);
  DevBuf<double> d_pop, d_out;
  DevBuf<int> d_int;
  DevBuf<long> d_counts;
  // population: x c cur logjac prop band
  d_pop.reserve(n * np + n + n * nd + n + n * np + n * nd);
  d_int.reserve(2 * n);
  d_counts.reserve(4 * n);
  d_out.reserve((size_t)nch * nkept * (np + 1 + (models ? nd : 0)));
  HIPCHK(hipMemset(d_pop, 0, sizeof(double) * d_pop.count()));
  HIPCHK(hipMemset(d_int, 0, sizeof(int) * 2 * n));
  HIPCHK(hipMemset(d_counts, 0, sizeof(long) * 4 * n));
  mcmc::State d = h;
  static_cast<Objective &>(d) = consts.d;
  double *q = d_pop;
  d.x = q; q += n * np;
  d.c = q; q += n;
  d.cur = q; q += n * nd;
  d.logjac = q; q += n;
  d.prop = q; q += n * np;
  double *d_band = q;
  d.band = d_band;
  d.inside = d_int;
  int *d_status = d_int + n;
  d.status = d_status;
  d.counts = d_counts;
  d.chain = d_out;
  d.chisq = d.chain + (size_t)nch * nkept * np;
  d.models = models ? d.chisq + (size_t)nch * nkept : nullptr;
  HIPCHK(hipMemcpy(d.x, x.data(), sizeof(double) * n * np, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.c, c.data(), sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.cur, cur.data(), sizeof(double) * n * nd, hipMemcpyHostToDevice));

  // accept counts at the end of a block, one slot per block in flight
  PinBuf<long> snap;
  snap.reserve(2 * n);
  void *snap_dev = nullptr;
  HIPCHK(hipHostGetDevicePointer(&snap_dev, snap.get(), 0));
  Events events;
  const long B = opts.block, nblocks = (nsteps + B - 1) / B;
  const unsigned threads = (unsigned)((nch + 63) / 64 * 64);
  auto launch = [&](long t, long *snap_slot) {
    hipLaunchKernelGGL(mcmc_advance, dim3(1), dim3(threads), 0, e.stream, d, t, (int)(t > 0), (int)(t < nsteps),
                       snap_slot);
    HIPCHK(hipGetLastError());
    if (t < nsteps) step_run_dev(e, d.prop, nch, npars, d_band, d_status, nullptr, e.stream, nullptr);
  };
  auto finished = [&](long b) {   // block b is done: wait for it and report
    HIPCHK(hipEventSynchronize(events.ev[b % 2]));
    if (!opts.progress) return;
    long acc = 0;
    for (size_t i = 0; i < n; i++) acc += snap.get()[(size_t)(b % 2) * n + i];
    opts.progress(std::min((b + 1) * B, nsteps), acc, opts.progress_user);
  };
  launch(0, nullptr);
  for (long b = 0; b < nblocks; b++) {
    if (b >= 2) finished(b - 2);   // at most two blocks in flight
    const long last = std::min((b + 1) * B, nsteps);
    for (long t = b * B + 1; t <= last; t++)
      launch(t, t == last ? static_cast<long *>(snap_dev) + (size_t)(b % 2) * n : nullptr);
    HIPCHK(hipEventRecord(events.ev[b % 2], e.stream));
  }
  for (long b = std::max(0L, nblocks - 2); b < nblocks; b++) finished(b);
  HIPCHK(hipStreamSynchronize(e.stream));

  const size_t rows = (size_t)nch * nkept;
  HIPCHK(hipMemcpy(chain, d.chain, sizeof(double) * rows * np, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(chisq, d.chisq, sizeof(double) * rows, hipMemcpyDeviceToHost));
  if (models) HIPCHK(hipMemcpy(models, d.models, sizeof(double) * rows * nd, hipMemcpyDeviceToHost));
  add_counters(d_counts, n, total);
  if (naccept_out) *naccept_out = total[0];
  if (nbad) {
    nbad[0] = 0;
    for (int s = 1; s < 4; s++) nbad[s] = total[s];
  }
}

}  // namespace bartrt
