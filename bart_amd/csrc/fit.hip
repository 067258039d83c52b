// Batched multi-start Levenberg-Marquardt fit in a box (MC3's `leastsq`; the reference's [MCMC] key of that name,
// examples/demo/BART_eclipse.cfg:98).  The arithmetic is fit_core.hpp's.  An iteration is two model launches: the
// S * nfree forward-difference rows of the Jacobians, then the S * K trial rows of a ladder of K dampings, every
// start's rows in one step_run_dev each -- the large batches the step is fastest at.  Between them one small kernel,
// fit_advance, one wave per start.  Everything is enqueued on the engine's stream; the host waits only every `check`
// iterations, to read how many starts are still running.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/bartrt.h"
#include "comm.hpp"
#include "engine.hpp"
#include "fit_core.hpp"
#include "lds.hpp"
#include "step.hpp"

namespace bartrt {
namespace {

enum { kPick = 0, kSolve = 1 };

struct WaveExec {
  template <class F>
  __device__ void each(F f) const {
    f((int)threadIdx.x);
    __syncthreads();
  }
};

// One wave per start (blockIdx.x).  pick: the start's first lane decides on the trial rows the step evaluated (pick 0:
// on the start's own model), updates the state, writes the next Jacobian rows and this start's slot of `running`
// (host-mapped; may be null).  solve: the wave builds A and g from the perturbed rows' band fluxes in LDS, factors the
// K damped systems and writes the K trial rows.
__global__ __launch_bounds__(fit::kLanes) void fit_advance(fit::Problem p, int phase, long it, int *running) {
  extern __shared__ double fit_lds[];
  const int s = blockIdx.x;
  if (phase == kPick) {
    if (threadIdx.x == 0) {
      fit::pick_start(p, s, it);
      if (running) running[s] = p.status[s] == fit::kRunning;
    }
    return;
  }
  fit::solve_start(p, fit::carve(fit_lds), s, WaveExec{});
}

size_t g_fit_lds_allowed = kLdsDefault;

void launch_advance(const fit::Problem &p, int phase, long it, int *running, hipStream_t st) {
  const size_t lds = phase == kSolve ? fit::kWorkBytes : 0;
  HIPCHK(allow_lds(fit_advance, lds, g_fit_lds_allowed));
  hipLaunchKernelGGL(fit_advance, dim3((unsigned)p.nstarts), dim3(fit::kLanes), lds, st, p, phase, it, running);
  HIPCHK(hipGetLastError());
}

// sizes and options both entry points refuse; returns nfree
int check_problem(const char *who, int nstarts, int npars, int ndata, const double *stepsize, const FitOpts &o) {
  const std::string w = who;
  if (nstarts < 1 || nstarts > (1 << 20) || npars < 1 || ndata < 1)
    throw std::invalid_argument(w + ": bad sizes (1 <= nstarts <= 2^20, npars >= 1, ndata >= 1)");
  if (npars > fit::kMaxPars) throw std::invalid_argument(w + ": too many parameters (at most 64)");
  if (o.nrungs < 1 || o.nrungs > fit::kMaxRungs) throw std::invalid_argument(w + ": 1 <= nrungs <= 8");
  if (o.maxiter < 0 || o.check < 1) throw std::invalid_argument(w + ": maxiter >= 0 and check >= 1");
  if (!(o.fdstep > 0) || !(o.ftol >= 0) || !(o.xtol >= 0) || !(o.lambda0 > 0))
    throw std::invalid_argument(w + ": fdstep and lambda0 must be positive, ftol and xtol not negative");
  const bool priors = o.prior || o.priorlow || o.priorup;
  if (priors && !(o.prior && o.priorlow && o.priorup))
    throw std::invalid_argument(w + ": prior, priorlow and priorup come together");
  int nfree = 0;
  if (const int bad = mcmc::check_stepsize(npars, stepsize, &nfree))
    throw std::invalid_argument(w + ": stepsize[" + std::to_string(bad - 1) + "] = " +
                                std::to_string(stepsize[bad - 1]) + " shares parameter " + std::to_string(bad - 1) +
                                " with a parameter that is out of range or itself shared");
  if (nfree < 1) throw std::invalid_argument(w + ": no free parameter (every stepsize is <= 0)");
  return nfree;
}

// the problem's constants and the starts' state in device memory
struct DeviceFit {
  DevBuf<double> consts, state, trace;
  DevBuf<int> ints;
  DevBuf<long> longs;
  fit::Problem d{};
  double *band = nullptr;
  int *mstatus = nullptr;
  size_t ntrace = 0;

  DeviceFit(int S, int npars, int ndata, int nfree, const double *pmin, const double *pmax, const double *stepsize,
            const double *data, const double *uncert, const FitOpts &o, bool want_trace) {
    const size_t np = npars, nd = ndata, n = S, rows = fit::max_rows(S, nfree, o.nrungs);
    const bool priors = o.prior != nullptr;
    std::vector<double> c;
    auto put = [&](const double *v, size_t m) { c.insert(c.end(), v, v + m); };
    put(pmin, np); put(pmax, np); put(stepsize, np);
    if (priors) { put(o.prior, np); put(o.priorlow, np); put(o.priorup, np); }
    put(data, nd); put(uncert, nd);
    consts.upload(c);
    d.nstarts = S; d.npars = npars; d.ndata = ndata; d.nfree = nfree; d.nrungs = o.nrungs;
    d.maxiter = o.maxiter; d.fdstep = o.fdstep; d.ftol = o.ftol; d.xtol = o.xtol; d.lambda0 = o.lambda0;
    const double *k = consts;
    d.pmin = k; d.pmax = k + np; d.stepsize = k + 2 * np;
    k += 3 * np;
    if (priors) { d.prior = k; d.priorlow = k + np; d.priorup = k + 2 * np; k += 3 * np; }
    d.data = k; d.uncert = k + nd;
    // x chisq lambda D cur jrows trows band
    const size_t total = n * np + n + n + n * np + n * nd + n * nfree * np + n * o.nrungs * np + rows * nd;
    // (these memsets run on the null stream; the engine's stream does not wait for that one.  Every caller follows
    // the constructor with a blocking hipMemcpy into this state before it launches: that copy orders them)
    state.reserve(total);
    HIPCHK(hipMemset(state, 0, sizeof(double) * total));
    double *q = state;
    d.x = q; q += n * np;
    d.chisq = q; q += n;
    d.lambda = q; q += n;
    d.D = q; q += n * np;
    d.cur = q; q += n * nd;
    d.jrows = q; q += n * nfree * np;
    d.trows = q; q += n * o.nrungs * np;
    band = q;
    d.band = band;
    ints.reserve(2 * n + rows);
    HIPCHK(hipMemset(ints, 0, sizeof(int) * (2 * n + rows)));
    d.status = ints; d.valid = ints + n;
    mstatus = ints + 2 * n;
    d.mstatus = mstatus;
    longs.reserve(5 * n);
    HIPCHK(hipMemset(longs, 0, sizeof(long) * 5 * n));
    d.niter = longs; d.nbad = longs + n;
    if (want_trace) {
      ntrace = n * (size_t)(o.maxiter + 1) * (np + 4);
      trace.reserve(ntrace);
      HIPCHK(hipMemset(trace, 0, sizeof(double) * ntrace));
      d.trace = trace;
    }
  }
};

}  // namespace

void fit_probe(int nstarts, int npars, const double *pmin, const double *pmax, const double *stepsize, int ndata,
               const double *data, const double *uncert, const FitOpts &o, const double *x, const double *lambda,
               double *D, const double *cur, const double *pband, const int *pstatus, double *trial, int *valid) {
  const int nfree = check_problem("fit_probe", nstarts, npars, ndata, stepsize, o);
  DeviceFit f(nstarts, npars, ndata, nfree, pmin, pmax, stepsize, data, uncert, o, false);
  const size_t np = npars, nd = ndata, n = nstarts;
  HIPCHK(hipMemcpy(f.d.x, x, sizeof(double) * n * np, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(f.d.lambda, lambda, sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(f.d.D, D, sizeof(double) * n * np, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(f.d.cur, cur, sizeof(double) * n * nd, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(f.band, pband, sizeof(double) * n * nfree * nd, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(f.mstatus, pstatus, sizeof(int) * n * nfree, hipMemcpyHostToDevice));
  launch_advance(f.d, kSolve, 1, nullptr, nullptr);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(trial, f.d.trows, sizeof(double) * n * o.nrungs * np, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(valid, f.d.valid, sizeof(int) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(D, f.d.D, sizeof(double) * n * np, hipMemcpyDeviceToHost));
}

void fit_run(Engine &e, int nstarts, int npars, const double *starts, const double *pmin, const double *pmax,
             const double *stepsize, int ndata, const double *data, const double *uncert, const FitOpts &o,
             double *best, double *chisq, int *status, long *niter, long *nbad) {
  if (!e.step) throw IoError{"fit: call step_setup first"};
  const int nfree = check_problem("fit", nstarts, npars, ndata, stepsize, o);
  if (ndata != e.step->nfilters) throw std::invalid_argument("fit: data length must equal the number of filters");
  if (e.lbl && e.comm) throw CommError{BARTRT_ENOTSUP, "fit: line-by-line engines do not take the communicator's path"};
  if (!e.comm && (e.lo != 0 || e.hi != e.Wfull))
    throw IoError{"fit: the engine is sharded and has no communicator (engine.comm_init); use run()"};

  const int S = nstarts, K = o.nrungs;
  const size_t np = npars, n = S;
  // the step's workspace grows (and waits for the device) here, not inside the loop
  step_ensure(e, (int)fit::max_rows(S, nfree, K));
  DeviceFit f(S, npars, ndata, nfree, pmin, pmax, stepsize, data, uncert, o, o.trace != nullptr);
  std::vector<double> x0(starts, starts + n * np);
  for (size_t s = 0; s < n; s++) mcmc::copy_shared(npars, stepsize, x0.data() + s * np);
  HIPCHK(hipMemcpy(f.d.x, x0.data(), sizeof(double) * n * np, hipMemcpyHostToDevice));

  PinBuf<int> running;
  running.reserve(n);
  std::fill(running.get(), running.get() + n, 1);
  void *running_dev = nullptr;
  HIPCHK(hipHostGetDevicePointer(&running_dev, running.get(), 0));
  auto model = [&](const double *rows, int m) {
    step_run_dev(e, rows, m, npars, f.band, f.mstatus, nullptr, e.stream, nullptr);
  };
  auto any_running = [&] {
    HIPCHK(hipStreamSynchronize(e.stream));
    return std::any_of(running.get(), running.get() + n, [](int r) { return r != 0; });
  };

  long last = 0;   // the last pick made
  model(f.d.x, S);
  for (long it = 0;; it++) {
    launch_advance(f.d, kPick, it, static_cast<int *>(running_dev), e.stream);
    last = it;
    if (it == o.maxiter) break;
    if (it % o.check == 0 && !any_running()) break;
    model(f.d.jrows, S * nfree);
    launch_advance(f.d, kSolve, it, nullptr, e.stream);
    model(f.d.trows, S * K);
  }
  HIPCHK(hipStreamSynchronize(e.stream));

  HIPCHK(hipMemcpy(best, f.d.x, sizeof(double) * n * np, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(chisq, f.d.chisq, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (status) HIPCHK(hipMemcpy(status, f.d.status, sizeof(int) * n, hipMemcpyDeviceToHost));
  if (niter) HIPCHK(hipMemcpy(niter, f.d.niter, sizeof(long) * n, hipMemcpyDeviceToHost));
  if (nbad) {
    std::vector<long> counts(4 * n);
    HIPCHK(hipMemcpy(counts.data(), f.d.nbad, sizeof(long) * 4 * n, hipMemcpyDeviceToHost));
    std::fill(nbad, nbad + 4, 0L);
    for (size_t s = 0; s < n; s++)
      for (int k = 1; k < 4; k++) nbad[k] += counts[4 * s + k];
  }
  if (o.trace) {
    // records past the last pick repeat it: every start had finished by then
    const size_t rec = np + 4, per = (size_t)(o.maxiter + 1) * rec;
    HIPCHK(hipMemcpy(o.trace, f.d.trace, sizeof(double) * f.ntrace, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < n; s++)
      for (long it = last + 1; it <= o.maxiter; it++) {
        double *to = o.trace + s * per + (size_t)it * rec;
        std::copy(to - rec, to, to);
        to[np + 2] = -1.0;
      }
  }
}

}  // namespace bartrt
