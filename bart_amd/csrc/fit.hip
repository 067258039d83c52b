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

#include "engine.hpp"
#include "fit_core.hpp"
#include "lds.hpp"
#include "retrieval_host.hpp"
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

// what both entry points refuse (e null: the probe, which has no engine); returns the problem with nfree counted
Objective check_problem(const char *who, const Engine *e, const RetrievalProblem &p, int nstarts, const FitOpts &o) {
  const std::string w = who;
  if (nstarts < 1 || nstarts > (1 << 20) || p.npars < 1 || p.ndata < 1)
    throw std::invalid_argument(w + ": bad sizes (1 <= nstarts <= 2^20, npars >= 1, ndata >= 1)");
  if (p.npars > fit::kMaxPars) throw std::invalid_argument(w + ": too many parameters (at most 64)");
  if (o.nrungs < 1 || o.nrungs > fit::kMaxRungs) throw std::invalid_argument(w + ": 1 <= nrungs <= 8");
  if (o.maxiter < 0 || o.check < 1) throw std::invalid_argument(w + ": maxiter >= 0 and check >= 1");
  if (!(o.fdstep > 0) || !(o.ftol >= 0) || !(o.xtol >= 0) || !(o.lambda0 > 0))
    throw std::invalid_argument(w + ": fdstep and lambda0 must be positive, ftol and xtol not negative");
  const Objective objective = check_retrieval(w, e, p);
  if (objective.nfree < 1) throw std::invalid_argument(w + ": no free parameter (every stepsize is <= 0)");
  return objective;
}

// the problem's constants and the starts' state in device memory
struct DeviceFit {
  DeviceObjective consts;
  DevBuf<double> state, trace;
  DevBuf<int> ints;
  DevBuf<long> longs;
  fit::Problem d{};
  double *band = nullptr;
  int *mstatus = nullptr;
  size_t ntrace = 0;

  DeviceFit(int S, const Objective &objective, const FitOpts &o, bool want_trace) : consts(objective) {
    const int nfree = objective.nfree;
    const size_t np = objective.npars, nd = objective.ndata, n = S, rows = fit::max_rows(S, nfree, o.nrungs);
    static_cast<Objective &>(d) = consts.d;
    d.nstarts = S; d.nrungs = o.nrungs;
    d.maxiter = o.maxiter; d.fdstep = o.fdstep; d.ftol = o.ftol; d.xtol = o.xtol; d.lambda0 = o.lambda0;
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

void fit_probe(const RetrievalProblem &p, int nstarts, const FitOpts &o, const double *x, const double *lambda,
               double *D, const double *cur, const double *pband, const int *pstatus, double *trial, int *valid) {
  const Objective objective = check_problem("fit_probe", nullptr, p, nstarts, o);
  DeviceFit f(nstarts, objective, o, false);
  const size_t np = p.npars, nd = p.ndata, n = nstarts, nfree = objective.nfree;
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

void fit_run(Engine &e, const RetrievalProblem &p, int nstarts, const double *starts, const FitOpts &o, double *best,
             double *chisq, int *status, long *niter, long *nbad) {
  if (!e.step) throw IoError{"fit: call step_setup first"};
  const Objective objective = check_problem("fit", &e, p, nstarts, o);

  const int S = nstarts, K = o.nrungs, npars = p.npars, nfree = objective.nfree;
  const size_t np = npars, n = S;
  // the step's workspace grows (and waits for the device) here, not inside the loop
  step_ensure(e, (int)fit::max_rows(S, nfree, K));
  DeviceFit f(S, objective, o, o.trace != nullptr);
  std::vector<double> x0(starts, starts + n * np);
  for (size_t s = 0; s < n; s++) copy_shared(npars, p.stepsize, x0.data() + s * np);
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
    std::fill(nbad, nbad + 4, 0L);
    add_counters(f.d.nbad, n, nbad);
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
