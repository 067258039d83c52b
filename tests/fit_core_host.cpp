// Stand-alone host program over bart_amd/csrc/fit_core.hpp, built and run by tests/test_fit_core_cpu.py (a host
// compiler alone, with the address and undefined-behaviour sanitizers).  It drives the same pick_start / solve_start
// functions the device kernel runs, the lanes of a start one after the other, over analytic models compiled in here.
//
//   fit_core_host check NPARS s0 s1 ...     mcmc::check_stepsize: 0 or 1 + the refused parameter
//   fit_core_host run PROBLEM OUT           the loop on the problem file; results as raw doubles in OUT
//
// PROBLEM (text, whitespace separated): S npars ndata model maxiter nrungs fdstep ftol xtol lambda0 priors reject_par
// reject_par2 reject_above, then pmin pmax stepsize prior priorlow priorup [npars each], data uncert [ndata each], starts
// [S][npars], aux [naux].  model 0: band = A p, aux = A [ndata][npars].  model 1: band_f = p0 exp(-p1 t_f) + p2, aux =
// t [ndata].  model 2 (Rosenbrock as two residuals, ndata = 2): band = (10 (p1 - p0^2), 1 - p0), no aux.  The model
// rejects (status 1, band -1) a row whose parameter reject_par, plus parameter reject_par2 where that is not negative,
// exceeds reject_above (reject_par < 0: never).
// OUT: the number of iterations made (solves), trace [S][maxiter + 1][npars + 4], then per iteration trial
// [S][nrungs][npars], valid [S], D [S][npars] as the solve left them, then best [S][npars], chisq [S], status [S],
// niter [S], nbad [S][4], then 1.0.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../bart_amd/csrc/fit_core.hpp"

using namespace bartrt;

static int run(const char *problem, const char *out_path) {
  std::ifstream in(problem);
  fit::Problem p{};
  int model_id, priors, reject_par, reject_par2;
  double reject_above;
  in >> p.nstarts >> p.npars >> p.ndata >> model_id >> p.maxiter >> p.nrungs >> p.fdstep >> p.ftol >> p.xtol >>
      p.lambda0 >> priors >> reject_par >> reject_par2 >> reject_above;
  if (!in || p.nstarts < 1 || p.npars < 1 || p.npars > fit::kMaxPars || p.ndata < 1 || p.nrungs < 1 ||
      p.nrungs > fit::kMaxRungs || p.maxiter < 0 || reject_par >= p.npars || reject_par2 >= p.npars)
    return 2;
  const int S = p.nstarts, np = p.npars, nd = p.ndata, K = p.nrungs;
  auto read = [&](size_t n) {
    std::vector<double> v(n);
    for (double &d : v) in >> d;
    return v;
  };
  const std::vector<double> pmin = read(np), pmax = read(np), stepsize = read(np), prior = read(np),
                            priorlow = read(np), priorup = read(np), data = read(nd), uncert = read(nd);
  std::vector<double> x = read((size_t)S * np);
  const std::vector<double> aux = read(model_id == 0 ? (size_t)nd * np : model_id == 1 ? (size_t)nd : 0);
  if (!in || (model_id == 1 && np < 3) || (model_id == 2 && (np < 2 || nd != 2))) return 2;
  p.pmin = pmin.data(); p.pmax = pmax.data(); p.stepsize = stepsize.data();
  p.data = data.data(); p.uncert = uncert.data();
  if (priors) { p.prior = prior.data(); p.priorlow = priorlow.data(); p.priorup = priorup.data(); }
  if (mcmc::check_stepsize(np, p.stepsize, &p.nfree) || p.nfree < 1) return 3;
  const int n = p.nfree;
  const size_t rows = fit::max_rows(S, n, K), rec = np + 4;
  std::vector<double> chisq(S), lambda(S), D((size_t)S * np), cur((size_t)S * nd), jrows((size_t)S * n * np),
      trows((size_t)S * K * np), band(rows * nd), trace((size_t)S * (p.maxiter + 1) * rec, 0.0),
      work(fit::kWorkBytes / sizeof(double) + 1);
  std::vector<int> status(S), valid(S), mstatus(rows);
  std::vector<long> niter(S), nbad((size_t)S * 4);
  p.x = x.data(); p.chisq = chisq.data(); p.lambda = lambda.data(); p.D = D.data(); p.cur = cur.data();
  p.status = status.data(); p.valid = valid.data(); p.niter = niter.data(); p.nbad = nbad.data();
  p.jrows = jrows.data(); p.trows = trows.data(); p.band = band.data(); p.mstatus = mstatus.data();
  p.trace = trace.data();
  const fit::Work w = fit::carve(work.data());
  auto model = [&](const double *r, int m) {
    for (int i = 0; i < m; i++) {
      const double *q = r + (size_t)i * np;
      double *b = band.data() + (size_t)i * nd;
      mstatus[i] = reject_par >= 0 && q[reject_par] + (reject_par2 >= 0 ? q[reject_par2] : 0.0) > reject_above ? 1 : 0;
      for (int f = 0; f < nd; f++) {
        double v = 0.0;
        if (model_id == 0)
          for (int j = 0; j < np; j++) v += aux[(size_t)f * np + j] * q[j];
        else if (model_id == 1)
          v = q[0] * std::exp(-q[1] * aux[f]) + q[2];
        else
          v = f == 0 ? 10.0 * (q[1] - q[0] * q[0]) : 1.0 - q[0];
        b[f] = mstatus[i] ? -1.0 : v;
      }
    }
  };
  std::FILE *out = std::fopen(out_path, "wb");
  if (!out) return 2;
  auto put = [&](const double *v, size_t m) { std::fwrite(v, sizeof(double), m, out); };
  auto put_ints = [&](auto &v) {
    const std::vector<double> d(v.begin(), v.end());
    put(d.data(), d.size());
  };
  std::vector<double> iters;   // what every solve left, in order
  long made = 0;
  for (int s = 0; s < S; s++) mcmc::copy_shared(np, p.stepsize, p.x + (size_t)s * np);
  model(p.x, S);
  for (int s = 0; s < S; s++) fit::pick_start(p, s, 0);
  for (long it = 1; it <= p.maxiter; it++) {
    bool any = false;
    for (int s = 0; s < S; s++) any = any || status[s] == fit::kRunning;
    if (!any) break;
    model(p.jrows, S * n);
    for (int s = 0; s < S; s++) fit::solve_start(p, w, s, fit::HostExec{});
    iters.insert(iters.end(), trows.begin(), trows.end());
    iters.insert(iters.end(), valid.begin(), valid.end());
    iters.insert(iters.end(), D.begin(), D.end());
    model(p.trows, S * K);
    for (int s = 0; s < S; s++) fit::pick_start(p, s, it);
    made = it;
  }
  // records past the last pick repeat it
  for (int s = 0; s < S; s++)
    for (long it = made + 1; it <= p.maxiter; it++) {
      double *to = trace.data() + ((size_t)s * (p.maxiter + 1) + it) * rec;
      for (size_t k = 0; k < rec; k++) to[k] = to[k - rec];
      to[np + 2] = -1.0;
    }
  const double dmade = (double)made, ok = 1.0;
  put(&dmade, 1);
  put(trace.data(), trace.size());
  put(iters.data(), iters.size());
  put(x.data(), x.size());
  put(chisq.data(), chisq.size());
  put_ints(status);
  put_ints(niter);
  put_ints(nbad);
  put(&ok, 1);
  std::fclose(out);
  return 0;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "check" && argc >= 3) {
    const int np = std::atoi(argv[2]);
    if (np < 1 || argc != 3 + np) return 2;
    std::vector<double> st(np);
    for (int j = 0; j < np; j++) st[j] = std::atof(argv[3 + j]);
    int nfree = 0;
    std::printf("%d\n", mcmc::check_stepsize(np, st.data(), &nfree));
    return 0;
  }
  if (mode == "run" && argc == 4) return run(argv[2], argv[3]);
  std::fprintf(stderr, "usage: see the head of tests/fit_core_host.cpp\n");
  return 2;
}
