// Stand-alone host program over bart_amd/csrc/mcmc_core.hpp and grid_core.hpp, built and run by
// tests/test_walks_core_cpu.py (a host compiler alone, with the address and undefined-behaviour sanitizers): the
// Metropolis random walk through the very propose / finish functions the device kernel runs, over an analytic model
// band = A p, and the samples of a model grid.
//
//   walks_core_host draws SEED T NCH NPARS        draws_row of every chain (%a, one line per chain)
//   walks_core_host run PROBLEM OUT               the loop on the problem file; results as raw doubles in OUT
//   walks_core_host grid SEED T NROWS NPARS params[NPARS] pmin[NPARS] pmax[NPARS] stepsize[NPARS]
//                                                 grid::sample of every row (%a, one line per row)
//
// PROBLEM (text, whitespace separated): nch npars ndata nsteps walk seed thin reject_par reject_above has_prior, then
// params pmin pmax stepsize prior priorlow priorup [npars each], data uncert [ndata each], A [ndata][npars].  The
// model rejects (status 1, band -1) a row whose parameter reject_par exceeds reject_above (reject_par < 0: never).
// OUT: chain [nch][nkept][npars], chisq [nch][nkept], models [nch][nkept][ndata], accepted [nsteps][nch] (0 / 1),
// counts [nch][4], then 1.0 (or 0.0 and nothing else when no chain starts on a physical model).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../bart_amd/csrc/grid_core.hpp"
#include "../bart_amd/csrc/mcmc_core.hpp"

using namespace bartrt::mcmc;

static int run(const char *problem, const char *out_path) {
  std::ifstream in(problem);
  State s{};
  int reject_par, has_prior;
  double reject_above;
  in >> s.nch >> s.npars >> s.ndata >> s.nsteps >> s.walk >> s.seed >> s.thin >> reject_par >> reject_above >> has_prior;
  if (!in || s.nch < 1 || s.npars < 1 || s.npars > kMaxPars || s.ndata < 1 || s.nsteps < 1 || s.thin < 1) return 2;
  const int nch = s.nch, np = s.npars, nd = s.ndata;
  auto read = [&](size_t n) {
    std::vector<double> v(n);
    for (double &d : v) in >> d;
    return v;
  };
  const std::vector<double> params = read(np), pmin = read(np), pmax = read(np), stepsize = read(np),
                            prior = read(np), priorlow = read(np), priorup = read(np), data = read(nd),
                            uncert = read(nd), A = read((size_t)nd * np);
  if (!in) return 2;
  s.pmin = pmin.data(); s.pmax = pmax.data(); s.stepsize = stepsize.data();
  s.data = data.data(); s.uncert = uncert.data();
  if (has_prior) { s.prior = prior.data(); s.priorlow = priorlow.data(); s.priorup = priorup.data(); }
  if (bartrt::check_stepsize(np, s.stepsize, &s.nfree)) return 3;
  const long nkept = kept_rows(s.nsteps, s.thin);
  std::vector<double> x((size_t)nch * np), c(nch), cur((size_t)nch * nd), logjac(nch), prop((size_t)nch * np),
      band((size_t)nch * nd), chain((size_t)nch * nkept * np), chisq((size_t)nch * nkept),
      models((size_t)nch * nkept * nd), accepted((size_t)s.nsteps * nch);
  std::vector<int> inside(nch), status(nch);
  std::vector<long> counts((size_t)nch * 4, 0);
  s.x = x.data(); s.c = c.data(); s.cur = cur.data(); s.logjac = logjac.data(); s.inside = inside.data();
  s.counts = counts.data(); s.prop = prop.data(); s.band = band.data(); s.status = status.data();
  s.chain = chain.data(); s.chisq = chisq.data(); s.models = models.data();
  auto model = [&](const double *rows, int n, double *b, int *st) {
    for (int i = 0; i < n; i++) {
      const double *p = rows + (size_t)i * np;
      st[i] = reject_par >= 0 && p[reject_par] > reject_above ? 1 : 0;
      for (int f = 0; f < nd; f++) {
        double v = 0.0;
        for (int j = 0; j < np; j++) v += A[(size_t)f * np + j] * p[j];
        b[(size_t)i * nd + f] = st[i] ? -1.0 : v;
      }
    }
  };
  std::FILE *out = std::fopen(out_path, "wb");
  if (!out) return 2;
  const double ok = start_population(s, params.data(), model, status.data(), nullptr) ? 1.0 : 0.0;
  if (ok != 0.0) {
    for (long t = 0; t < s.nsteps; t++) {
      for (int i = 0; i < nch; i++) propose(s, t, i);
      model(prop.data(), nch, band.data(), status.data());
      for (int i = 0; i < nch; i++) {
        const long before = counts[(size_t)i * 4];
        finish(s, t, i);
        accepted[(size_t)t * nch + i] = (double)(counts[(size_t)i * 4] - before);
      }
    }
    std::vector<double> cnt(counts.begin(), counts.end());
    std::fwrite(chain.data(), sizeof(double), chain.size(), out);
    std::fwrite(chisq.data(), sizeof(double), chisq.size(), out);
    std::fwrite(models.data(), sizeof(double), models.size(), out);
    std::fwrite(accepted.data(), sizeof(double), accepted.size(), out);
    std::fwrite(cnt.data(), sizeof(double), cnt.size(), out);
  }
  std::fwrite(&ok, sizeof(double), 1, out);
  std::fclose(out);
  return 0;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "draws" && argc == 6) {
    const unsigned long long seed = std::strtoull(argv[2], nullptr, 0), t = std::strtoull(argv[3], nullptr, 0);
    const int nch = std::atoi(argv[4]), np = std::atoi(argv[5]);
    if (nch < 1 || np < 1 || np > kMaxPars) return 2;
    std::vector<double> row(kDrawsHead + np);
    for (int i = 0; i < nch; i++) {
      draws_row(seed, t, nch, i, np, row.data());
      for (double v : row) std::printf("%a ", v);
      std::printf("\n");
    }
    return 0;
  }
  if (mode == "grid" && argc >= 6) {
    const unsigned long long seed = std::strtoull(argv[2], nullptr, 0), t = std::strtoull(argv[3], nullptr, 0);
    const int nrows = std::atoi(argv[4]), np = std::atoi(argv[5]);
    if (nrows < 1 || np < 1 || np > kMaxPars || argc != 6 + 4 * np) return 2;
    std::vector<double> v(4 * (size_t)np), row(np);
    for (size_t k = 0; k < v.size(); k++) v[k] = std::strtod(argv[6 + k], nullptr);
    const double *params = v.data(), *pmin = params + np, *pmax = pmin + np, *stepsize = pmax + np;
    if (bartrt::check_stepsize(np, stepsize, nullptr)) return 3;
    if (bartrt::grid::check_box(np, pmin, pmax, stepsize)) return 4;
    for (int i = 0; i < nrows; i++) {
      bartrt::grid::sample(seed, t, i, np, params, pmin, pmax, stepsize, row.data());
      for (double x : row) std::printf("%a ", x);
      std::printf("\n");
    }
    return 0;
  }
  if (mode == "run" && argc == 4) return run(argv[2], argv[3]);
  std::fprintf(stderr, "usage: see the head of tests/walks_core_host.cpp\n");
  return 2;
}
