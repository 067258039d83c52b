// Stand-alone host program over the grouped sampler's host-buildable parts, built and run by
// tests/test_mcmc_groups_cpu.py (a host compiler alone, with the address and undefined-behaviour sanitizers):
// mcmc::group_state / start_groups of bart_amd/csrc/mcmc_core.hpp and check_groups / check_problem of
// bart_amd/csrc/retrieval_check.hpp.  It drives G groups the way the device loop does -- common arrays, group g's State
// a slice of them, one model call per iteration over all G nch rows -- over an analytic model band = A p.
//
//   mcmc_groups_host run PROBLEM OUTSTEM     the grouped loop; group g's results as raw doubles in OUTSTEM.g
//   mcmc_groups_host check G NCH BAD         check_groups on G problems of 7 parameters, group BAD (if >= 0) with
//                                            stepsize[6] = -7: prints "ok" or the refusal's message
//
// PROBLEM (text, whitespace separated): G nch npars ndata nsteps snooker thin reject_par reject_above, then per group
// seed and params pmin pmax stepsize prior priorlow priorup [npars each], data uncert [ndata each]; then A
// [ndata][npars].  The model is tests/mcmc_core_host.cpp's, and OUTSTEM.g has that program's layout: chain
// [nch][nkept][npars], chisq [nch][nkept], models [nch][nkept][ndata], accepted [nsteps][nch], counts [nch][4], then
// 1.0 (or 0.0 alone where no chain of the group starts on a physical model).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../bart_amd/csrc/retrieval_check.hpp"

using namespace bartrt;
using namespace bartrt::mcmc;

struct GroupInput {
  unsigned long long seed;
  std::vector<double> params, pmin, pmax, stepsize, prior, priorlow, priorup, data, uncert;
};

static int run(const char *problem, const std::string &stem) {
  std::ifstream in(problem);
  State all{};
  int G, np, nd, reject_par;
  double reject_above;
  in >> G >> all.nch >> np >> nd >> all.nsteps >> all.snooker >> all.thin >> reject_par >> reject_above;
  if (!in || !groups_fit(G, all.nch) || np < 1 || np > kMaxPars || nd < 1 || all.nsteps < 1 || all.thin < 1) return 2;
  const int nch = all.nch;
  auto read = [&](size_t n) {
    std::vector<double> v(n);
    for (double &d : v) in >> d;
    return v;
  };
  std::vector<GroupInput> input(G);
  for (GroupInput &gi : input) {
    in >> gi.seed;
    gi.params = read(np); gi.pmin = read(np); gi.pmax = read(np); gi.stepsize = read(np);
    gi.prior = read(np); gi.priorlow = read(np); gi.priorup = read(np); gi.data = read(nd); gi.uncert = read(nd);
  }
  const std::vector<double> A = read((size_t)nd * np);
  if (!in) return 2;
  std::vector<Objective> stated;
  for (const GroupInput &gi : input)
    stated.push_back(Objective{np, nd, 0, gi.pmin.data(), gi.pmax.data(), gi.stepsize.data(), gi.data.data(),
                               gi.uncert.data(), gi.prior.data(), gi.priorlow.data(), gi.priorup.data()});
  const std::vector<Objective> checked = check_groups("mcmc_groups_host", G, nch, stated.data(), check_problem);

  // the common arrays, as the device loop lays them out
  const size_t N = (size_t)G * nch, nkept = (size_t)kept_rows(all.nsteps, all.thin);
  std::vector<double> x(N * np), c(N), cur(N * nd), logjac(N), prop(N * np), band(N * nd), chain(N * nkept * np),
      chisq(N * nkept), models(N * nkept * nd), accepted((size_t)all.nsteps * N);
  std::vector<int> inside(N), status(N);
  std::vector<long> counts(N * 4, 0);
  all.x = x.data(); all.c = c.data(); all.cur = cur.data(); all.logjac = logjac.data(); all.inside = inside.data();
  all.counts = counts.data(); all.prop = prop.data(); all.band = band.data(); all.status = status.data();
  all.chain = chain.data(); all.chisq = chisq.data(); all.models = models.data();
  std::vector<State> gs;
  std::vector<const double *> params;
  for (int g = 0; g < G; g++) {
    gs.push_back(group_state(all, g, checked[g], input[g].seed));
    params.push_back(input[g].params.data());
  }
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
  std::vector<char> ok(G);
  start_groups(gs.data(), G, params.data(), model, status.data(), nullptr, ok.data());
  for (long t = 0; t < all.nsteps; t++) {
    for (int g = 0; g < G; g++)
      for (int i = 0; i < nch; i++) propose(gs[g], t, i);
    model(prop.data(), (int)N, band.data(), status.data());   // one batch over every group's rows
    for (int g = 0; g < G; g++)
      for (int i = 0; i < nch; i++) {
        const long before = gs[g].counts[(size_t)i * 4];
        finish(gs[g], t, i);
        accepted[((size_t)g * all.nsteps + t) * nch + i] = (double)(gs[g].counts[(size_t)i * 4] - before);
      }
  }
  for (int g = 0; g < G; g++) {
    std::FILE *out = std::fopen((stem + "." + std::to_string(g)).c_str(), "wb");
    if (!out) return 2;
    const double good = ok[g] ? 1.0 : 0.0;
    if (ok[g]) {
      const size_t r = (size_t)g * nch;
      const std::vector<double> cnt(counts.begin() + r * 4, counts.begin() + (r + nch) * 4);
      std::fwrite(chain.data() + r * nkept * np, sizeof(double), (size_t)nch * nkept * np, out);
      std::fwrite(chisq.data() + r * nkept, sizeof(double), (size_t)nch * nkept, out);
      std::fwrite(models.data() + r * nkept * nd, sizeof(double), (size_t)nch * nkept * nd, out);
      std::fwrite(accepted.data() + (size_t)g * all.nsteps * nch, sizeof(double), (size_t)all.nsteps * nch, out);
      std::fwrite(cnt.data(), sizeof(double), cnt.size(), out);
    }
    std::fwrite(&good, sizeof(double), 1, out);
    std::fclose(out);
  }
  return 0;
}

static int check(int G, int nch, int bad) {
  const double lo[7] = {-5, -5, -5, -5, -5, -5, -5}, hi[7] = {5, 5, 5, 5, 5, 5, 5}, one[3] = {1, 1, 1};
  const double good_step[7] = {0.1, 0.0, 0.0, 0.0, 0.1, 0.1, -6.0}, bad_step[7] = {0.1, 0.0, 0.0, 0.0, 0.1, 0.1, -7.0};
  std::vector<Objective> stated;
  for (int g = 0; g < (groups_fit(G, nch) ? G : 0); g++)   // (a refused count reads no problem)
    stated.push_back(Objective{7, 3, 0, lo, hi, g == bad ? bad_step : good_step, one, one, nullptr, nullptr, nullptr});
  try {
    const std::vector<Objective> got = check_groups("mcmc_groups_host", G, nch, stated.data(), check_problem);
    std::printf("ok %d groups, %d free\n", (int)got.size(), got.empty() ? 0 : got[0].nfree);
  } catch (const std::invalid_argument &err) {
    std::printf("%s\n", err.what());
  }
  return 0;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "run" && argc == 4) return run(argv[2], argv[3]);
  if (mode == "check" && argc == 5) return check(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
  std::fprintf(stderr, "usage: see the head of tests/mcmc_groups_host.cpp\n");
  return 2;
}
