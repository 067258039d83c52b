// Stand-alone host program over bart_amd/csrc/mcmc_core.hpp, built and run by tests/test_mcmc_core_cpu.py (a host
// compiler alone, with the address and undefined-behaviour sanitizers).  It drives the same propose / finish functions
// the device kernel runs, one chain after the other, over an analytic model band = A p.
//
//   mcmc_core_host philox                         the known answers, one line of four words each
//   mcmc_core_host edges                          the uniforms of all-zero and all-ones words (%a)
//   mcmc_core_host draws SEED T NCH NPARS         draws_row of every chain (%a, one line per chain)
//   mcmc_core_host check NPARS s0 s1 ...          check_stepsize: 0 or 1 + the refused parameter
//   mcmc_core_host run PROBLEM OUT                the loop on the problem file; results as raw doubles in OUT
//
// PROBLEM (text, whitespace separated): nch npars ndata nsteps snooker seed thin reject_par reject_above, then
// params pmin pmax stepsize prior priorlow priorup [npars each], data uncert [ndata each], A [ndata][npars].  The
// model rejects (status 1, band -1) a row whose parameter reject_par exceeds reject_above (reject_par < 0: never).
// OUT: chain [nch][nkept][npars], chisq [nch][nkept], models [nch][nkept][ndata], accepted [nsteps][nch] (0 / 1),
// counts [nch][4], then 1.0 (or 0.0 and nothing else when no chain starts on a physical model).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../bart_amd/csrc/mcmc_core.hpp"

using namespace bartrt::mcmc;

static void print_words(Words c, uint32_t k0, uint32_t k1) {
  const Words o = philox4x32_10(c, k0, k1);
  std::printf("%08x %08x %08x %08x\n", o.w[0], o.w[1], o.w[2], o.w[3]);
}

static int run(const char *problem, const char *out_path) {
  std::ifstream in(problem);
  State s{};
  int reject_par;
  double reject_above;
  in >> s.nch >> s.npars >> s.ndata >> s.nsteps >> s.snooker >> s.seed >> s.thin >> reject_par >> reject_above;
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
  s.prior = prior.data(); s.priorlow = priorlow.data(); s.priorup = priorup.data();
  if (check_stepsize(np, s.stepsize, &s.nfree)) return 3;
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
  if (mode == "philox") {
    print_words({{0, 0, 0, 0}}, 0, 0);
    print_words({{~0u, ~0u, ~0u, ~0u}}, ~0u, ~0u);
    print_words({{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}}, 0xa4093822u, 0x299f31d0u);
    return 0;
  }
  if (mode == "edges") {
    std::printf("%a %a\n", uniform53(0, 0), uniform53(~0u, ~0u));
    return 0;
  }
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
  if (mode == "check" && argc >= 3) {
    const int np = std::atoi(argv[2]);
    if (np < 1 || argc != 3 + np) return 2;
    std::vector<double> st(np);
    for (int j = 0; j < np; j++) st[j] = std::atof(argv[3 + j]);
    int nfree = 0;
    std::printf("%d\n", check_stepsize(np, st.data(), &nfree));
    return 0;
  }
  if (mode == "run" && argc == 4) return run(argv[2], argv[3]);
  std::fprintf(stderr, "usage: see the head of tests/mcmc_core_host.cpp\n");
  return 2;
}
