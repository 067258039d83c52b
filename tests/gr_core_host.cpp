// Host program of tests/test_gr_core_cpu.py and tests/test_gpu_mcmc_converge.py: bart_amd/csrc/gr_core.hpp built by a
// host compiler alone, run on a chain the test wrote.
//
//   gr_core_host stat IN OUT       gr::statistic, the very functions the device kernels run
//   gr_core_host onepass IN OUT    the same statistic from per-chain sums of x and x^2 in one pass: what the header
//                                  forbids, here so that the accuracy test can show that it would catch it
//
// IN (doubles): nch nkept npars r0 r1 threshold, stepsize[npars], chain[nch][nkept][npars].
// OUT (doubles): psrf[npars], triples[nch][npars][3], converged, 1.0 (written last).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../bart_amd/csrc/gr_core.hpp"

using namespace bartrt;

static int onepass(const double *chain, int nch, long nkept, int npars, const double *stepsize, long r0, long r1,
                   double threshold, double *psrf, double *triples) {
  if (!gr::testable(nch, r0, r1)) return 0;
  const double n = (double)(r1 - r0);
  for (int i = 0; i < nch; i++)
    for (int j = 0; j < npars; j++) {
      if (!(stepsize[j] > 0)) continue;
      double s = 0.0, ss = 0.0;
      for (long r = r0; r < r1; r++) {
        const double x = chain[((size_t)i * nkept + r) * npars + j];
        s += x;
        ss += x * x;
      }
      double *t = triples + ((size_t)i * npars + j) * 3;
      t[0] = n;
      t[1] = s / n;
      t[2] = ss - s * s / n;
    }
  for (int j = 0; j < npars; j++)
    if (stepsize[j] > 0) psrf[j] = gr::psrf_of(triples + (size_t)j * 3, (size_t)npars * 3, nch);
  return gr::converged_of(psrf, stepsize, npars, gr::threshold_of(threshold));
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  double head[6];
  if (std::fread(head, sizeof(double), 6, f) != 6) return 4;
  const int nch = (int)head[0], npars = (int)head[2];
  const long nkept = (long)head[1], r0 = (long)head[3], r1 = (long)head[4];
  if (nch < 1 || npars < 1 || npars > kMaxPars || nkept < 1 || r0 < 0 || r1 < r0 || r1 > nkept) return 5;
  std::vector<double> stepsize(npars), chain((size_t)nch * nkept * npars);
  if (std::fread(stepsize.data(), sizeof(double), stepsize.size(), f) != stepsize.size()) return 6;
  if (std::fread(chain.data(), sizeof(double), chain.size(), f) != chain.size()) return 7;
  std::fclose(f);
  std::vector<double> out((size_t)npars + (size_t)nch * npars * 3 + 2, 0.0);
  double *psrf = out.data(), *triples = psrf + npars;
  int converged;
  if (!std::strcmp(argv[1], "stat"))
    converged = gr::statistic(chain.data(), nch, nkept, npars, stepsize.data(), r0, r1, head[5], psrf, triples);
  else if (!std::strcmp(argv[1], "onepass"))
    converged = onepass(chain.data(), nch, nkept, npars, stepsize.data(), r0, r1, head[5], psrf, triples);
  else
    return 2;
  out[out.size() - 2] = converged;
  out[out.size() - 1] = 1.0;
  f = std::fopen(argv[3], "wb");
  if (!f) return 8;
  const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  return std::fclose(f) == 0 && ok ? 0 : 9;
}
