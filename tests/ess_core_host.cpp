// Host program of tests/test_ess_core_cpu.py and tests/test_gpu_mcmc_ess.py: bart_amd/csrc/ess_core.hpp built by a host
// compiler alone, run on a chain the test wrote.
//
//   ess_core_host IN OUT       ess::statistic, the very functions the device kernels run
//
// IN (doubles): nch nkept npars r0 r1 maxlag target, stepsize[npars], chain[nch][nkept][npars].
// OUT (doubles): tau[nch][npars], ess[npars], truncated[nch][npars], acf[nch][npars][K + 1] (K = min(maxlag, n - 1),
// maxlag 0 read as the default; no entry where K < 0), mean[nch][npars] (the mean every difference was taken about; 0
// for a parameter that is not free or where there is no test), reached, 1.0 (written last).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../bart_amd/csrc/ess_core.hpp"

using namespace bartrt;

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  double head[7];
  if (std::fread(head, sizeof(double), 7, f) != 7) return 4;
  const int nch = (int)head[0], npars = (int)head[2];
  const long nkept = (long)head[1], r0 = (long)head[3], r1 = (long)head[4], maxlag = (long)head[5];
  if (nch < 1 || npars < 1 || npars > kMaxPars || nkept < 1 || r0 < 0 || r1 < r0 || r1 > nkept) return 5;
  if (maxlag < 0 || maxlag > ess::kMaxLag) return 5;
  std::vector<double> stepsize(npars), chain((size_t)nch * nkept * npars);
  if (std::fread(stepsize.data(), sizeof(double), stepsize.size(), f) != stepsize.size()) return 6;
  if (std::fread(chain.data(), sizeof(double), chain.size(), f) != chain.size()) return 7;
  std::fclose(f);
  const size_t pairs = (size_t)nch * npars;
  const long K = ess::lags(ess::maxlag_of(maxlag), r1 - r0);
  const size_t nacf = K >= 0 ? pairs * (size_t)(K + 1) : 0;
  std::vector<double> tau(pairs), stat(npars), acf(nacf), mean(pairs, 0.0);
  std::vector<int> truncated(pairs);
  const int reached = ess::statistic(chain.data(), nch, nkept, npars, stepsize.data(), r0, r1, maxlag, head[6],
                                     tau.data(), stat.data(), truncated.data(), nacf ? acf.data() : nullptr);
  if (ess::testable(r0, r1))
    for (int i = 0; i < nch; i++)
      for (int j = 0; j < npars; j++)
        if (stepsize[j] > 0) mean[(size_t)i * npars + j] = ess::mean(chain.data(), nkept, npars, r0, r1, i, j);
  std::vector<double> out;
  out.insert(out.end(), tau.begin(), tau.end());
  out.insert(out.end(), stat.begin(), stat.end());
  out.insert(out.end(), truncated.begin(), truncated.end());
  out.insert(out.end(), acf.begin(), acf.end());
  out.insert(out.end(), mean.begin(), mean.end());
  out.push_back(reached);
  out.push_back(1.0);
  f = std::fopen(argv[2], "wb");
  if (!f) return 8;
  const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  return std::fclose(f) == 0 && ok ? 0 : 9;
}
