// The integrated autocorrelation time and the effective sample size (ESS) of the resident sampler's chain, stated once
// for host and device (mcmc.hip: mcmc_ess_lags, mcmc_ess_finish; bartrt_mcmc_ess).  Plain inline functions on plain
// pointers, no HIP call, in the idiom of gr_core.hpp: the kernels run them, and a host compiler alone builds them for
// the CPU tests (tests/ess_core_host.cpp).
//
// INPUT.  chain[nch][nkept][npars] in the resident loop's layout, a row range [r0, r1) common to all chains with
// n = r1 - r0, stepsize[npars] and maxlag; parameter j is free where stepsize[j] > 0 (retrieval.hpp).
// K = min(maxlag, n - 1); maxlag 0 reads as kDefaultLag, more than kMaxLag is refused by the callers.
//
// MEAN.  For every chain i and free parameter j the mean m is gr_core.hpp's: the tiles' gr::leaf merged in ascending
// order by gr::merge.  It is not restated here.
//
// LAGGED SUMS.  For k = 0 ... K:  S_k = sum over r = r0 ... r1 - 1 - k of (x_r - m)(x_{r+k} - m).  THE ORDER IS FIXED
// HERE and depends on no launch shape: each S_k is accumulated in ONE accumulator in ascending row order; the two
// differences are formed first, then their product, then the add (lag_add), and nothing is contracted.  No sum of raw
// values or of raw squares is formed anywhere: gr_core.hpp's remark about a radius of 97 000 km holds here as well.
//
// AUTOCORRELATION TIME.  rho_k = S_k / S_0,  P_t = rho_{2t} + rho_{2t+1},  tau = -1 + 2 sum P_t over t = 0, 1, ...,
// stopping before the first P_t <= 0: Geyer's initial positive sequence (Geyer 1992, "Practical Markov chain Monte
// Carlo", Statist. Sci. 7, 473), written from the paper and not from MC3's source, which is absent from the reference
// checkout.  If the pairs run out at K (2t + 1 > K) before a non-positive one is met, the chain's entry is marked
// TRUNCATED and tau is the sum so far.  tau < 1 is kept as computed: no clamp.  S_0 = 0 (a constant column) gives what
// IEEE arithmetic gives: every rho is NaN, no P_t compares <= 0, so tau is NaN and the entry is truncated.
//
// ESS.  ess_j = sum over the chains, in chain order, of n / tau_ij.  REACHED means: there is a free parameter, every
// free ess_j is finite and >= the target, and no chain of a free parameter is truncated.  A NaN or an inf never counts.
//
// One chain is enough, unlike the Gelman-Rubin test.  There is a test when n >= gr::kMinRows; otherwise every output
// is zero.  Parameters that are not free give zeros.
#pragma once
#include "gr_core.hpp"

namespace bartrt {
namespace ess {

constexpr int kLanes = 256;          // lags per workgroup of mcmc_ess_lags (lane = lag) and rows per window step
constexpr long kDefaultLag = 1024;
constexpr long kMaxLag = 4096;

RETRIEVAL_HD bool testable(long r0, long r1) { return r0 >= 0 && r1 - r0 >= gr::kMinRows; }
// (0 reads as the default)
RETRIEVAL_HD long maxlag_of(long maxlag) { return maxlag == 0 ? kDefaultLag : maxlag; }
// K of a range of n rows; maxlag as maxlag_of gives it
RETRIEVAL_HD long lags(long maxlag, long n) { return maxlag < n - 1 ? maxlag : n - 1; }

// the mean of rows [r0, r1) of chain i, parameter j: gr_core.hpp's tiles, merged in ascending order
RETRIEVAL_HD double mean(const double *chain, long nkept, int npars, long r0, long r1, int i, int j) {
  double a[3], b[3];
  gr::leaf(chain, nkept, npars, r0, r1, i, 0, j, a);
  for (long k = 1; k < gr::tiles(r0, r1); k++) {
    gr::leaf(chain, nkept, npars, r0, r1, i, k, j, b);
    gr::merge(a, b);
  }
  return a[1];
}

RETRIEVAL_HD double diff(double x, double m) {
  RETRIEVAL_EXACT
  return x - m;
}

// one term of a lagged sum: the product of two differences, rounded, then added
RETRIEVAL_HD double lag_add(double s, double da, double db) {
  RETRIEVAL_EXACT
  const double p = da * db;
  return s + p;
}

// S_k of one column (col[r * npars] is row r) about m
RETRIEVAL_HD double lagged_sum(const double *col, int npars, long r0, long r1, double m, long k) {
  double s = 0.0;
  for (long r = r0; r + k < r1; r++) s = lag_add(s, diff(col[(size_t)r * npars], m), diff(col[(size_t)(r + k) * npars], m));
  return s;
}

// tau of one chain and parameter from S[0 .. K]; *truncated set or cleared
RETRIEVAL_HD double tau_of(const double *S, long K, int *truncated) {
  RETRIEVAL_EXACT
  const double s0 = S[0];
  double sum = 0.0;
  int stopped = 0;
  for (long t = 0; 2 * t + 1 <= K; t++) {
    const double a = S[2 * t] / s0, b = S[2 * t + 1] / s0, p = a + b;
    if (p <= 0.0) {
      stopped = 1;
      break;
    }
    sum = sum + p;
  }
  *truncated = !stopped;
  return -1.0 + 2.0 * sum;
}

// ess of one parameter from the chains' tau[nch][stride doubles apart]
RETRIEVAL_HD double ess_of(const double *tau, size_t stride, int nch, long n) {
  RETRIEVAL_EXACT
  double e = 0.0;
  for (int i = 0; i < nch; i++) e = e + (double)n / tau[i * stride];
  return e;
}

// ess[npars], truncated[nch][npars]
RETRIEVAL_HD int reached_of(const double *ess, const int *truncated, const double *stepsize, int nch, int npars,
                            double target) {
  int nfree = 0, ok = 1;
  for (int j = 0; j < npars; j++) {
    if (!(stepsize[j] > 0)) continue;
    nfree++;
    ok = ok && std::isfinite(ess[j]) && ess[j] >= target;
    for (int i = 0; i < nch; i++) ok = ok && !truncated[(size_t)i * npars + j];
  }
  return nfree > 0 && ok;
}

// The whole statistic in one place, for host code: tau[nch][npars], ess[npars], truncated[nch][npars], acf (may be
// null) [nch][npars][K + 1] = the S_k; returns reached.  maxlag as the caller gave it (0: the default).
inline int statistic(const double *chain, int nch, long nkept, int npars, const double *stepsize, long r0, long r1,
                     long maxlag, double target, double *tau, double *ess, int *truncated, double *acf) {
  const long n = r1 - r0, K = lags(maxlag_of(maxlag), n);
  for (int j = 0; j < npars; j++) ess[j] = 0.0;
  for (size_t q = 0; q < (size_t)nch * npars; q++) {
    tau[q] = 0.0;
    truncated[q] = 0;
  }
  if (acf && K >= 0)
    for (size_t q = 0; q < (size_t)nch * npars * (K + 1); q++) acf[q] = 0.0;
  if (!testable(r0, r1) || r1 > nkept) return 0;
  double *own = acf ? nullptr : new double[K + 1];
  for (int i = 0; i < nch; i++)
    for (int j = 0; j < npars; j++) {
      if (!(stepsize[j] > 0)) continue;
      const size_t q = (size_t)i * npars + j;
      double *S = acf ? acf + q * (K + 1) : own;
      const double m = mean(chain, nkept, npars, r0, r1, i, j);
      const double *col = chain + (size_t)i * nkept * npars + j;
      for (long k = 0; k <= K; k++) S[k] = lagged_sum(col, npars, r0, r1, m, k);
      tau[q] = tau_of(S, K, truncated + q);
    }
  delete[] own;
  for (int j = 0; j < npars; j++)
    if (stepsize[j] > 0) ess[j] = ess_of(tau + j, (size_t)npars, nch, n);
  return reached_of(ess, truncated, stepsize, nch, npars, target);
}

}  // namespace ess
}  // namespace bartrt
