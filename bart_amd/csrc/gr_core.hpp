// The Gelman-Rubin convergence statistic of the resident sampler's chain, stated once for host and device (mcmc.hip:
// mcmc_gr_leaf, mcmc_gr_merge, mcmc_gr_finish; bartrt_mcmc_gr).  Plain inline functions on plain pointers, no HIP
// call: the kernels run them one lane per (chain, tile, parameter), per (chain, parameter) and per parameter, and a
// host compiler alone builds them for the CPU tests (tests/gr_core_host.cpp).
//
// INPUT.  chain[nch][nkept][npars] in the resident loop's layout, a row range [r0, r1) common to all chains, and
// stepsize[npars]; parameter j is free where stepsize[j] > 0 (retrieval.hpp).
//
// TRIPLES.  For every chain i and every free parameter j: (n, mean, M2) of the rows, M2 = sum (x - mean)^2.  THE
// SUMMATION ORDER IS FIXED HERE and does not depend on who runs it or on a launch shape:
//   - tile k holds the kTile consecutive rows r0 + k kTile ... (the last tile: up to r1).  Its mean is the sum of its
//     values in row order divided by their number; its M2 the sum, in row order, of (x - mean)^2: two passes.
//   - the tiles are merged in ascending order into the first one with the pairwise update (Chan, Golub & LeVeque 1983):
//       n = n_a + n_b;  d = mean_b - mean_a;  mean = mean_a + d n_b / n;  M2 = M2_a + (M2_b + d d n_a n_b / n)
//     with the products taken from the left and the division last ((d n_b) / n, (((d d) n_a) n_b) / n).
// No sum of squares of the values themselves is formed anywhere: a radius of 97 000 km that varies by a few km would
// lose every digit to it.
//
// STATISTIC.  Per free parameter, the sums over the chains in chain order:
//   W = (sum_i M2_i / (n - 1)) / nch
//   B = n (sum_i (mean_i - m)^2) / (nch - 1),   m = (sum_i mean_i) / nch
//   R = sqrt(((n - 1) / n W + B / n) / W)
// This is bart_amd/sampler.py's gelman_rubin, which is the formula as we recall it of MC3's
// gelmanrubin.convergetest; the MC3 submodule of the reference checkout is empty, so it could not be read there.
// psrf[j] = 0 for a parameter that is not free, and its triples are zeros.  W = 0 (a constant column) gives what IEEE
// arithmetic gives: NaN, or inf where B > 0.
//
// CONVERGED means: there is a free parameter, and every free R is finite and below the threshold.  A NaN or an inf
// never counts as converged.  The default threshold 1.01 is MC3's "within 1% of unity", likewise recalled and not
// read from its source.
//
// There is a test only with nch >= 2 and r1 - r0 >= kMinRows (the guard sampler.py has always applied); otherwise
// every output is zero.
#pragma once
#include "retrieval.hpp"

namespace bartrt {
namespace gr {

constexpr long kTile = 256;     // rows per tile
constexpr long kMinRows = 4;
constexpr double kThreshold = 1.01;
constexpr int kFinishLanes = 64;   // the finisher's workgroup: parameter j on lane j (kMaxPars of them at most)
static_assert(kFinishLanes >= kMaxPars, "one lane per parameter");

RETRIEVAL_HD bool testable(int nch, long r0, long r1) { return nch >= 2 && r0 >= 0 && r1 - r0 >= kMinRows; }
RETRIEVAL_HD long tiles(long r0, long r1) { return (r1 - r0 + kTile - 1) / kTile; }

// (n, mean, M2) of tile k of chain i, parameter j, into t[3]
RETRIEVAL_HD void leaf(const double *chain, long nkept, int npars, long r0, long r1, int i, long k, int j, double *t) {
  RETRIEVAL_EXACT
  const long lo = r0 + k * kTile, hi = lo + kTile < r1 ? lo + kTile : r1;
  const double *col = chain + (size_t)i * nkept * npars + j;
  double sum = 0.0;
  for (long r = lo; r < hi; r++) sum += col[(size_t)r * npars];
  const double n = (double)(hi - lo), mean = sum / n;
  double m2 = 0.0;
  for (long r = lo; r < hi; r++) {
    const double d = col[(size_t)r * npars] - mean;
    m2 += d * d;
  }
  t[0] = n;
  t[1] = mean;
  t[2] = m2;
}

// b merged into a
RETRIEVAL_HD void merge(double *a, const double *b) {
  RETRIEVAL_EXACT
  const double na = a[0], nb = b[0], n = na + nb, d = b[1] - a[1];
  a[1] = a[1] + (d * nb) / n;
  a[2] = a[2] + (b[2] + (((d * d) * na) * nb) / n);
  a[0] = n;
}

// R of one free parameter from the chains' triples t[nch][stride doubles apart]
RETRIEVAL_HD double psrf_of(const double *t, size_t stride, int nch) {
  RETRIEVAL_EXACT
  const double n = t[0];
  double w = 0.0, m = 0.0;
  for (int i = 0; i < nch; i++) {
    w += t[i * stride + 2] / (n - 1.0);
    m += t[i * stride + 1];
  }
  w = w / nch;
  m = m / nch;
  double b = 0.0;
  for (int i = 0; i < nch; i++) {
    const double d = t[i * stride + 1] - m;
    b += d * d;
  }
  b = n * b / (nch - 1);
  return sqrt(((n - 1.0) / n * w + b / n) / w);
}

// (0 reads as the default)
RETRIEVAL_HD double threshold_of(double threshold) { return threshold == 0.0 ? kThreshold : threshold; }

RETRIEVAL_HD int converged_of(const double *psrf, const double *stepsize, int npars, double threshold) {
  int nfree = 0, ok = 1;
  for (int j = 0; j < npars; j++) {
    if (!(stepsize[j] > 0)) continue;
    nfree++;
    ok = ok && std::isfinite(psrf[j]) && psrf[j] < threshold;
  }
  return nfree > 0 && ok;
}

// The whole statistic in one place, for host code: psrf[npars], triples[nch][npars][3]; returns converged.
inline int statistic(const double *chain, int nch, long nkept, int npars, const double *stepsize, long r0, long r1,
                     double threshold, double *psrf, double *triples) {
  for (int j = 0; j < npars; j++) psrf[j] = 0.0;
  for (size_t q = 0; q < (size_t)nch * npars * 3; q++) triples[q] = 0.0;
  if (!testable(nch, r0, r1) || r1 > nkept) return 0;
  for (int i = 0; i < nch; i++)
    for (int j = 0; j < npars; j++) {
      if (!(stepsize[j] > 0)) continue;
      double *a = triples + ((size_t)i * npars + j) * 3, b[3];
      leaf(chain, nkept, npars, r0, r1, i, 0, j, a);
      for (long k = 1; k < tiles(r0, r1); k++) {
        leaf(chain, nkept, npars, r0, r1, i, k, j, b);
        merge(a, b);
      }
    }
  for (int j = 0; j < npars; j++)
    if (stepsize[j] > 0) psrf[j] = psrf_of(triples + (size_t)j * 3, (size_t)npars * 3, nch);
  return converged_of(psrf, stepsize, npars, threshold_of(threshold));
}

}  // namespace gr
}  // namespace bartrt
