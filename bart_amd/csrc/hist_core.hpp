// Marginal histograms of the columns of a matrix, their range and the highest-density region of a histogram, stated
// once for host and device (hist.hip: hist_bin, hist_pairs, hist_range; bartrt_marginals, bartrt_marginals_range,
// bartrt_hpd).  Plain inline functions on plain pointers, no HIP call, in the idiom of gr_core.hpp and quant_core.hpp:
// the kernels run them, and a host compiler alone builds them for the CPU tests (tests/hist_core_host.cpp).
//
// BINNING.  For strictly increasing finite edges e[0 .. nbins] a value x falls in bin i iff e[i] <= x < e[i + 1], and
// x == e[nbins] falls in bin nbins - 1.  Everything else is classified, not dropped: x < e[0] (and -inf) is BELOW,
// x > e[nbins] (and +inf) is ABOVE, a NaN is NAN.  The edges need not be uniform.  The DECISION is always the
// comparison of x with the edges themselves: classify() first guesses a bin from a uniform grid over [e[0], e[nbins]]
// (one multiply), accepts the guess only if e[g] <= x < e[g + 1] holds, and otherwise finds the bin by bisection over
// the edges.  A wrong guess costs time, never a count.  -0.0 and +0.0 compare equal, so with an edge at 0.0 both fall
// in the bin that starts there.  This is what np.histogram and np.histogram2d count, given the same edges, integer
// for integer (numpy corrects its own uniform estimate against the edges, and np.histogram2d searches them).
//
// PAIRS.  A row counts in the pair (a, b) iff both of its values are in range: np.histogram2d's behaviour.
//
// ORDER.  Counts are integers; the kernels add them with LDS and global integer atomics, whose result is the same in
// any order.  No floating-point number is accumulated anywhere.
//
// RANGE.  The smallest and the largest FINITE value of a column among the rows that count, and the number of finite
// values, through quant_core.hpp's order-preserving 64-bit keys: the minimum and maximum of keys are exact and
// associative, so any reduction order gives the same bits.  -0.0 orders before +0.0: a column of both has lo = -0.0
// and hi = +0.0.  No finite value: NaN, NaN, 0.
//
// HPD.  The highest-density region of a histogram counts[nbins] at a fraction 0 < p <= 1: order the bins by
// descending count, ties by ascending index; take the shortest prefix whose cumulative count c satisfies
// (double)c >= p * (double)N, N the sum of the counts.  The region is the set of those bins: mask[nbins], the threshold
// (the smallest count included), the included total and the number of maximal runs of included bins (2 for a bimodal
// histogram cut between its modes).  N = 0: an empty mask and zeros.  This is MC3's credible region taken on the
// HISTOGRAM instead of on a kernel density estimate: MC3 smooths the samples with a Gaussian KDE and thresholds the
// density; here the density is the bin count (kde_core.hpp builds the KDE and takes the region on it with hpd_of).
#pragma once
#include <algorithm>
#include <vector>

#include "quant_core.hpp"

namespace bartrt {
namespace hist {

constexpr int kMaxSel = kMaxPars;        // selected columns of one call (the parameter limit of bartrt_mcmc_gr)
constexpr int kMaxBins = 1024;           // bins of a marginal
constexpr int kMaxPairBins = 128;        // with pairs: 128 x 128 32-bit cells are the 64 kB a workgroup has by default
// what classify returns besides a bin
constexpr int kBelow = -1, kAbove = -2, kNan = -3;
// the compact bin index the pair kernel reads: a bin, or "does not count" (out of range, NaN, a masked row)
constexpr unsigned short kNotCounted = 0xffffu;
static_assert(kMaxBins < kNotCounted, "a bin index fits 16 bits beside the sentinel");

// the uniform grid's scale for a guess, nbins / (e[nbins] - e[0]); any value, inf and NaN included, is harmless
RETRIEVAL_HD double guess_scale(const double *e, int nbins) { return (double)nbins / (e[nbins] - e[0]); }

// The bin of x among e[0 .. nbins] (BINNING above), or kBelow / kAbove / kNan.  scale: guess_scale(e, nbins).
RETRIEVAL_HD int classify(double x, const double *e, int nbins, double scale) {
  if (x != x) return kNan;
  if (x < e[0]) return kBelow;
  if (x >= e[nbins]) return x > e[nbins] ? kAbove : nbins - 1;
  // e[0] <= x < e[nbins]: the guess, checked against the edges
  const double t = (x - e[0]) * scale;
  int g = !(t >= 0.0) ? 0 : (t >= (double)nbins ? nbins - 1 : (int)t);
  if (e[g] <= x && x < e[g + 1]) return g;
  // bisection: the largest i with e[i] <= x
  int lo = 0, hi = nbins;                // e[lo] <= x < e[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// are e[0 .. nbins] finite and strictly increasing ?  The index of the first edge that is not, or -1.
inline int bad_edge(const double *e, int nbins) {
  for (int i = 0; i <= nbins; i++) {
    const uint64_t b = quant::bits_of(e[i]);
    if ((b & quant::kExp) == quant::kExp) return i;          // inf or NaN
    if (i > 0 && !(e[i - 1] < e[i])) return i;
  }
  return -1;
}

// the range's running state: keys of the smallest and largest finite value, and their number
struct Range {
  uint64_t lo = ~0ull, hi = 0ull, n = 0ull;
};
RETRIEVAL_HD bool is_finite(double x) { return (quant::bits_of(x) & quant::kExp) != quant::kExp; }
RETRIEVAL_HD void range_add(Range &r, double x) {
  if (!is_finite(x)) return;
  const uint64_t k = quant::key_of(x);
  if (k < r.lo) r.lo = k;
  if (k > r.hi) r.hi = k;
  r.n++;
}
RETRIEVAL_HD double range_value(uint64_t key, uint64_t n) {
  return n ? quant::value_of(key) : quant::double_of(quant::kExp | (quant::kExp >> 1));
}

// Host restatement of the kernels for tests: x[nrows][ld], ok[nrows] or null, cols[nsel], edges[nsel][nbins + 1] ->
// h1[nsel][nbins], out[nsel][3] (below, above, NaN) and, h2 not null, h2[npairs][nbins][nbins] over a < b, a-major.
inline void marginals(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols, int nbins,
                      const double *edges, uint64_t *h1, uint64_t *out, uint64_t *h2) {
  const long npairs = (long)nsel * (nsel - 1) / 2;
  std::fill(h1, h1 + (size_t)nsel * nbins, 0ull);
  std::fill(out, out + (size_t)nsel * 3, 0ull);
  if (h2) std::fill(h2, h2 + (size_t)npairs * nbins * nbins, 0ull);
  std::vector<int> bin((size_t)nsel);
  for (long r = 0; r < nrows; r++) {
    if (ok && !ok[r]) continue;
    for (int s = 0; s < nsel; s++) {
      const double *e = edges + (size_t)s * (nbins + 1);
      const int b = classify(x[(size_t)r * ld + cols[s]], e, nbins, guess_scale(e, nbins));
      bin[s] = b;
      if (b >= 0) h1[(size_t)s * nbins + b]++; else out[(size_t)s * 3 + (-1 - b)]++;
    }
    if (!h2) continue;
    size_t p = 0;
    for (int a = 0; a < nsel; a++)
      for (int b = a + 1; b < nsel; b++, p++)
        if (bin[a] >= 0 && bin[b] >= 0) h2[(p * nbins + bin[a]) * nbins + bin[b]]++;
  }
}

// the same for the range: lohi[nsel][2], nfinite[nsel]
inline void marginals_range(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols,
                            double *lohi, uint64_t *nfinite) {
  for (int s = 0; s < nsel; s++) {
    Range g;
    for (long r = 0; r < nrows; r++)
      if (!ok || ok[r]) range_add(g, x[(size_t)r * ld + cols[s]]);
    lohi[2 * s] = range_value(g.lo, g.n);
    lohi[2 * s + 1] = range_value(g.hi, g.n);
    nfinite[s] = g.n;
  }
}

// HPD above, for counts (T = uint64_t) and for a density on a grid (T = double; kde_core.hpp states that rule).  The
// total is the last cumulative sum IN THE DESCENDING ORDER: for integers any order gives the same number, for doubles
// this one is the rule.  nbins >= 1, 0 < p <= 1 and values that are neither negative nor NaN are the caller's to check.
template <class T>
inline void hpd_of(const T *counts, int nbins, double p, unsigned char *mask, T *threshold, T *included, int *nruns) {
  std::fill(mask, mask + nbins, (unsigned char)0);
  *threshold = *included = 0;
  *nruns = 0;
  std::vector<int> order((size_t)nbins);
  for (int i = 0; i < nbins; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return counts[a] != counts[b] ? counts[a] > counts[b] : a < b; });
  T N = 0;
  for (int k = 0; k < nbins; k++) N += counts[order[k]];
  if (N == 0) return;
  const double want = p * (double)N;
  T c = 0;
  for (int k = 0; k < nbins; k++) {
    const int i = order[k];
    mask[i] = 1;
    c += counts[i];
    *threshold = counts[i];
    if ((double)c >= want) break;
  }
  *included = c;
  for (int i = 0; i < nbins; i++) *nruns += mask[i] && (i == 0 || !mask[i - 1]);
}

inline void hpd(const uint64_t *counts, int nbins, double p, unsigned char *mask, uint64_t *threshold, uint64_t *included,
                int *nruns) {
  hpd_of(counts, nbins, p, mask, threshold, included, nruns);
}

}  // namespace hist
}  // namespace bartrt
