// Exact order statistics of the columns of a matrix, and the percentile rule on top of them, stated once for host and
// device (quant.hip: quant_count, quant_walk; bartrt_colselect, bartrt_posterior_tp).  Plain inline functions on plain
// pointers, no HIP call, in the idiom of gr_core.hpp: the kernels run them, and a host compiler alone builds them for
// the CPU tests (tests/quant_core_host.cpp).
//
// KEYS.  A double is mapped to a 64-bit key whose unsigned order is the order np.sort gives doubles: the sign bit of
// a non-negative value is flipped, every bit of a negative value is flipped.  The keys then run -inf, the negatives,
// -0, +0, the positives, +inf.  NaN: np.sort puts every NaN, of either sign, behind +inf.  A NaN's sign bit is
// therefore cleared before the map, so that it lands above +inf's key; value_of gives back a NaN with the same payload
// and a clear sign bit.  Every other double, the two zeros and the denormals included, goes through the map and back
// unchanged, bit for bit.  Among themselves NaNs are ordered by payload, which np.sort leaves open.
//
// SELECTION.  The element of rank k (zero-based, among the n rows that count) is found digit by digit from the top:
// kPasses passes of kBits bits.  Pass p counts, for every value of digit p, the elements whose higher digits equal the
// prefix found so far (histogram), walks the counts to the bucket that holds rank k (walk), appends that digit to the
// prefix and keeps the rank inside the bucket.  After the last pass the prefix is the key of the answer.  Nothing is
// computed: the answer is one of the inputs, the value np.sort(col)[k] has, bit for bit (the two zeros apart, which
// compare equal and which np.sort may leave in either order).
//
// ORDER.  The counts are integers.  The kernels add them up with LDS and global integer atomics, whose result is the
// same in any order: the output depends on no launch shape, no slab size and no scheduling.
//
// PERCENTILES.  np.percentile's default (linear) method: the virtual index of percent q among n sorted values is
// v = (n - 1) (q / 100), its neighbours are lo = floor(v) and hi = min(lo + 1, n - 1), and the weight is w = v - lo.
// The value is numpy's own expression (numpy/lib/_function_base_impl.py, _lerp): a + (b - a) w where w < 0.5 and
// b - (b - a)(1 - w) otherwise, every operation rounded on its own (no contraction).
#pragma once
#include "retrieval.hpp"

namespace bartrt {
namespace quant {

constexpr int kBits = 4;                    // digit width
constexpr int kPasses = 64 / kBits;         // most significant digit first
constexpr int kBins = 1 << kBits;
constexpr int kMaxRanks = 16;               // ranks one selection call serves
constexpr int kMaxPercents = kMaxRanks / 2; // two ranks per percentile

constexpr uint64_t kSign = 0x8000000000000000ull;
constexpr uint64_t kExp = 0x7ff0000000000000ull;

RETRIEVAL_HD uint64_t bits_of(double x) {
  uint64_t b;
  __builtin_memcpy(&b, &x, sizeof b);
  return b;
}
RETRIEVAL_HD double double_of(uint64_t b) {
  double x;
  __builtin_memcpy(&x, &b, sizeof x);
  return x;
}
RETRIEVAL_HD bool is_nan_bits(uint64_t b) { return (b & ~kSign) > kExp; }

// the order-preserving key of a double's bits (KEYS above)
RETRIEVAL_HD uint64_t key_of_bits(uint64_t b) {
  if (is_nan_bits(b)) b &= ~kSign;
  return (b & kSign) ? ~b : (b | kSign);
}
RETRIEVAL_HD uint64_t key_of(double x) { return key_of_bits(bits_of(x)); }
// the inverse map
RETRIEVAL_HD uint64_t bits_of_key(uint64_t k) { return (k & kSign) ? (k & ~kSign) : ~k; }
RETRIEVAL_HD double value_of(uint64_t k) { return double_of(bits_of_key(k)); }

// digit p of a key (p = 0: the most significant), and the bits above it
RETRIEVAL_HD int shift_of(int p) { return 64 - kBits * (p + 1); }
RETRIEVAL_HD int digit(uint64_t k, int p) { return (int)((k >> shift_of(p)) & (uint64_t)(kBins - 1)); }
RETRIEVAL_HD uint64_t above(uint64_t k, int p) { return p == 0 ? 0 : k >> (shift_of(p) + kBits); }
// does the key carry the prefix found in passes 0 .. p - 1 ?
RETRIEVAL_HD bool matches(uint64_t k, uint64_t prefix, int p) { return above(k, p) == above(prefix, p); }
RETRIEVAL_HD uint64_t append(uint64_t prefix, int p, int d) { return prefix | ((uint64_t)d << shift_of(p)); }

// The walk over a digit histogram hist[kBins] (stride elements apart): the bucket that holds rank *k, and *k made the
// rank inside that bucket.  -1, *k unchanged, when the histogram holds *k elements or fewer (no such rank).
template <class Count>
RETRIEVAL_HD int walk(const Count *hist, size_t stride, long *k) {
  long r = *k;
  for (int d = 0; d < kBins; d++) {
    const long c = (long)hist[d * stride];
    if (r < c) {
      *k = r;
      return d;
    }
    r -= c;
  }
  return -1;
}

// Host selection of one column (col[r * stride] is row r, rows with ok[r] == 0 left out, ok may be null) by the
// passes above: the value of rank k, or a NaN when fewer than k + 1 rows count.  The kernels' restatement for tests.
inline double select(const double *col, size_t stride, long nrows, const unsigned char *ok, long k) {
  uint64_t prefix = 0;
  for (int p = 0; p < kPasses; p++) {
    long hist[kBins] = {0};
    for (long r = 0; r < nrows; r++) {
      if (ok && !ok[r]) continue;
      const uint64_t key = key_of(col[(size_t)r * stride]);
      if (matches(key, prefix, p)) hist[digit(key, p)]++;
    }
    const int d = walk(hist, 1, &k);
    if (d < 0) return double_of(kExp | (kExp >> 1));
    prefix = append(prefix, p, d);
  }
  return value_of(prefix);
}

// np.percentile's linear rule (PERCENTILES above), n >= 1, 0 <= q <= 100
inline void percentile_rule(long n, double q, long *lo, long *hi, double *w) {
  RETRIEVAL_EXACT
  const double f = q / 100.0;
  const double v = (double)(n - 1) * f;
  long l = (long)std::floor(v);
  if (l < 0) l = 0;
  if (l > n - 1) l = n - 1;
  *lo = l;
  *hi = l + 1 < n - 1 ? l + 1 : n - 1;
  *w = v - (double)l;
}

// the value between the order statistics a (rank lo) and b (rank hi): numpy's _lerp
RETRIEVAL_HD double interpolate(double a, double b, double w) {
  RETRIEVAL_EXACT
  const double d = b - a;
  if (w >= 0.5) {
    const double u = 1.0 - w;
    const double p = d * u;
    return b - p;
  }
  const double p = d * w;
  return a + p;
}

}  // namespace quant
}  // namespace bartrt
