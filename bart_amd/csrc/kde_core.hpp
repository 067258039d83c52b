// A Gaussian kernel density estimate of the columns of a matrix on a grid, and the credible region of a density on a
// grid, stated once for host and device (kde.hip: kde_leaf, kde_merge, kde_fold, kde_stat, kde_sum, kde_add, kde_finish;
// bartrt_kde, bartrt_hpd_pdf).  Plain inline functions on plain pointers, no HIP call, in the idiom of hist_core.hpp,
// gr_core.hpp and ess_core.hpp: the kernels run them, and a host compiler alone builds them for the CPU tests
// (tests/kde_core_host.cpp).  The functions that take an exponential are templates on it: the device passes the RT
// kernels' exp_rt (kernels.hpp), the host program std::exp.
//
// ROWS.  A row counts for a column iff the mask is absent or non-zero there AND the column's value in it is finite.  A
// row the mask lets through whose value is an infinity or a NaN is counted in the column's `nonfinite` and otherwise
// does not exist (bartrt_marginals_range's behaviour; scipy.stats.gaussian_kde would return NaN everywhere).
//
// MOMENTS.  n, mean and M2 = sum (x - mean)^2 over the rows that count, with no sum of squares of the values anywhere
// (gr_core.hpp says why).  The order is fixed here and depends on no launch shape, chunk or round:
//   - the column's REFERENCE is the value in row 0 of the matrix if that is finite (whatever the mask says), else 0.0;
//     every value enters as y = x - ref.  For a column like a radius of 97 000 km that varies by a few km the y are
//     exact and small, and the means below are held to the variation's size, not the radius'.  The reference costs no
//     pass over the matrix; its price is that the moments are as accurate as max |x - ref| / std allows, so a first
//     row that holds a wild value (a sentinel like 1e300, even under a mask that removes it) takes digits from the
//     std of an otherwise good column -- never more than a reference of 0.0 would for values of that size;
//   - a LEAF is kMomentRows consecutive rows of the matrix (the last: up to the end).  Its mean is the sum of its y in
//     row order divided by their number, its M2 the sum in row order of (y - mean)^2: two passes (gr::leaf's);
//   - the kLeavesPerTile leaves of a TILE (kKdeTileRows consecutive rows) are merged in ascending order into the
//     first, and the tiles' triples in ascending order into one, by gr::merge unchanged; a triple with n = 0 is
//     skipped and one merged into n = 0 is copied;
//   - mean = ref + mean_y; std = sqrt(M2 / (n - 1)).
//
// BANDWIDTH.  h = factor std; the factor is Scott's n^(-1/5) (kScott), Silverman's (3 n / 4)^(-1/5) (kSilverman) --
// scipy.stats.gaussian_kde's bw_method for one dimension, here by inv_fifth_root below -- or the caller's positive
// scalar (kFactor).
//
// DENSITY at a grid point g:  pdf(g) = S / ((n h) sqrt(2 pi)),  S = sum_i E(-0.5 (u_i u_i)),  u_i = (g - x_i) rh,
// rh = 1 / h, with the products as written and nothing contracted; a term whose argument is below kArgMin (the RT
// kernels' kExpMin) is zero.  With E = exp_rt the density is that of exp_rt's FORMULA, which is not exp: its degree-9
// interpolant is within 7e-14 relative of exp and its one-step reduction by a rounded ln2 adds 2.3e-17 per unit of
// |a| / ln2, 2e-14 at 700 (kernels.hpp); the fp64 evaluation lies within 4e-16 of the formula (tests/
// test_gpu_rt_math.py).  So a device density is within about 1e-13 relative of the one with exp, not within 4e-16.  ORDER OF THE SUM: rows are cut into tiles of kKdeTileRows consecutive rows of the matrix;
// a tile's sum starts at 0.0 and takes its rows in ascending order, ONE accumulator per grid point; S starts at 0.0 and
// takes the tile sums in ascending order.  A row that does not count adds nothing -- or +0.0, which is the same bits in
// a sum that is never negative (tile_sum is handed a NaN for such a row).  No atomics: nothing depends on a schedule.
//
// DEGENERATE.  A column with n < 2, or whose std or h is zero or not finite (or 1 / h not finite), has h = NaN and a
// pdf row of NaN; its n, mean and std are reported as they are (mean NaN for n = 0, std NaN for n < 2).
//
// REGION (host only).  The credible region of pdf[n] at a fraction 0 < p <= 1: the grid points in descending order of
// pdf, ties by ascending index; cumulative sums in that order by plain additions; the total is the last of them; the
// region is the shortest prefix whose sum c has c >= p total.  -> mask, the threshold (smallest pdf included), the
// included sum and the number of maximal runs.  A NaN or a negative value anywhere, or total == 0: an empty mask and
// zeros.  It is hist::hpd_of, the code of the histogram's region.  The rule is ours: MC3's credregion could not be
// read (the reference checkout's modules/MCcubed is empty), so this is stated against SciPy's density and is not
// checked against MC3's source.
#pragma once
#include "gr_core.hpp"
#include "hist_core.hpp"

// (the exponentials of neighbouring rows are independent; only the additions are a chain)
#if defined(__clang__)
#define KDE_UNROLL _Pragma("unroll 4")
#else
#define KDE_UNROLL
#endif

namespace bartrt {
namespace kde {

constexpr long kMomentRows = 256;                 // rows of a leaf of the moments
constexpr long kLeavesPerTile = 8;
constexpr long kKdeTileRows = kMomentRows * kLeavesPerTile;   // rows of a tile: part of the rule, not a tunable
constexpr int kMaxGrid = 1024;
constexpr int kScott = 0, kSilverman = 1, kFactor = 2;
constexpr double kArgMin = -708.0;                // (kernels.hpp's kExpMin; kde.hip asserts it)
constexpr double kSqrt2Pi = 2.50662827463100050242;
constexpr int kQuad = 4;                          // a column's running moments: n, mean of y, M2, nonfinite

RETRIEVAL_HD double nan_value() { return quant::double_of(quant::kExp | (quant::kExp >> 1)); }
RETRIEVAL_HD long tiles(long nrows) { return (nrows + kKdeTileRows - 1) / kKdeTileRows; }
RETRIEVAL_HD long leaves(long nrows) { return (nrows + kMomentRows - 1) / kMomentRows; }

RETRIEVAL_HD double reference(const double *x, long col) { return hist::is_finite(x[col]) ? x[col] : 0.0; }

// the value of (row, col) for tile_sum: NaN for a row that does not count
RETRIEVAL_HD double staged(const double *x, long ld, const unsigned char *ok, long row, long col) {
  if (ok && !ok[row]) return nan_value();
  const double v = x[(size_t)row * ld + col];
  return hist::is_finite(v) ? v : nan_value();
}

// the quad of rows [r0, r1) of one column
RETRIEVAL_HD void leaf(const double *x, long ld, const unsigned char *ok, long r0, long r1, long col, double ref, double *q) {
  RETRIEVAL_EXACT
  double n = 0.0, bad = 0.0, sum = 0.0;
  for (long r = r0; r < r1; r++) {
    if (ok && !ok[r]) continue;
    const double v = x[(size_t)r * ld + col];
    if (!hist::is_finite(v)) {
      bad += 1.0;
      continue;
    }
    n += 1.0;
    sum += v - ref;
  }
  const double mean = n > 0.0 ? sum / n : 0.0;
  double m2 = 0.0;
  for (long r = r0; r < r1; r++) {
    if (ok && !ok[r]) continue;
    const double v = x[(size_t)r * ld + col];
    if (!hist::is_finite(v)) continue;
    const double d = (v - ref) - mean;
    m2 += d * d;
  }
  q[0] = n;
  q[1] = mean;
  q[2] = m2;
  q[3] = bad;
}

// quad b merged into quad a
RETRIEVAL_HD void merge_into(double *a, const double *b) {
  a[3] += b[3];
  if (b[0] == 0.0) return;
  if (a[0] == 0.0) {
    a[0] = b[0];
    a[1] = b[1];
    a[2] = b[2];
    return;
  }
  gr::merge(a, b);
}

RETRIEVAL_HD void clear_quad(double *q) { q[0] = q[1] = q[2] = q[3] = 0.0; }

// the leaves [l0, l1) of leaf[.][stride doubles apart] merged in ascending order into q (cleared here)
RETRIEVAL_HD void merge_leaves(const double *leaf, size_t stride, long l0, long l1, double *q) {
  clear_quad(q);
  for (long l = l0; l < l1; l++) merge_into(q, leaf + (size_t)l * stride);
}

// q^(-1/5): the library's pow as a seed, then one Newton step for y^-5 = q in correctly rounded operations alone,
// y (6 - q y^5) / 5 with the fifth power taken from the left.  A seed off by d relative leaves 3 d^2, so the result
// rests on no library's accuracy claim beyond a seed good to 1e-10; its roundings are counted in tests/kde_restate.py
RETRIEVAL_HD double inv_fifth_root(double q) {
  RETRIEVAL_EXACT
  const double y = pow(q, -0.2);
  const double y5 = (((y * y) * y) * y) * y;
  return (y * (6.0 - q * y5)) / 5.0;
}

RETRIEVAL_HD double factor_of(int rule, double factor, double n) {
  if (rule == kScott) return inv_fifth_root(n);
  if (rule == kSilverman) return inv_fifth_root(n * 0.75);
  return factor;
}

RETRIEVAL_HD bool usable(double h) { return h > 0.0 && hist::is_finite(h) && hist::is_finite(1.0 / h); }

// stat[4] = n, mean, std, h of a column from its merged quad
RETRIEVAL_HD void finish_moments(const double *q, double ref, int rule, double factor, double *stat) {
  RETRIEVAL_EXACT
  const double n = q[0];
  stat[0] = n;
  stat[1] = n >= 1.0 ? ref + q[1] : nan_value();
  const double sd = n >= 2.0 ? sqrt(q[2] / (n - 1.0)) : nan_value();
  stat[2] = sd;
  const double h = sd > 0.0 && hist::is_finite(sd) ? factor_of(rule, factor, n) * sd : nan_value();
  stat[3] = usable(h) ? h : nan_value();
}

// a tile's sum at g: v[n] the tile's values in row order (staged), rh = 1 / h
template <class Exp>
RETRIEVAL_HD double tile_sum(const double *v, long n, double g, double rh, Exp ex) {
  RETRIEVAL_EXACT
  double sum = 0.0;
  KDE_UNROLL
  for (long i = 0; i < n; i++) {
    const double u = (g - v[i]) * rh;
    const double a = -0.5 * (u * u);
    sum += a >= kArgMin ? ex(a) : 0.0;
  }
  return sum;
}

// the density from S and the column's stat (a degenerate column: NaN)
RETRIEVAL_HD double normalised(double sum, const double *stat) {
  RETRIEVAL_EXACT
  const double h = stat[3];
  if (!(h == h)) return nan_value();
  return sum / ((stat[0] * h) * kSqrt2Pi);
}

// The whole moments rule in one place, for host code: the merged quad of column col and its reference.
inline void moments(const double *x, long nrows, long ld, const unsigned char *ok, long col, double *q, double *ref) {
  *ref = reference(x, col);
  clear_quad(q);
  for (long k = 0; k < tiles(nrows); k++) {
    const long r0 = k * kKdeTileRows, r1 = std::min(nrows, r0 + kKdeTileRows);
    double t[kQuad], l[kQuad];
    clear_quad(t);
    for (long a = r0; a < r1; a += kMomentRows) {
      leaf(x, ld, ok, a, std::min(r1, a + kMomentRows), col, *ref, l);
      merge_into(t, l);
    }
    merge_into(q, t);
  }
}

// The whole estimate in one place, for host code: x[nrows][ld], ok[nrows] or null, cols[nsel], grid[nsel][ngrid] ->
// pdf[nsel][ngrid], stat[nsel][4], nonfinite[nsel]
template <class Exp>
inline void density(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols, int ngrid,
                    const double *grid, int rule, double factor, double *pdf, double *stat, uint64_t *nonfinite, Exp ex) {
  std::vector<double> v((size_t)kKdeTileRows), sum((size_t)ngrid);
  for (int s = 0; s < nsel; s++) {
    double q[kQuad], ref, *st = stat + (size_t)s * 4;
    moments(x, nrows, ld, ok, cols[s], q, &ref);
    finish_moments(q, ref, rule, factor, st);
    nonfinite[s] = (uint64_t)q[3];
    std::fill(sum.begin(), sum.end(), 0.0);
    const double rh = 1.0 / st[3];
    for (long k = 0; k < tiles(nrows) && st[3] == st[3]; k++) {
      const long r0 = k * kKdeTileRows, n = std::min(nrows - r0, kKdeTileRows);
      for (long i = 0; i < n; i++) v[i] = staged(x, ld, ok, r0 + i, cols[s]);
      for (int j = 0; j < ngrid; j++) sum[j] = sum[j] + tile_sum(v.data(), n, grid[(size_t)s * ngrid + j], rh, ex);
    }
    for (int j = 0; j < ngrid; j++) pdf[(size_t)s * ngrid + j] = normalised(sum[j], st);
  }
}

// REGION above.  n >= 1, 0 < p <= 1 are the caller's to check.
inline void hpd_pdf(const double *pdf, int n, double p, unsigned char *mask, double *threshold, double *included, int *nruns) {
  for (int i = 0; i < n; i++)
    if (!(pdf[i] >= 0.0)) {              // a NaN or a negative value
      std::fill(mask, mask + n, (unsigned char)0);
      *threshold = *included = 0.0;
      *nruns = 0;
      return;
    }
  hist::hpd_of(pdf, n, p, mask, threshold, included, nruns);
}

}  // namespace kde
}  // namespace bartrt
