// The display rule of a model spectrum, stated once for host and device (specenv.hip: spec_display;
// bartrt_spectrum_display_dev, bartrt_posterior_spectrum).  What the reference's best-fit spectrum figure plots is not
// the spectrum itself (reference code/bestFit.py:645-648, :655, :662): an eclipse spectrum is divided by the stellar
// flux and scaled by (Rp/Rs)^2, and every geometry's curve goes through scipy.ndimage.gaussian_filter1d with sigma 2.
// Plain inline functions on plain pointers, no HIP call, in the idiom of quant_core.hpp: the kernel runs them, and a
// host compiler alone builds them for the CPU tests (tests/specenv_core_host.cpp).
//
// VALUE.  With a stellar flux y[i] = x[i] / sflux[i] * rprs * rprs, evaluated left to right: one division and two
// multiplications, each correctly rounded, which is what numpy computes for `spectrum / sflux * rprs * rprs`, bit for
// bit.  Without one (transit, direct) y[i] = x[i].
//
// SMOOTHING.  scipy.ndimage.correlate1d with a symmetric kernel of radius r, given as its half half[0..r] (half[0] the
// centre), in mode `reflect`: the half-sample-symmetric extension  d c b a | a b c d | d c b a,  repeated as often as
// needed, so a row shorter than the radius (W = 1 included) is defined.  reflect_index(i, W) is that extension's index
// map for any integer i.  The weights are the caller's (bart_amd.posterior.gauss_half makes SciPy's).
//
// ORDER.  One summation order: the centre term y[l] half[0] first, then the pairs (y[l-j] + y[l+j]) half[j] from the
// OUTERMOST pair j = r inwards to j = 1, each pair's sum, its product and the addition to the running sum rounded on
// its own (no contraction: RETRIEVAL_EXACT below, and -ffp-contract=off where a host compiler contracts by default).
// It is the order of SciPy's own loop for symmetric kernels (scipy/ndimage/src/ni_filters.c, NI_Correlate1D).  With
// r = 0 the smoothing is the identity: y[l] itself, half is not read.
//
// DECIMATION.  stride >= 1 keeps output column c from grid sample c * stride: Wk = ceil(W / stride) columns.  The
// smoothing always runs on the full grid; only the kept samples are evaluated.
#pragma once
#include "retrieval.hpp"

namespace bartrt {
namespace specenv {

constexpr int kMaxRadius = 64;   // the ABI's limit on r

// the weights as a kernel argument
struct HalfKernel {
  double w[kMaxRadius + 1];
};

// the kept columns of a W-sample grid
RETRIEVAL_HD long kept_columns(long W, long stride) { return (W + stride - 1) / stride; }

// the index in [0, W) that the half-sample-symmetric extension of a W-sample row has at any integer i
RETRIEVAL_HD long reflect_index(long i, long W) {
  const long period = 2 * W;
  long m = i % period;
  if (m < 0) m += period;
  return m < W ? m : period - 1 - m;
}

// the value before smoothing (VALUE above)
RETRIEVAL_HD double display_value(double x, bool has_sflux, double sflux, double rprs) {
  RETRIEVAL_EXACT
  if (!has_sflux) return x;
  const double a = x / sflux;
  const double b = a * rprs;
  return b * rprs;
}

// the smoothed value at l of the sequence y(i) (any callable; the caller maps i into its storage) in the order above
template <class At>
RETRIEVAL_HD double smooth_at(At &&y, long l, int r, const double *half) {
  RETRIEVAL_EXACT
  if (r == 0) return y(l);
  double acc = y(l) * half[0];
  for (int j = r; j >= 1; j--) {
    const double s = y(l - j) + y(l + j);
    const double p = s * half[j];
    acc = acc + p;
  }
  return acc;
}

// One row on the host: x[W] (and sflux[W] or null) -> out[kept_columns(W, stride)].  The kernel's restatement for
// tests: the same three functions on the row as it lies, no staging.
inline void display_row(const double *x, long W, const double *sflux, double rprs, int r, const double *half,
                        long stride, double *out) {
  const auto y = [&](long i) {
    const long g = reflect_index(i, W);
    return display_value(x[g], sflux != nullptr, sflux ? sflux[g] : 1.0, rprs);
  };
  const long Wk = kept_columns(W, stride);
  for (long c = 0; c < Wk; c++) out[c] = smooth_at(y, c * stride, r, half);
}

}  // namespace specenv
}  // namespace bartrt
