// The optimiser's arithmetic, stated once for host and device: a batched multi-start Levenberg-Marquardt fit in a box
// (MC3's `leastsq`), the way mcmc_core.hpp states the sampler's.  Plain inline functions on plain pointers, no HIP
// call: the kernel (fit.hip: fit_advance) runs them one start per wave, and a host compiler alone builds them for the
// CPU tests (tests/fit_core_host.cpp).
//
// PARAMETERS.  Free, fixed and shared as retrieval.hpp reads `stepsize`; shared parameters are copied after every
// update and every perturbation.  The q-th free parameter is "column q"; nfree <= npars <= 64.
//
// RESIDUALS.  Row f < ndata is (band_f - data_f) / uncert_f.  With prior arrays, every parameter j with a non-zero
// priorlow[j] or priorup[j] adds the row (p_j - prior_j) / w, w = priorlow[j] below prior_j and priorup[j] above; a
// side whose width is zero does not constrain (the row is 0 there).  chisq is the sum of squares of all rows, data
// rows in filter order, then prior rows in parameter order, in one running sum.
//
// AN ITERATION is two model launches around two phases.
//   pick   (serial, a start's first lane) reads the K trial rows' band fluxes and statuses, takes the lowest chisq
//          among the valid rungs with status 0 (ties: the lowest rung); below the current chisq it is accepted and
//          lambda = max(lambda_k / 10, 1e-12), otherwise lambda *= 10^K and past 1e12 the start ends STALLED.  An
//          accepted step that lowers chisq by at most ftol * chisq, or moves every free parameter by at most
//          xtol * (|x_j| + stepsize_j), ends the start CONVERGED; so does a chisq of exactly zero, which no step can
//          lower.  Then it writes the nfree forward-difference rows:
//          x with x_j + h_j, h_j = fdstep * stepsize_j, the sign flipped where x_j + h_j leaves [pmin_j, pmax_j].
//          pick 0 takes the start's own model instead (rejected: NO_START).
//   solve  (the wave; lane q owns column q) streams the residual rows into A = J^T J and g = J^T r, row after row in
//          the order above, every lane summing its own column: no sum crosses lanes, so its order is the same
//          everywhere.  A column whose perturbed model is rejected (status 1 to 3, counted in nbad) is frozen for
//          this iteration; so is a parameter on a bound whose -g_j points outward.  D_j = max(D_j, A_jj) over the
//          fit.  For rung k, lambda_k = lambda 10^(k-1): (A + lambda_k diag D) delta = -g by Cholesky, left-looking,
//          column by column with the lanes on the rows; frozen columns are replaced by the identity with a zero
//          right-hand side (delta_j = 0 exactly).  A non-positive pivot or a non-finite delta makes the rung invalid:
//          its trial row is x itself and its bit in `valid` is clear.  Trial row k is clip(x + delta_k) to the box.
// A finished start keeps writing its final point into its rows, so every launch evaluates valid models.
//
// Each phase of solve is a loop over lanes (Exec::each): on the device the lanes are the wave's and each() ends in a
// barrier; on the host they run one after the other.  A phase reads what earlier phases wrote and writes only what
// its lane owns, so the two orders give the same numbers.
#pragma once
#include "mcmc_core.hpp"   // (not used here: programs that include this header alone find the sampler's names through it)
#include "retrieval.hpp"

#define FIT_HD RETRIEVAL_HD
#define FIT_EXACT RETRIEVAL_EXACT

namespace bartrt {
namespace fit {

using bartrt::kMaxPars;
constexpr int kMaxRungs = 8;
constexpr int kLanes = 64, kLdA = 64, kLdW = 65;   // W's rows are padded: it is read along rows and along columns
enum Status { kRunning = 0, kConverged = 1, kStalled = 2, kIterLimit = 3, kNoStart = 4 };
constexpr double kLambdaMin = 1e-12, kLambdaMax = 1e12;

// Every pointer is memory of the side that calls.
struct Problem : Objective {
  int nstarts, nrungs;
  long maxiter;
  double fdstep, ftol, xtol, lambda0;
  // the starts' state
  double *x;        // [S][npars]
  double *chisq;    // [S]
  double *lambda;   // [S]
  double *D;        // [S][npars] Marquardt's scaling (free parameters' slots)
  double *cur;      // [S][ndata] band fluxes at x
  int *status;      // [S]
  int *valid;       // [S] bit k: rung k of the last solve is valid
  long *niter;      // [S] iterations made
  long *nbad;       // [S][4] models rejected with status 1, 2, 3
  // the exchange with the model: the rows it is evaluated on (x itself for the starts' own models, then the
  // S * nfree Jacobian rows and the S * nrungs trial rows in turn, a start's rows together), and the band fluxes and
  // statuses of the launch that ran last
  double *jrows, *trows;
  const double *band;
  const int *mstatus;
  double *trace;    // [S][maxiter + 1][npars + 4]: x, chisq, lambda, chosen rung (-1: none), status; or null
};

FIT_HD size_t max_rows(int nstarts, int nfree, int nrungs) {
  return (size_t)nstarts * (size_t)(nfree > nrungs ? nfree : nrungs);
}

// scratch of one start's solve: LDS on the device
struct Work {
  double *A;                          // [64][kLdA] A[i][q] at i * kLdA + q
  double *W;                          // [64][kLdW] column c of the factor (and of M before it) at c * kLdW + i
  double *g, *jrow, *h, *diag, *t, *y, *z, *dlt;   // [64]
  int *jidx, *rej, *frozen, *flag;    // [64]; flag[0]: this rung is invalid, flag[1]: the valid mask
};
constexpr size_t kWorkDoubles = (size_t)kLanes * kLdA + (size_t)kLanes * kLdW + 8 * kLanes;
constexpr size_t kWorkBytes = kWorkDoubles * sizeof(double) + 4 * kLanes * sizeof(int);

FIT_HD Work carve(void *mem) {
  Work w;
  double *d = static_cast<double *>(mem);
  w.A = d; d += (size_t)kLanes * kLdA;
  w.W = d; d += (size_t)kLanes * kLdW;
  w.g = d; w.jrow = d + kLanes; w.h = d + 2 * kLanes; w.diag = d + 3 * kLanes; w.t = d + 4 * kLanes;
  w.y = d + 5 * kLanes; w.z = d + 6 * kLanes; w.dlt = d + 7 * kLanes;
  int *i = reinterpret_cast<int *>(d + 8 * kLanes);
  w.jidx = i; w.rej = i + kLanes; w.frozen = i + 2 * kLanes; w.flag = i + 3 * kLanes;
  return w;
}

struct HostExec {
  template <class F>
  void each(F f) const {
    for (int q = 0; q < kLanes; q++) f(q);
  }
};

FIT_HD bool has_prior(const Problem &p, int j) {
  return p.prior && p.priorlow && p.priorup && (p.priorlow[j] != 0.0 || p.priorup[j] != 0.0);
}

FIT_HD double prior_res(const Problem &p, int j, double v) {
  FIT_EXACT
  const double d = v - p.prior[j], w = d < 0.0 ? p.priorlow[j] : p.priorup[j];
  return w != 0.0 ? d / w : 0.0;
}

FIT_HD double data_res(const Problem &p, const double *band, int f) {
  FIT_EXACT
  return (band[f] - p.data[f]) / p.uncert[f];
}

FIT_HD double chisq_of(const Problem &p, const double *band, const double *point) {
  FIT_EXACT
  double c = 0.0;
  for (int f = 0; f < p.ndata; f++) {
    const double r = data_res(p, band, f);
    c += r * r;
  }
  for (int j = 0; j < p.npars; j++)
    if (has_prior(p, j)) {
      const double r = prior_res(p, j, point[j]);
      c += r * r;
    }
  return c;
}

// the parameter of column q (-1: there is no such column)
FIT_HD int free_index(const Problem &p, int q) {
  for (int j = 0; j < p.npars; j++)
    if (p.stepsize[j] > 0 && q-- == 0) return j;
  return -1;
}

FIT_HD double step_h(const Problem &p, int j, double xj) {
  FIT_EXACT
  const double h = p.fdstep * p.stepsize[j];
  return (xj + h > p.pmax[j] || xj + h < p.pmin[j]) ? -h : h;
}

FIT_HD double pow10_rung(int k) {   // 10^(k - 1), 0 <= k <= kMaxRungs
  const double t[kMaxRungs + 1] = {0.1, 1.0, 10.0, 100.0, 1e3, 1e4, 1e5, 1e6, 1e7};
  return t[k];
}

// the forward-difference rows of start s (a finished start: its point, nfree times)
FIT_HD void write_jacobian_rows(const Problem &p, int s) {
  FIT_EXACT
  const int np = p.npars;
  const double *x = p.x + (size_t)s * np;
  int q = 0;
  for (int j = 0; j < np; j++) {
    if (!(p.stepsize[j] > 0)) continue;
    double *row = p.jrows + ((size_t)s * p.nfree + q++) * np;
    for (int m = 0; m < np; m++) row[m] = x[m];
    if (p.status[s] != kRunning) continue;
    row[j] = x[j] + step_h(p, j, x[j]);
    copy_shared(np, p.stepsize, row);
  }
}

// pick number `it` of start s (it = 0: the start's own model).  Serial.
FIT_HD void pick_start(const Problem &p, int s, long it) {
  FIT_EXACT
  const int np = p.npars, nd = p.ndata, K = p.nrungs;
  double *x = p.x + (size_t)s * np, *cur = p.cur + (size_t)s * nd;
  long *nbad = p.nbad + (size_t)s * 4;
  int rung = -1;
  if (it == 0) {
    const int st = p.mstatus[s];
    for (int k = 0; k < 4; k++) nbad[k] = 0;
    for (int j = 0; j < np; j++) p.D[(size_t)s * np + j] = 0.0;
    p.niter[s] = 0;
    p.valid[s] = 0;
    p.lambda[s] = p.lambda0;
    copy_shared(np, p.stepsize, x);
    if (st != 0) {
      if (st >= 1 && st <= 3) nbad[st]++;
      p.status[s] = kNoStart;
      p.chisq[s] = INFINITY;
    } else {
      const double *b = p.band + (size_t)s * nd;
      for (int f = 0; f < nd; f++) cur[f] = b[f];
      p.chisq[s] = chisq_of(p, cur, x);
      p.status[s] = !std::isfinite(p.chisq[s]) ? kNoStart : p.chisq[s] == 0.0 ? kConverged : kRunning;
    }
  } else if (p.status[s] == kRunning) {
    p.niter[s]++;
    int best = -1;
    double cbest = INFINITY;
    for (int k = 0; k < K; k++) {
      if (!(p.valid[s] >> k & 1)) continue;
      const size_t r = (size_t)s * K + k;
      const int st = p.mstatus[r];
      if (st >= 1 && st <= 3) nbad[st]++;
      if (st != 0) continue;
      const double c = chisq_of(p, p.band + r * nd, p.trows + r * np);
      if (c < cbest) {
        cbest = c;
        best = k;
      }
    }
    if (best >= 0 && cbest < p.chisq[s]) {
      const size_t r = (size_t)s * K + best;
      const double *xn = p.trows + r * np, *b = p.band + r * nd;
      bool conv = p.chisq[s] - cbest <= p.ftol * p.chisq[s], moved = false;
      for (int j = 0; j < np; j++)
        if (p.stepsize[j] > 0 && fabs(xn[j] - x[j]) > p.xtol * (fabs(x[j]) + p.stepsize[j])) moved = true;
      if (!moved) conv = true;
      for (int j = 0; j < np; j++) x[j] = xn[j];
      for (int f = 0; f < nd; f++) cur[f] = b[f];
      p.chisq[s] = cbest;
      p.lambda[s] = fmax(p.lambda[s] * pow10_rung(best) / 10.0, kLambdaMin);
      rung = best;
      if (conv || cbest == 0.0) p.status[s] = kConverged;
    } else {
      for (int k = 0; k < K; k++) p.lambda[s] *= 10.0;
      if (p.lambda[s] > kLambdaMax) p.status[s] = kStalled;
    }
  }
  if (p.status[s] == kRunning && it >= p.maxiter) p.status[s] = kIterLimit;
  if (p.trace) {
    double *rec = p.trace + ((size_t)s * (p.maxiter + 1) + it) * (np + 4);
    for (int j = 0; j < np; j++) rec[j] = x[j];
    rec[np] = p.chisq[s];
    rec[np + 1] = p.lambda[s];
    rec[np + 2] = rung;
    rec[np + 3] = p.status[s];
  }
  write_jacobian_rows(p, s);
}

// one residual row into A and g: r0 the row at x, rq(q) the row at column q's perturbed point
template <class Exec, class Rq>
FIT_HD void accumulate_row(const Work &w, int n, double r0, Rq rq, Exec ex) {
  ex.each([&](int q) {
    FIT_EXACT
    if (q < n) w.jrow[q] = w.rej[q] ? 0.0 : (rq(q) - r0) / w.h[q];
  });
  ex.each([&](int q) {
    FIT_EXACT
    if (q >= n) return;
    const double jq = w.jrow[q];
    for (int i = 0; i < n; i++) w.A[i * kLdA + q] += w.jrow[i] * jq;
    w.g[q] += jq * r0;
  });
}

// the solve phase of start s: its K trial rows into p.trows, the valid mask into p.valid[s]
template <class Exec>
FIT_HD void solve_start(const Problem &p, const Work &w, int s, Exec ex) {
  const int np = p.npars, nd = p.ndata, n = p.nfree, K = p.nrungs;
  const double *x = p.x + (size_t)s * np, *cur = p.cur + (size_t)s * nd;
  double *trial = p.trows + (size_t)s * K * np;
  if (p.status[s] != kRunning) {
    ex.each([&](int k) {
      if (k < K)
        for (int m = 0; m < np; m++) trial[(size_t)k * np + m] = x[m];
    });
    return;
  }
  const double *pband = p.band + (size_t)s * n * nd;
  const int *pstat = p.mstatus + (size_t)s * n;
  ex.each([&](int q) {
    FIT_EXACT
    if (q >= n) return;
    const int j = free_index(p, q);
    w.jidx[q] = j;
    w.h[q] = step_h(p, j, x[j]);
    w.rej[q] = pstat[q];
    w.g[q] = 0.0;
    for (int i = 0; i < n; i++) w.A[i * kLdA + q] = 0.0;
  });
  for (int f = 0; f < nd; f++) {
    const double r0 = data_res(p, cur, f);
    accumulate_row(w, n, r0, [&](int q) { return data_res(p, pband + (size_t)q * nd, f); }, ex);
  }
  for (int m = 0; m < np; m++) {
    if (!has_prior(p, m)) continue;
    const double r0 = prior_res(p, m, x[m]);
    // parameter m at column q's perturbed point: moved when it is the column's parameter or a copy of it
    accumulate_row(w, n, r0, [&](int q) {
      FIT_EXACT
      const int j = w.jidx[q];
      const bool moves = m == j || (p.stepsize[m] < 0 && (int)(-p.stepsize[m]) - 1 == j);
      return prior_res(p, m, moves ? x[j] + w.h[q] : x[m]);
    }, ex);
  }
  ex.each([&](int q) {
    FIT_EXACT
    if (q == 0) {
      for (int i = 0; i < n; i++)
        if (w.rej[i] >= 1 && w.rej[i] <= 3) p.nbad[(size_t)s * 4 + w.rej[i]]++;
      w.flag[1] = 0;
    }
    if (q >= n) return;
    const int j = w.jidx[q];
    double &D = p.D[(size_t)s * np + j];
    if (!w.rej[q]) D = fmax(D, w.A[q * kLdA + q]);
    w.diag[q] = D;
    const bool outward = (x[j] <= p.pmin[j] && w.g[q] > 0.0) || (x[j] >= p.pmax[j] && w.g[q] < 0.0);
    w.frozen[q] = w.rej[q] != 0 || outward;
  });
  for (int k = 0; k < K; k++) {
    const double lam = p.lambda[s] * pow10_rung(k);
    ex.each([&](int q) {
      FIT_EXACT
      if (q == 0) w.flag[0] = 0;
      if (q >= n) return;
      for (int i = 0; i < n; i++) {
        double v = i == q ? 1.0 : 0.0;
        if (!w.frozen[i] && !w.frozen[q]) v = w.A[i * kLdA + q] + (i == q ? lam * w.diag[q] : 0.0);
        w.W[q * kLdW + i] = v;
      }
      w.y[q] = w.frozen[q] ? 0.0 : -w.g[q];
    });
    // left-looking Cholesky, column c: lane i forms row i's entry, the pivot is read by all
    for (int c = 0; c < n; c++) {
      ex.each([&](int i) {
        FIT_EXACT
        if (i < c || i >= n) return;
        double v = w.W[c * kLdW + i];
        for (int m = 0; m < c; m++) v -= w.W[m * kLdW + i] * w.W[m * kLdW + c];
        w.t[i] = v;
      });
      ex.each([&](int i) {
        FIT_EXACT
        if (i < c || i >= n) return;
        const double piv = w.t[c];
        const bool ok = piv > 0.0 && piv < INFINITY;
        const double root = sqrt(ok ? piv : 1.0);
        if (i == c) {
          if (!ok) w.flag[0] = 1;
          w.W[c * kLdW + c] = root;
        } else {
          w.W[c * kLdW + i] = w.t[i] / root;
        }
      });
    }
    for (int c = 0; c < n; c++)          // L z = y
      ex.each([&](int i) {
        FIT_EXACT
        if (i < c || i >= n) return;
        const double zc = w.y[c] / w.W[c * kLdW + c];
        if (i == c) w.z[c] = zc;
        else w.y[i] -= w.W[c * kLdW + i] * zc;
      });
    for (int c = n - 1; c >= 0; c--)     // L^T delta = z
      ex.each([&](int i) {
        FIT_EXACT
        if (i > c) return;
        const double dc = w.z[c] / w.W[c * kLdW + c];
        if (i == c) w.dlt[c] = dc;
        else w.z[i] -= w.W[i * kLdW + c] * dc;
      });
    ex.each([&](int q) {
      if (q < n && !std::isfinite(w.dlt[q])) w.flag[0] = 1;
    });
    ex.each([&](int q) {
      FIT_EXACT
      if (q != 0) return;
      double *row = trial + (size_t)k * np;
      for (int m = 0; m < np; m++) row[m] = x[m];
      if (w.flag[0]) return;
      w.flag[1] |= 1 << k;
      for (int i = 0; i < n; i++) {
        const int j = w.jidx[i];
        if (!w.frozen[i]) row[j] = fmin(fmax(x[j] + w.dlt[i], p.pmin[j]), p.pmax[j]);
      }
      copy_shared(np, p.stepsize, row);
    });
  }
  ex.each([&](int q) {
    if (q == 0) p.valid[s] = w.flag[1];
  });
}

}  // namespace fit
}  // namespace bartrt
