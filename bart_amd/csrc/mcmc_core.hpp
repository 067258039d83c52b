// The sampler's arithmetic, stated once for host and device: the counter-based random draws, the DEMC, snooker and
// Metropolis random-walk moves, shared parameters, Gaussian priors and the acceptance rule of the resident loop
// (mcmc.hip: mcmc_advance, mcmc_advance_groups).  Plain inline functions on plain pointers, no HIP call: the kernel runs them one chain per
// lane, the host runs them for the start of a run, and a host compiler alone builds them for the CPU tests
// (tests/mcmc_core_host.cpp).
//
// GENERATOR.  Philox4x32-10 (Salmon et al. 2011).  key = (seed low word, seed high word); counter = (t low word,
// t high word, chain, slot).  t is the iteration, 0 <= t < 2^63; the start of a run draws at t = kStartT + round
// (round 0: the jittered start, rounds 1..20: the re-draws of chains that start on a rejected model).  No draw
// depends on how many other draws were made, and the generator has no state anywhere: a run resumed at iteration t0
// (State::first) makes the draws of the global iterations t0, t0 + 1, ... and none at kStartT.
//
// Each block of four words gives two uniforms, u0 from words (0, 1) and u1 from words (2, 3): the top 53 bits h of
// the 64-bit number (word 0 high), u = (h + 0.5) 2^-53 in double arithmetic, and 1 - 2^-53 where that sum rounds to 1
// (h + 0.5 is not a double above 2^52), so 0 < u < 1 always.  A pair of normals comes from Box-Muller on (u0, u1):
// n0 = r cos(2 pi u1), n1 = r sin(2 pi u1), r = sqrt(-2 log u0).
//
//   slot        u0 / n0                          u1 / n1
//   0           partner r1                       partner r2
//   1           snooker's third chain z          snooker's gamma = 1.2 + u1
//   2           acceptance uniform               (unused)
//   3 + j / 2   jitter normal of parameter j     jitter normal of parameter j + 1       (j even; DEMC and mrw moves and
//                                                                                        the start, free parameters only)
//
// The model grids of `walk = unif` (grid_core.hpp) read the same jitter slots as UNIFORMS: u0 for parameter j, u1 for
// parameter j + 1, no Box-Muller.
//
// WALKS.  State::walk = 0: DEMC or, with State::snooker and more than three chains, snooker (every tenth iteration a
// DEMC move with gamma = 1).  walk = kWalkMrw: Metropolis random walk, prop_j = x_j + stepsize_j n_j for every free
// parameter j with the jitter normal n_j of the table, logjac = 0; no partner is drawn (slots 0 and 1 go unread), no
// rule of the move reads t, and any number of chains >= 1 will do: the chains do not see one another.  kWalkUnif is
// not a walk of this loop (no data, no acceptance): grid_core.hpp and grid.hip serve it.  Whatever the walk, the box
// test, shared parameters, the acceptance rule, priors, thinning and the output rows are the one common path below.
//
// PARAMETERS.  Free, fixed and shared as retrieval.hpp reads `stepsize`; DEMC moves, jitter and the box touch the free
// ones alone, and shared ones follow in every proposal and start point.
//
// CHI-SQUARE.  The data term is summed over the filters in index order.  With prior arrays and priorlow[j] != 0,
// parameter j adds ((p_j - prior_j) / sigma)^2, sigma = priorlow[j] below prior_j and priorup[j] above.  The chisq the
// loop keeps and writes out is the data term PLUS the prior terms.
#pragma once
#include "retrieval.hpp"

#define MCMC_HD RETRIEVAL_HD
#define MCMC_EXACT RETRIEVAL_EXACT

namespace bartrt {
namespace mcmc {

using bartrt::kMaxPars;         // (retrieval.hpp's, under the names this namespace has always given them)
using bartrt::check_stepsize;
using bartrt::copy_shared;
constexpr int kMaxChains = 1024;
constexpr unsigned kSlotPartners = 0, kSlotSnooker = 1, kSlotAccept = 2, kSlotJitter = 3;
constexpr unsigned long long kStartT = 0xFFFFFFFFFFFFFF00ull;
constexpr int kStartRounds = 20;
constexpr int kWalkMrw = 2, kWalkUnif = 3;   // State::walk (0: as State::snooker says); MC3's `walk` keys mrw and unif

struct Words {
  uint32_t w[4];
};

MCMC_HD Words philox4x32_10(Words c, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.w[0], p1 = (uint64_t)0xCD9E8D57u * c.w[2];
    const Words n = {{(uint32_t)(p1 >> 32) ^ c.w[1] ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w[3] ^ k1,
                      (uint32_t)p0}};
    c = n;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

MCMC_HD Words block(unsigned long long seed, unsigned long long t, int chain, unsigned slot) {
  const Words c = {{(uint32_t)t, (uint32_t)(t >> 32), (uint32_t)chain, slot}};
  return philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

MCMC_HD double uniform53(uint32_t hi, uint32_t lo) {
  MCMC_EXACT
  const uint64_t h = (((uint64_t)hi << 32) | lo) >> 11;
  const double u = ((double)h + 0.5) * 0x1p-53;
  return u < 1.0 ? u : 1.0 - 0x1p-53;
}

MCMC_HD void uniforms(unsigned long long seed, unsigned long long t, int chain, unsigned slot, double &u0,
                      double &u1) {
  const Words b = block(seed, t, chain, slot);
  u0 = uniform53(b.w[0], b.w[1]);
  u1 = uniform53(b.w[2], b.w[3]);
}

MCMC_HD void normals(unsigned long long seed, unsigned long long t, int chain, unsigned slot, double &n0,
                     double &n1) {
  MCMC_EXACT
  double u0, u1;
  uniforms(seed, t, chain, slot, u0, u1);
  const double r = sqrt(-2.0 * log(u0)), a = 6.283185307179586 * u1;
  n0 = r * cos(a);
  n1 = r * sin(a);
}

// uniform over the chains other than i, a, b (a, b < 0: unused), from the uniform u
MCMC_HD int other(double u, int nch, int i, int a, int b) {
  MCMC_EXACT
  int ex[3] = {i, a, b};
  const int k = 1 + (a >= 0) + (b >= 0);
  // ascending; unused entries (-1) come first
  if (ex[0] > ex[1]) { const int s = ex[0]; ex[0] = ex[1]; ex[1] = s; }
  if (ex[1] > ex[2]) { const int s = ex[1]; ex[1] = ex[2]; ex[2] = s; }
  if (ex[0] > ex[1]) { const int s = ex[0]; ex[0] = ex[1]; ex[1] = s; }
  int draw = (int)(u * (nch - k));
  if (draw >= nch - k) draw = nch - k - 1;
  for (int q = 3 - k; q < 3; q++) draw += draw >= ex[q];
  return draw;
}

// The run as the two halves of an iteration see it.  Every pointer is memory of the side that calls (device memory
// in the kernel, host memory in host code).
struct State : Objective {
  int nch;
  int snooker;                               // the walk asked for; it applies with more than three chains
  unsigned long long seed;
  long nsteps, thin;                         // rows t = thin - 1, 2 thin - 1, ... and the last iteration are written
  long first;                                // this call makes the global iterations first <= t < first + nsteps (a
                                             // resumed run: first > 0, a multiple of thin); every rule reads the global t
  // the population, kept between the halves
  double *x;        // [nch][npars] current points
  double *c;        // [nch] their chisq (data + prior terms; inf: not on a physical model)
  double *cur;      // [nch][ndata] their band fluxes
  double *logjac;   // [nch] of the pending proposal
  int *inside;      // [nch] the pending proposal lies in the box (else the model was given the current point)
  long *counts;     // [nch][4] accepted proposals, models rejected with status 1, 2, 3
  // the exchange with the model
  double *prop;         // [nch][npars] rows the model is evaluated on
  const double *band;   // [nch][ndata] its band fluxes
  const int *status;    // [nch] its statuses
  // results
  double *chain, *chisq;  // [nch][nkept][npars], [nch][nkept]
  double *models;         // [nch][nkept][ndata] band fluxes of the chains' current states, or null
  int walk;               // 0: DEMC / snooker as `snooker` says; kWalkMrw: Metropolis random walk
};

MCMC_HD long kept_rows(long nsteps, long thin) { return (nsteps + thin - 1) / thin; }

MCMC_HD double prior_term(const State &s, const double *p) {
  MCMC_EXACT
  double c = 0.0;
  if (!s.prior || !s.priorlow || !s.priorup) return c;
  for (int j = 0; j < s.npars; j++) {
    if (s.priorlow[j] == 0.0) continue;
    const double d = p[j] - s.prior[j];
    const double r = d / (d < 0.0 ? s.priorlow[j] : s.priorup[j]);
    c += r * r;
  }
  return c;
}

// chisq of a model row at the point p: data term in filter order, then the prior terms
MCMC_HD double chisq_of(const State &s, const double *band, const double *p) {
  MCMC_EXACT
  double c = 0.0;
  for (int f = 0; f < s.ndata; f++) {
    const double r = (band[f] - s.data[f]) / s.uncert[f];
    c += r * r;
  }
  return c + prior_term(s, p);
}

MCMC_HD bool accepts(double u, double cp, double c, double logjac) {
  MCMC_EXACT
  return std::isfinite(cp) && log(u) < -0.5 * (cp - c) + logjac;
}

// Start point of chain i: round 0 is the configured point, jittered by the stepsizes for every chain but the first;
// a later round re-draws it a tenth as wide.  Free parameters are clipped to the box; shared ones follow.
MCMC_HD void start_point(const State &s, int round, int i, const double *params, double *xi) {
  MCMC_EXACT
  const double width = round == 0 ? (i > 0 ? 1.0 : 0.0) : 0.1;
  for (int j = 0; j < s.npars; j += 2) {
    const bool f0 = s.stepsize[j] > 0, f1 = j + 1 < s.npars && s.stepsize[j + 1] > 0;
    double n0 = 0.0, n1 = 0.0;
    if ((f0 || f1) && width != 0.0) normals(s.seed, kStartT + (unsigned)round, i, kSlotJitter + j / 2, n0, n1);
    xi[j] = params[j] + (f0 ? width * s.stepsize[j] * n0 : 0.0);
    if (f0) xi[j] = fmin(fmax(xi[j], s.pmin[j]), s.pmax[j]);
    if (j + 1 < s.npars) {
      xi[j + 1] = params[j + 1] + (f1 ? width * s.stepsize[j + 1] * n1 : 0.0);
      if (f1) xi[j + 1] = fmin(fmax(xi[j + 1], s.pmin[j + 1]), s.pmax[j + 1]);
    }
  }
  copy_shared(s.npars, s.stepsize, xi);
}

// The moves: from chain i's point xi into pi, which holds a copy of xi; free parameters only.  Returns logjac.
// Metropolis random walk: every free parameter moves by its own stepsize times its jitter normal.
MCMC_HD double move_mrw(const State &s, long t, int i, const double *xi, double *pi) {
  MCMC_EXACT
  for (int j = 0; j < s.npars; j += 2) {
    const bool f0 = s.stepsize[j] > 0, f1 = j + 1 < s.npars && s.stepsize[j + 1] > 0;
    if (!f0 && !f1) continue;
    double n0, n1;
    normals(s.seed, (unsigned long long)t, i, kSlotJitter + j / 2, n0, n1);
    if (f0) pi[j] = xi[j] + s.stepsize[j] * n0;
    if (f1) pi[j + 1] = xi[j + 1] + s.stepsize[j + 1] * n1;
  }
  return 0.0;
}

// DEMC and snooker: the moves that read the population
MCMC_HD double move_population(const State &s, long t, int i, const double *xi, double *pi) {
  MCMC_EXACT
  const int nch = s.nch, np = s.npars;
  double u0, u1;
  uniforms(s.seed, (unsigned long long)t, i, kSlotPartners, u0, u1);
  const int r1 = nch > 1 ? other(u0, nch, i, -1, -1) : i;
  const int r2 = nch > 2 ? other(u1, nch, i, r1, -1) : r1;
  const double *x1 = s.x + (size_t)r1 * np, *x2 = s.x + (size_t)r2 * np;
  double logjac = 0.0;
  if (s.snooker && nch > 3 && t % 10 != 0) {
    // snooker update: move along the line through a third chain
    uniforms(s.seed, (unsigned long long)t, i, kSlotSnooker, u0, u1);
    const double *xz = s.x + (size_t)other(u0, nch, i, r1, r2) * np;
    double nd = 0.0, proj = 0.0;
    for (int j = 0; j < np; j++)
      if (s.stepsize[j] > 0) nd += (xi[j] - xz[j]) * (xi[j] - xz[j]);
    nd = sqrt(nd);
    if (nd == 0.0) nd = 1.0;
    for (int j = 0; j < np; j++)
      if (s.stepsize[j] > 0) proj += (x1[j] - x2[j]) * (xi[j] - xz[j]) / nd;
    const double g = 1.2 + u1;
    double ndn = 0.0;
    for (int j = 0; j < np; j++)
      if (s.stepsize[j] > 0) {
        pi[j] = xi[j] + g * proj * (xi[j] - xz[j]) / nd;
        ndn += (pi[j] - xz[j]) * (pi[j] - xz[j]);
      }
    logjac = (s.nfree - 1) * (log(fmax(sqrt(ndn), 1e-300)) - log(nd));
  } else {
    const double gam = t % 10 == 0 ? 1.0 : 2.38 / sqrt(2.0 * (s.nfree > 1 ? s.nfree : 1));
    for (int j = 0; j < np; j += 2) {
      const bool f0 = s.stepsize[j] > 0, f1 = j + 1 < np && s.stepsize[j + 1] > 0;
      if (!f0 && !f1) continue;
      double n0, n1;
      normals(s.seed, (unsigned long long)t, i, kSlotJitter + j / 2, n0, n1);
      if (f0) pi[j] = xi[j] + gam * (x1[j] - x2[j]) + 1e-3 * s.stepsize[j] * n0;
      if (f1) pi[j + 1] = xi[j + 1] + gam * (x1[j + 1] - x2[j + 1]) + 1e-3 * s.stepsize[j + 1] * n1;
    }
  }
  return logjac;
}

// First half of iteration t for chain i: the proposal from the population x into row i of prop.  A proposal outside
// the box is not sent to the model: the row gets the chain's current point and inside[i] = 0.
MCMC_HD void propose(const State &s, long t, int i) {
  MCMC_EXACT
  const int np = s.npars;
  const double *xi = s.x + (size_t)i * np;
  double *pi = s.prop + (size_t)i * np;
  for (int j = 0; j < np; j++) pi[j] = xi[j];
  // (one walk per run: the branch is the same for every chain)
  const double logjac = s.walk == kWalkMrw ? move_mrw(s, t, i, xi, pi) : move_population(s, t, i, xi, pi);
  int in = 1;
  for (int j = 0; j < np; j++)
    if (s.stepsize[j] > 0) in = in && pi[j] >= s.pmin[j] && pi[j] <= s.pmax[j];
  if (in) copy_shared(np, s.stepsize, pi);
  else
    for (int j = 0; j < np; j++) pi[j] = xi[j];
  s.inside[i] = in;
  s.logjac[i] = logjac;
}

// Second half of iteration t for chain i, once the model has run on prop: chisq, the decision, the chain's new
// state, its counters and (on a kept iteration) its output rows.  A proposal that fell outside the box is refused
// and its model row (the current point's) is not counted as a rejected model.
MCMC_HD void finish(const State &s, long t, int i) {
  const int np = s.npars, nd = s.ndata;
  double *xi = s.x + (size_t)i * np, *ci = s.cur + (size_t)i * nd;
  const double *pi = s.prop + (size_t)i * np, *bi = s.band + (size_t)i * nd;
  double cp = INFINITY;
  if (s.inside[i]) {
    const int st = s.status[i];
    if (st >= 1 && st <= 3) s.counts[(size_t)i * 4 + st]++;
    if (st == 0) cp = chisq_of(s, bi, pi);
  }
  double u, unused;
  uniforms(s.seed, (unsigned long long)t, i, kSlotAccept, u, unused);
  if (accepts(u, cp, s.c[i], s.logjac[i])) {
    for (int j = 0; j < np; j++) xi[j] = pi[j];
    for (int f = 0; f < nd; f++) ci[f] = bi[f];
    s.c[i] = cp;
    s.counts[(size_t)i * 4]++;
  }
  if ((t + 1) % s.thin != 0 && t != s.first + s.nsteps - 1) return;
  const size_t row = (size_t)i * kept_rows(s.nsteps, s.thin) + (size_t)((t - s.first) / s.thin);
  for (int j = 0; j < np; j++) s.chain[row * np + j] = xi[j];
  s.chisq[row] = s.c[i];
  if (s.models)
    for (int f = 0; f < nd; f++) s.models[row * nd + f] = ci[f];
}

// GROUPS.  Several independent retrievals of one shape (nch chains, npars parameters, ndata data each) advance in one
// loop over common arrays: x, prop, band, status, cur, c, logjac, inside and counts hold G nch rows, group g's from row
// g nch on; chain, chisq and models are [G][nch][nkept]...  `all` carries the call's common fields and the heads of those
// arrays; group g's State is its own problem and seed over its slices, and chain i of the group is row i of each: every
// rule above runs on it as on a run of its own (draws keyed by the group's seed and the LOCAL chain index, partners
// from the group alone).  A null array of `all` stays null.
MCMC_HD State group_state(const State &all, int g, const Objective &o, unsigned long long seed) {
  State s = all;
  static_cast<Objective &>(s) = o;
  s.seed = seed;
  const size_t r = (size_t)g * all.nch, k = r * (size_t)kept_rows(all.nsteps, all.thin), np = o.npars, nd = o.ndata;
#define MCMC_SLICE(field, n) if (s.field) s.field += (n)
  MCMC_SLICE(x, r * np); MCMC_SLICE(c, r); MCMC_SLICE(cur, r * nd); MCMC_SLICE(logjac, r); MCMC_SLICE(inside, r);
  MCMC_SLICE(counts, r * 4); MCMC_SLICE(prop, r * np); MCMC_SLICE(band, r * nd); MCMC_SLICE(status, r);
  MCMC_SLICE(chain, k * np); MCMC_SLICE(chisq, k); MCMC_SLICE(models, k * nd);
#undef MCMC_SLICE
  return s;
}

// what one loop takes: every group one workgroup of at most kMaxChains lanes, and no more than kMaxChains rows in all
MCMC_HD bool groups_fit(long ngroups, long nch) {
  return ngroups >= 1 && nch >= 1 && nch <= kMaxChains && ngroups * nch <= kMaxChains;
}

// Host code.  The start of a run: the configured point jittered by the stepsizes, chains that start on a rejected
// model re-drawn up to kStartRounds times, every round ONE model call on the chains of all groups.  gs [ngroups] are
// group_state's (slices of common arrays, gs[0] at their head), params[g] group g's configured point.
// model(rows [n][npars], n, band [n][ndata], status [n]) is the batched model; status [ngroups nch] is scratch.  A
// group whose chains all stand on a model is left alone in the later rounds (its rows are evaluated again with the
// rest and not read), so it gets the start of a run of its own.  Fills x, c and cur; counts the rejected models in
// nbad[g][1..3] (null: not counted).  ok[g] = 0: no chain of group g starts on a physical model.
template <class Model>
inline void start_groups(const State *gs, int ngroups, const double *const *params, Model &&model, int *status,
                         long *nbad, char *ok) {
  const int nch = gs[0].nch;
  char *active = ok;   // (during the rounds: the group still re-draws)
  auto evaluate = [&] {
    model(gs[0].x, ngroups * nch, gs[0].cur, status);
    for (int g = 0; g < ngroups; g++) {
      if (!active[g]) continue;
      const State &s = gs[g];
      const int *st = status + (size_t)g * nch;
      for (int i = 0; i < nch; i++) {
        if (nbad && st[i] >= 1 && st[i] <= 3) nbad[(size_t)g * 4 + st[i]]++;
        s.c[i] = st[i] == 0 ? chisq_of(s, s.cur + (size_t)i * s.ndata, s.x + (size_t)i * s.npars) : INFINITY;
      }
    }
  };
  for (int g = 0; g < ngroups; g++) {
    active[g] = 1;
    for (int i = 0; i < nch; i++) start_point(gs[g], 0, i, params[g], gs[g].x + (size_t)i * gs[g].npars);
  }
  evaluate();
  for (int round = 1; round <= kStartRounds; round++) {
    bool any_bad = false;
    for (int g = 0; g < ngroups; g++) {
      if (!active[g]) continue;
      const State &s = gs[g];
      bool bad = false;
      for (int i = 0; i < nch; i++)
        if (!std::isfinite(s.c[i])) {
          bad = true;
          start_point(s, round, i, params[g], s.x + (size_t)i * s.npars);
        }
      active[g] = bad;
      any_bad = any_bad || bad;
    }
    if (!any_bad) break;
    evaluate();
  }
  for (int g = 0; g < ngroups; g++) {
    ok[g] = 0;
    for (int i = 0; i < nch; i++)
      if (std::isfinite(gs[g].c[i])) ok[g] = 1;
  }
}

// one run: false where no chain starts on a physical model
template <class Model>
inline bool start_population(const State &s, const double *params, Model &&model, int *status, long *nbad) {
  char ok = 0;
  start_groups(&s, 1, &params, model, status, nbad, &ok);
  return ok != 0;
}

// Diagnostics (bartrt_mcmc_draws): every draw of chain i at iteration t among nch chains, as doubles:
// out[0..4] the uniforms of r1, r2, z, gamma and acceptance, out[5] log of the acceptance uniform, out[6..8] the
// partners r1, r2, z (z = -1 with fewer than four chains), out[9 + j] the jitter normal of parameter j.
constexpr int kDrawsHead = 9;
MCMC_HD void draws_row(unsigned long long seed, unsigned long long t, int nch, int i, int npars, double *out) {
  double unused;
  uniforms(seed, t, i, kSlotPartners, out[0], out[1]);
  uniforms(seed, t, i, kSlotSnooker, out[2], out[3]);
  uniforms(seed, t, i, kSlotAccept, out[4], unused);
  out[5] = log(out[4]);
  const int r1 = nch > 1 ? other(out[0], nch, i, -1, -1) : i;
  const int r2 = nch > 2 ? other(out[1], nch, i, r1, -1) : r1;
  out[6] = r1;
  out[7] = r2;
  out[8] = nch > 3 ? other(out[2], nch, i, r1, r2) : -1;
  for (int j = 0; j < npars; j += 2) {
    double n0, n1;
    normals(seed, t, i, kSlotJitter + j / 2, n0, n1);
    out[kDrawsHead + j] = n0;
    if (j + 1 < npars) out[kDrawsHead + j + 1] = n1;
  }
}

}  // namespace mcmc
}  // namespace bartrt
