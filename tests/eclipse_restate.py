"""The eclipse column (csrc/integ.hpp, rt_eclipse*.hpp) restated in mpmath at 50 digits -- TEST INFRASTRUCTURE ONLY.

Written from the definitions in the header comments of csrc/integ.hpp and csrc/rt_eclipse_s1s.hpp; it shares no code
with the kernels or with oracle/rt_oracle.c column_eclipse.  Inputs are doubles, each taken exactly: per layer (counted
FROM THE TOP, k = 0 the top layer) the extinction e_k (transit_restate.extinction: the records' weights times the
table values at the records' offsets, with its error term de_k), the path length dr_k = r_{k-1} - r_k (word 0 of the
layer record), the Planck exponent x_k = (c2 / T_k) nu (word 1 times nu); nu; toomuch; per ray 1 / mu_a, the weight
w_a and the threshold thr_a as the engine holds them (engine.ray_args); the deck layer kend.

    tau, rules 0 / 2   tau_k = sum_{j=1..k} (e_{j-1} + e_j) dr_j / 2
    tau, rule 1        even k: S_k = S_{k-2} + panel(dr_{k-1}, dr_k; e_{k-2}, e_{k-1}, e_k), tau_k = S_k;
                       odd k: tau_k = S_{k-1} + (e_{k-1} + e_k) dr_k / 2           (panels (0,1,2), (2,3,4), ...)
    panel(h0, h1; y0, y1, y2) = (h0 + h1) / 6 [(2 - h1/h0) y0 + (h0 + h1)^2 / (h0 h1) y1 + (2 - h0/h1) y2];
                       h0 = 0 or h1 = 0: the two trapezoids h0 (y0 + y1) / 2 + h1 (y1 + y2) / 2
    cut vertical       last = the first k in 1 .. kend with tau_k > toomuch, else kend; the same for every ray
    cut slant          last_a = the first k in 1 .. kend with tau_k > thr_a (<=> fl(tau_k / mu_a) > toomuch), else kend
    deck_a             a deck lies on kend, last_a = kend and tau_kend did not pass the cut
    B_k = 2 h c^2 nu^3 / (exp(x_k) - 1),  E_ak = exp(-tau_k / mu_a),  y_ak = B_k E_ak
    rule 0             I_a = sum_{k=1..last} (B_{k-1} + B_k) / 2 (E_{a,k-1} - E_ak)              [+ y_a,last on a deck]
    rule 2             I_a = (1 / mu_a) sum_{k=1..last} (y_{a,k-1} + y_ak) / 2 (tau_k - tau_{k-1})            [+ deck]
    rule 1             the points (tau_k, y_ak), k = 0 .. last, and -- when a layer exists below `last` and no deck was
                       reached -- the pad point (tau_last + p, 0), p = 1 (cut vertical) or mu_a (cut slant: one unit of
                       SLANT depth).  n points: n even starts with the trapezoid of the first interval, then panels;
                       n odd is all panels.  I_a = (1 / mu_a) sum                                             [+ deck]
    F = sum_a w_a I_a

RUNNING ERROR BOUNDS: what a correct fp64 evaluation in any of the kernels' (and the oracle's) orders of operations may
differ by; first order in u = 2^-53, every count rounded up, 1e-6 of slack.  DERIVED from the arithmetic, never fitted
to a device result.  The documented figures used: exp_rt within EXP_REL = 4e-16 of its interpolant and the interpolant
within 7.5e-14 + 2.4e-17 |n| of exp (csrc/kernels.hpp; tests/test_rt_math_cpu.py), |n| <= 1.4427 |x| + 1; the
reciprocals RCP = 2.3e-15 (rcp_n1, the wider of the two figures tests/test_gpu_rt_math.py asserts: the single-wave
forms take one Newton step for the panel reciprocals, the others rcp_core at 1.2e-16 -- the single-wave forms set
this count); the Planck term 4e-16 e^x / (e^x - 1) + 2.3e-15 of its own formula (the same file); the resampled CIA
planes 32 u (transit_restate.CIA_ALLOW, inside de_k).

  extinction.  de_k of transit_restate.extinction (T + 4 roundings on the magnitude sum, the CIA allowance).
  tau, rules 0 / 2.  A term rounds three times (sum, product, the running sum; the half is exact):
      dterm_k = (de_{k-1} + de_k) dr_k / 2 + 3 u |term_k|;   dtau_k = sum dterm + (k + 1) u sum |term|.
  tau, rule 1.  The radius weights use true divisions: hs, hs / 6, the quotient, 2 - q, hs^2, h0 h1, the products:
      at most 12 u on each |w_i e_i| (the oracle's order of the same panel included) and the cancellation of 2 - q:
      2 u (hs / 6) q |e|.   dpanel = sum |w_i| de_i + 12 u S + 2 u (hs / 6) (q0 |e_{k-2}| + q2 |e_k|), S = sum |w_i e_i|;
      dtau_k (even) = sum dpanel + (panels + 3) u sum S; odd: + dterm_k + u (|S_{k-1}| + |term_k|).
  tau differences.  The intensity rules of tau read h_k = tau_k - tau_{k-1}.  Its error is NOT dtau_k + dtau_{k-1}:
      the common part S cancels.  dh_k = the errors of the pieces that differ (odd k: term_k; even k: panel_k and
      term_{k-1}) + 4 u (|tau_k| + |tau_{k-1}|) (each depth's own roundings, the fused panel chain's partial sums, the
      slant forms' product tau / mu) + u |h_k|.  The pad interval p: 2 u (|tau_last| + p) + u p.
  Planck.  x_k = c nu rounds (the oracle: four roundings): 4 u x e^x / (e^x - 1); exp_rt's interpolant and rounding under
      the difference: (4e-16 + 7.5e-14 + 2.4e-17 (1.4427 x + 1)) e^x / (e^x - 1); rcp_n1 2.3e-15; the numerator
      2 h nu^3 c^2 and the product: 8 u.   dB_k = B_k relB_k.
  transmittance.  d(exp(-tau / mu)) = E dtau / mu; the product tau / mu (the oracle: a division) 3 u |x|; exp_rt as
      above with |n| <= 1.4427 x + 1.   relE_ak = 4e-16 + 7.5e-14 + 2.4e-17 (1.4427 x + 1) + 3 u x + dtau_k / mu_a.
      The SQ ray (the square-root ray order: slot A - 1 is the square of slot 0): twice the first ray's relative error,
      one more rounding, and the distance of 1 / mu_last from 2 / mu_first (up to 8.9e-16 relative: order_angles_for_
      square), tau |1 / mu_l - 2 / mu_f|; the larger of this and the direct evaluation is taken.
      The clamps as ABSOLUTE allowances: exp(kExpMin) = 3.4e-308, and beyond tau_cap = 708 / max_a (1 / mu_a) the floor
      exp(-tau_cap / mu_a).      dE = E relE + allowances;  dy = y (relB + relE + u) + B allowances.
  rule 0.  dterm = (dB_{k-1} + dB_k) / 2 |E_{k-1} - E_k| + (B_{k-1} + B_k) / 2 (dE_{k-1} + dE_k) + 4 u |term|;
      dI = sum dterm + (last + 1) u sum |term| + dy_last (deck) + u |I|.
  rule 2.  dterm = [(dy_{k-1} + dy_k) / 2 |h_k| + |y_{k-1} + y_k| / 2 dh_k] / mu + 5 u |term|; the sum as in rule 0.
  rule 1.  The panel weights over tau, w0 = h0 / 3 + h1 / 6 - h1^2 / (6 h0), w2 its mirror, w1 = hs^3 / (6 h0 h1):
      the PROPAGATION of dh is the conditioning term, dw ~ w dh / h, large exactly where panels are thin:
        dw0 = (1/3 + h1^2 / (6 h0^2)) dh0 + |1/6 - h1 / (3 h0)| dh1,   dw2 mirrored,
        dw1 = |w1| (|3 / hs - 1 / h0| dh0 + |3 / hs - 1 / h1| dh1),
      plus the weights' own roundings through the reciprocals: (2 RCP + 10 u) |w_i| and (RCP + 2 u) (hs / 6) q.
      dpanel = sum (dw_i |y_i| + |w_i| dy_i) + 4 u sum |w_i y_i|; a trapezoid: dh (|y| sum) / 2 + h (dy sum) / 2 + 4 u.
      A dead ray's pad panel rebuilt after the walk takes four fresh exponentials: the same dy.
      dI = [sum dpanel + (n + 1) u sum |terms|] / mu + 2 u |I| + dy_last (deck).
  flux.  Quadrature last (sum_a w_a I_a: A + 1 roundings) or first (w_a / mu_a rounded, the angle sum of A terms under
      every layer's weight, then the layer sum): the SUM of the two counts is taken, which covers the larger:
      dF = sum_a w_a dI_a + (2 A + 6) u sum_a w_a T_a,  T_a = the sum of |terms| of I_a.
"""
from __future__ import annotations

import mpmath
import numpy as np

from transit_restate import DPS, EXP_REL, EXP_RT_FIT, EXP_RT_LN2, SLACK, U, mp_array, to_float  # noqa: F401

RCP = 2.3e-15
EXP_MIN_ABS = 3.4e-308           # exp(kExpMin), kExpMin = -708 (csrc/kernels.hpp)
K_H, K_LS, K_KB = 6.6260755e-27, 2.99792458e10, 1.380658e-16      # csrc/kernels.hpp (and oracle/rt_oracle.h)
SQ_TOL = 8.9e-16                 # order_angles_for_square (csrc/rt_launch.hpp)
mpf = mpmath.mpf

MUTANTS = ("pad_vertical", "pad_on_bottom", "pad_with_deck", "parity", "cut_late", "cut_ge", "deck_dropped", "deck_above",
           "sq_unsquared", "trapezoids", "zero_width")


class Rays:
    """invmu, wgt, thr (doubles, the raygrid's order); first / last: the slots of the SQ pair or None."""

    def __init__(self, invmu, wgt, thr, sq_pair=None):
        self.invmu, self.wgt, self.thr = (np.asarray(x, float) for x in (invmu, wgt, thr))
        self.sq = sq_pair
        self.A = len(self.invmu)

    @classmethod
    def from_engine(cls, ra):
        """engine.ray_args() -> Rays."""
        pair = (int(ra["order"][0]), int(ra["order"][-1])) if ra["sq"] else None
        return cls(ra["invmu"], ra["wgt"], ra["thr"], pair)

    @classmethod
    def from_grid(cls, angles_deg, toomuch):
        """The host's arithmetic restated in numpy (no GPU): thr through bartrt_slant_thresholds, a host call."""
        from bart_amd import engine
        ang = np.asarray(angles_deg, float)
        A = len(ang)
        lo = np.array([0.0 if a == 0 else 0.5 * (ang[a - 1] + ang[a]) for a in range(A)])
        hi = np.array([90.0 if a == A - 1 else 0.5 * (ang[a] + ang[a + 1]) for a in range(A)])
        pi = 3.141592653589793
        wgt = pi * (np.sin(hi * pi / 180.0) ** 2 - np.sin(lo * pi / 180.0) ** 2)
        invmu = 1.0 / np.cos(ang * pi / 180.0)
        pair = None
        for i in range(A):
            for j in range(A):
                if pair is None and i != j and abs(invmu[j] - 2.0 * invmu[i]) <= SQ_TOL * invmu[j]:
                    pair = (i, j)
        return cls(invmu, wgt, engine.slant_thresholds(toomuch, invmu)[0], pair)


class Col:
    pass


def _panel_w(h0, h1):
    hs = h0 + h1
    return hs / 6 * (2 - h1 / h0), hs / 6 * (hs * hs / (h0 * h1)), hs / 6 * (2 - h0 / h1)


def taus(e, de, dr, kend, rule1):
    """One column: e[L] mpf, de[L] floats, dr[L] mpf -> (tau[kend + 1] mpf, dtau[kend + 1], dh[kend + 1]); dh[k]: the
    bound on tau_k - tau_{k-1}."""
    zero = mpf(0)
    tau, dtau, dh = [zero], [0.0], [0.0]
    ae = [abs(float(x)) for x in e]
    drf = [float(x) for x in dr]
    if not rule1:
        esum, asum = 0.0, 0.0
        for k in range(1, kend + 1):
            t = (e[k - 1] + e[k]) * dr[k] / 2
            dt = (de[k - 1] + de[k]) * drf[k] / 2 + 3 * U * abs(float(t))
            esum += dt; asum += abs(float(t))
            tau.append(tau[-1] + t)
            dtau.append((esum + (k + 1) * U * asum) * SLACK)
            dh.append((dt + 4 * U * (abs(float(tau[k])) + abs(float(tau[k - 1]))) + U * abs(float(t))) * SLACK)
        return tau, dtau, dh
    S, esum, asum, npan = zero, 0.0, 0.0, 0
    dtrap = [0.0] * (kend + 2)
    for k in range(1, kend + 1):
        if k & 1:
            t = (e[k - 1] + e[k]) * dr[k] / 2
            dtrap[k] = (de[k - 1] + de[k]) * drf[k] / 2 + 3 * U * abs(float(t))
            tau.append(S + t)
            dtau.append((esum + (npan + 3) * U * asum + dtrap[k] + U * (abs(float(S)) + abs(float(t)))) * SLACK)
            piece = dtrap[k]
        else:
            h0, h1 = dr[k - 1], dr[k]
            if h0 == 0 or h1 == 0:
                w = (h0 / 2, (h0 + h1) / 2, h1 / 2)
                canc = 0.0
            else:
                w = _panel_w(h0, h1)
                canc = 2 * U * float((h0 + h1) / 6) * (float(h1 / h0) * ae[k - 2] + float(h0 / h1) * ae[k])
            wf = [abs(float(x)) for x in w]
            Sp = wf[0] * ae[k - 2] + wf[1] * ae[k - 1] + wf[2] * ae[k]
            dp = wf[0] * de[k - 2] + wf[1] * de[k - 1] + wf[2] * de[k] + 12 * U * Sp + canc
            S = S + w[0] * e[k - 2] + w[1] * e[k - 1] + w[2] * e[k]
            esum += dp; asum += Sp; npan += 1
            tau.append(S)
            dtau.append((esum + (npan + 3) * U * asum) * SLACK)
            piece = dp + dtrap[k - 1]
        h = abs(float(tau[k] - tau[k - 1]))
        dh.append((piece + 4 * U * (abs(float(tau[k])) + abs(float(tau[k - 1]))) + U * h) * SLACK)
    return tau, dtau, dh


def planck(x, nu):
    """-> (B mpf, relB) of the exponent x (mpf) at the wavenumber nu (a double)."""
    n = mpf(nu)
    ex = mpmath.exp(x)
    B = 2 * mpf(K_H) * n * n * n * mpf(K_LS) * mpf(K_LS) / (ex - 1)
    xf = float(x)
    assert xf < 700.0, xf
    amp = float(ex / (ex - 1))
    rel = (4 * U * xf + EXP_REL + EXP_RT_FIT + EXP_RT_LN2 * (1.4427 * xf + 1.0)) * amp + RCP + 8 * U
    return B, rel * SLACK


def prepare(e, de, dr, xB, nu, rays: Rays, kend, deck_on, toomuch, L):
    """The parts of a set of columns that do not depend on the rule's intensity form or the cut: e[L, nc] mpf,
    de[L, nc], dr[L] doubles, xB[L, nc] mpf (Planck exponents), nu[nc] doubles."""
    c = Col()
    with mpmath.workdps(DPS):
        c.L, c.kend, c.deck_on, c.toomuch, c.rays, c.nc = int(L), int(kend), bool(deck_on), float(toomuch), rays, e.shape[1]
        drm = [mpf(float(x)) for x in dr]
        c.tau, c.dtau, c.dh, c.B, c.relB, c.E, c.relE, c.absE = {}, {}, {}, [], [], {}, {}, {}
        tcap = 708.0 / float(np.max(rays.invmu))
        for i in range(c.nc):
            Bs = [planck(xB[k, i], nu[i]) for k in range(kend + 1)]
            c.B.append([b for b, _ in Bs]); c.relB.append([r for _, r in Bs])
            for r1 in (False, True):
                t, dt, dh = taus(list(e[:, i]), list(de[:, i]), drm, kend, r1)
                c.tau[r1, i], c.dtau[r1, i], c.dh[r1, i] = t, dt, dh
                tf = [float(x) for x in t]
                rel = {}
                for a in range(rays.A):
                    im = mpf(float(rays.invmu[a]))
                    c.E[r1, i, a] = [mpmath.exp(-x * im) for x in t]
                    rel[a] = [EXP_REL + EXP_RT_FIT + EXP_RT_LN2 * (1.4427 * abs(v) * rays.invmu[a] + 1.0)
                              + 3 * U * abs(v) * rays.invmu[a] + d * rays.invmu[a] for v, d in zip(tf, dt)]
                    c.absE[r1, i, a] = [EXP_MIN_ABS + (float(mpmath.exp(-tcap * rays.invmu[a])) if v > tcap else 0.0) for v in tf]
                if rays.sq:
                    f, l = rays.sq
                    gap = abs(float(mpf(float(rays.invmu[l])) - 2 * mpf(float(rays.invmu[f]))))
                    rel[l] = [max(d, 2 * s + U + abs(v) * gap) for d, s, v in zip(rel[l], rel[f], tf)]
                for a in range(rays.A):
                    c.relE[r1, i, a] = [x * SLACK for x in rel[a]]
    return c


def cut_of(tau, thr, kend, ge=False):
    for k in range(1, kend + 1):
        if tau[k] > thr or (ge and tau[k] == thr):
            return k, True
    return kend, False


def solve(c: Col, i, rule, cut, mutant=None, ray=0, last_override=None):
    """Column i under (rule, cut 'vertical' | 'slant') -> dict(last[A], deck[A], I[A] mpf, dI[A], F mpf, dF, tau, dtau).
    mutant: one of MUTANTS (a deliberate mistake; `ray`: the ray it applies to where it names one).  last_override:
    {ray: last} -- the other outcome of an undecided cut (the ray then did not pass the cut on that layer unless the
    override is its own layer, where it did)."""
    with mpmath.workdps(DPS):
        r1 = rule == 1
        rays, kend, L = c.rays, c.kend, c.L
        tau, dtau, dh, B, relB = c.tau[r1, i], c.dtau[r1, i], c.dh[r1, i], c.B[i], c.relB[i]
        zero = mpf(0)
        out = {"last": [], "deck": [], "I": [], "dI": [], "T": [], "tau": tau, "dtau": dtau}
        for a in range(rays.A):
            thr = mpf(float(rays.thr[a])) if cut == "slant" else mpf(c.toomuch)
            last, passed = cut_of(tau, thr, kend, ge=mutant == "cut_ge")
            if last_override and a in last_override:
                last, passed = last_override[a]
            if mutant == "cut_late" and a == ray and passed and last + 1 <= kend:
                last, passed = last + 1, True
            deck = c.deck_on and last == kend and not passed
            ea = a
            if mutant == "sq_unsquared" and rays.sq and a == rays.sq[1]:
                ea = rays.sq[0]
            E, relE, absE = c.E[r1, i, ea], c.relE[r1, i, a], c.absE[r1, i, a]
            im = float(rays.invmu[a])
            y = [B[k] * E[k] for k in range(last + 1)]
            Bf = [float(B[k]) for k in range(last + 1)]
            Ef = [float(E[k]) for k in range(last + 1)]
            dE = [Ef[k] * relE[k] + absE[k] for k in range(last + 1)]
            dy = [abs(float(y[k])) * (relB[k] + relE[k] + U) + Bf[k] * absE[k] for k in range(last + 1)]
            I, err, T = zero, 0.0, 0.0
            if rule == 0:
                for k in range(1, last + 1):
                    t = (B[k - 1] + B[k]) / 2 * (E[k - 1] - E[k])
                    I += t; T += abs(float(t))
                    err += ((Bf[k - 1] * relB[k - 1] + Bf[k] * relB[k]) / 2 * abs(Ef[k - 1] - Ef[k])
                            + (Bf[k - 1] + Bf[k]) / 2 * (dE[k - 1] + dE[k]) + 4 * U * abs(float(t)))
                err += (last + 1) * U * T
            elif rule == 2:
                for k in range(1, last + 1):
                    h = tau[k] - tau[k - 1]
                    t = (y[k - 1] + y[k]) / 2 * h * mpf(im)
                    I += t; T += abs(float(t))
                    err += im * ((dy[k - 1] + dy[k]) / 2 * abs(float(h)) + abs(float(y[k - 1] + y[k])) / 2 * dh[k]) + 5 * U * abs(float(t))
                err += (last + 1) * U * T
            else:
                xs, ys, dys, hs, dhs = list(tau[:last + 1]), list(y), list(dy), [], []
                for k in range(1, last + 1):
                    hs.append(tau[k] - tau[k - 1]); dhs.append(dh[k])
                pad = not deck and last + 1 < L
                if mutant == "pad_on_bottom" and last + 1 >= L and not deck:
                    pad = True
                if mutant == "pad_with_deck" and deck and last + 1 < L:
                    pad = True
                if pad:
                    p = 1 / mpf(im) if (cut == "slant" and mutant != "pad_vertical") else mpf(1)
                    hs.append(p); dhs.append((2 * U * (abs(float(tau[last])) + float(p)) + U * float(p)) * SLACK)
                    ys.append(zero); dys.append(0.0)
                if mutant == "zero_width":
                    pts = list(tau[:last + 1]) + ([tau[last]] if pad else [])
                    hs = [h if h != 0 else mpf(U) * pts[j + 1] for j, h in enumerate(hs)]
                n = len(ys)
                s, serr, sT = zero, 0.0, 0.0

                def trap(j):
                    v = hs[j] / 2 * (ys[j] + ys[j + 1])
                    a_ = abs(float(hs[j])) / 2 * (abs(float(ys[j])) + abs(float(ys[j + 1])))
                    return v, dhs[j] / 2 * (abs(float(ys[j])) + abs(float(ys[j + 1]))) + abs(float(hs[j])) / 2 * (dys[j] + dys[j + 1]) + 4 * U * a_, a_

                start = 0
                even = (n & 1) == 0
                if mutant == "parity":
                    even = not even
                if n >= 2 and even:
                    v, e_, a_ = trap(0)
                    s += v; serr += e_; sT += a_
                    start = 1
                j = start
                while j + 2 <= n - 1:
                    h0, h1 = hs[j], hs[j + 1]
                    if h0 == 0 or h1 == 0 or mutant == "trapezoids":
                        for jj in (j, j + 1):
                            v, e_, a_ = trap(jj)
                            s += v; serr += e_; sT += a_
                    else:
                        w = _panel_w(h0, h1)
                        f0, f1, fs = float(h0), float(h1), float(h0 + h1)
                        wf = [abs(float(x)) for x in w]
                        d0, d1 = dhs[j], dhs[j + 1]
                        q0, q2 = abs(f1 / f0), abs(f0 / f1)
                        rnd = 2 * RCP + 10 * U
                        canc = (RCP + 2 * U) * abs(fs) / 6
                        dw = [(1 / 3 + q0 * q0 / 6) * d0 + abs(1 / 6 - f1 / (3 * f0)) * d1 + rnd * wf[0] + canc * q0,
                              wf[1] * (abs(3 / fs - 1 / f0) * d0 + abs(3 / fs - 1 / f1) * d1) + rnd * wf[1],
                              (1 / 3 + q2 * q2 / 6) * d1 + abs(1 / 6 - f0 / (3 * f1)) * d0 + rnd * wf[2] + canc * q2]
                        yy = [abs(float(ys[j + m])) for m in range(3)]
                        a_ = sum(wf[m] * yy[m] for m in range(3))
                        s += w[0] * ys[j] + w[1] * ys[j + 1] + w[2] * ys[j + 2]
                        serr += sum(dw[m] * yy[m] + wf[m] * dys[j + m] for m in range(3)) + 4 * U * a_
                        sT += a_
                    j += 2
                I = s * mpf(im)
                T = im * sT
                err = im * (serr + (n + 1) * U * sT) + U * abs(float(I))
            err += U * abs(float(I))
            if deck and mutant != "deck_dropped":
                kd = last - 1 if (mutant == "deck_above" and last >= 1) else last
                I += y[kd]; err += dy[kd]; T += abs(float(y[kd]))
            out["last"].append(last); out["deck"].append(deck); out["I"].append(I); out["dI"].append(err * SLACK); out["T"].append(T)
        w = rays.wgt
        out["F"] = sum((mpf(float(w[a])) * out["I"][a] for a in range(rays.A)), zero)
        out["dF"] = (sum(w[a] * out["dI"][a] for a in range(rays.A)) + (2 * rays.A + 6) * U * sum(w[a] * out["T"][a] for a in range(rays.A))) * SLACK
    return out


def undecided(c: Col, i, rule, cut):
    """[(ray, layer)]: the layers at or above a ray's cut (the deck layer's decision included) whose exact tau lies
    within its bound of the ray's threshold -- a correct evaluation may decide them either way."""
    r1 = rule == 1
    tau, dtau = c.tau[r1, i], c.dtau[r1, i]
    bad = []
    for a in range(c.rays.A if cut == "slant" else 1):
        thr = float(c.rays.thr[a]) if cut == "slant" else c.toomuch
        last, _ = cut_of(tau, mpf(thr), c.kend)
        for k in range(1, last + 1):
            if abs(float(tau[k] - mpf(thr))) <= dtau[k]:
                bad.append((a, k))
    return bad


def outcomes(c: Col, i, rule, cut):
    """The column under every outcome of its undecided decisions taken one at a time (the exact one first)."""
    res = [solve(c, i, rule, cut)]
    for a, k in undecided(c, i, rule, cut):
        r1 = rule == 1
        thr = mpf(float(c.rays.thr[a])) if cut == "slant" else mpf(c.toomuch)
        exact_passed = c.tau[r1, i][k] > thr
        if exact_passed:       # the other outcome: not passed on k, the walk goes on below
            last, passed = c.kend, False
            for kk in range(k + 1, c.kend + 1):
                if c.tau[r1, i][kk] > thr:
                    last, passed = kk, True
                    break
        else:
            last, passed = k, True
        rays_ = range(c.rays.A) if cut == "vertical" else [a]
        res.append(solve(c, i, rule, cut, last_override={r: (last, passed) for r in rays_}))
    return res


def mutants(c: Col, i, rule, cut):
    """{name: F mpf} of column i under each deliberate mistake that changes anything on it."""
    base = solve(c, i, rule, cut)
    out = {}
    for m in MUTANTS:
        for ray in (range(c.rays.A) if m == "cut_late" else [0]):
            r = solve(c, i, rule, cut, mutant=m, ray=ray)
            if r["F"] != base["F"]:
                out[m if m != "cut_late" else "cut_late%d" % ray] = r["F"]
    return out


def absdev(got, ref):
    with mpmath.workdps(DPS):
        return abs(mpf(float(got)) - ref)
