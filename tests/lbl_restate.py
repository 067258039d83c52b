"""The line-by-line Voigt extinction of one layer state (csrc/lbl.hip) restated in mpmath at 34 digits -- TEST
INFRASTRUCTURE ONLY.

Written from the header comment of lbl.hip and from the sampling / width-grid conventions in the docstring of
oracle/lbl_oracle.py; it shares nothing with either beyond the constants' values, each taken as the double the engine
holds (prep_restate._c).  The inputs are the doubles the engine reads, taken exactly; nothing is rounded before the
result.  Per line j of isotope i at a state (T, p, q):

  dop_i = sqrt(2 ln2 k T / m_i) / c                       aD = nu_j dop_i
  aL_i  = sqrt(2) / (c sqrt(pi k T)) p sum_{c in H2, He} q_c ((d + d_c) / 2)^2 sqrt(1 / m_i + 1 / m_c)
  Z_i(T): linear on the database's temperature grid, the end values outside it (one node: that value)
  scale = ratio_i q_mol p / (k T) / Z_i       or, per gram of the molecule,   ratio_i / (Z_i m_mol amu)
  S_j   = SIGCTE gf_j scale exp(max(-hc E_j / kT, -708)) (1 - exp(max(-hc nu_j / kT, -708)))
  kept:   S_j >= ethresh max_j S_j (the maximum over the database's lines, wherever they lie) and S_j > 0
  e(nu) += S_j sqrt(ln2 / pi) / aD  Re w(sqrt(ln2) (|nu - nu_j| + i aL) / aD)     for |nu - nu_j| <= nwidth max(aD, aL)

with w(z) = exp(-z^2) erfc(-i z).  Oversampled states (dv > 1: the smallest divisor of wnosamp with wndelt / dv <= half
the narrowest half-width, max(wn_first dop_i, aL_i) over the isotopes) are summed on the fine grid wn_first + k wndelt /
dv and reduced: odd dv a mean of dv points, even dv of dv + 1 points with half-weight ends, the window clipped to the
full grid and normalised by the weights it keeps.  Width-grid mode: a line takes the profile of the nearest grid
widths (nearest in the logarithm), centred on the sampling point nearest to its centre (floor(t + 1/2)), reaching
floor(nwidth max(gd, gl) / step) points either side.

The sampling points are the only doubles formed here in fp64: wn_first + k * step with the product and the sum rounded
one after the other, as lbl.hip states it does -- two IEEE operations Python's floats repeat to the bit.

THE BOUND.  Every term of a point's sum is positive, so |device - exact| <= sum_terms term * eps_term + n u sum (n
additions, each rounding at most u = 2^-53 of a partial sum <= the sum).  eps_term is the sum of

  branch claim .... what lbl.hip documents for the branch (x, y) falls in (CLAIM below); where a point lies within 1e-13
                    of a branch seam, the larger of the two.  Beyond |z| = 8 with y < 1 an absolute 2 exp(y^2 - x^2) is
                    added to K: the series drop the exp(-z^2) term (on the real axis Re w = exp(-x^2), the series give 0)
  K's roundings ... counted per branch (ROUND_*): far 12 operations and one rcp_n1 (2.2e-15); the series 2 NT + 10
                    operations and rcp_n1 three times over (inv^2 in t, inv in the result); Weideman 80; the Taylor
                    branch 7 per order, plus the cancellation in a_1 = 2 x y D - 2 y / sqrt(pi) (D ~ (1 + 1/2x^2) /
                    (sqrt(pi) x): two roundings of a term 2 x^2 + 1 times the difference), plus exp_rt_fma3's 7e-14
  arguments ....... x carries NX = 10 roundings (dop: m_i amu, three products, a quotient, sqrt halves those and adds
                    its own, / c: 5; nu_j dop: 6; sqrt(ln2)_d / aD: 7.5; |nu - nu_j| and the product: 9.5), y NY = 25
                    (aL: sqrt(2) / (c sqrt(pi k T)): 5, p: 1, the collider sum: 9, its product: 1 -- 16; times xs:
                    24.5).  They enter through the exact partial derivatives, which the recurrence w' = -2 z w + 2 i /
                    sqrt(pi) gives for free: (|x K_x| NX + |y K_y| NY) u / K
  amplitude ....... NA = 10 (aD: 6, three operations, the two constants) and the strength: N_SCALE = 13 roundings of
                    scale (Z: 4, n = p / kT: 2, three operations, SIGCTE), the two products and the difference, and for
                    each exponential exp_core's documented error (1.7e-17 of the interpolant, 4e-16 held on the device by
                    tests/test_gpu_rt_math.py) plus three roundings of its argument, |a| 3 u; the second one times
                    e^b / (1 - e^b)
  the product ..... amp * K: u.

Reduction of an oversampled state: the weighted bounds, plus (dv + 2) u of the value (dv + 1 fused steps on positive
numbers and the quotient).  Width-grid profiles: x has 4 roundings, y and amp 3 (the grid widths are inputs; an ulp of
libm between the engine's exp/log and numpy's is counted as one of them).

DECISIONS the device takes in doubles cannot be repeated exactly; one closer to its threshold than the roundings of the
compared quantities is UNDECIDED and widens the point's interval to "with and without":

  cut ............. |nu - nu_j| (u) against nwidth max(aD, aL) (17 u): D_CUT = 32 u
  threshold ....... S_j against ethresh max S: both strengths' eps (above) plus 2 u
  dv .............. wndelt / k (u) against wmin / 2 (17 u): D_DV = 32 u; the whole state is undecided
  nearest node .... t = (ln a - ln0) / dln + 1/2 within (NY u + 4 u (|ln a| + |ln0|)) / dln + 2 u |t| of an integer
  centre, reach ... (nu_j - wn_first) dv / wndelt + 1/2, and nwidth max(gd, gl) / step, within 4 u of an integer
                    (relative to the value).

An undecided pair adds its term to the interval's lower or upper slack; an undecided width-grid line (node, centre or
reach) is taken out of the lower end and put back at its profile's peak in the upper end over every point either
placement can reach.  `Result` carries value, bound, lo, hi and the undecided flag per output point."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import mpmath
import numpy as np

from prep_restate import AMU, H, KB, LS, PI_DOUBLE, _c

DPS = 34
U = 2.0 ** -53
SIGCTE, LN2_D, SQRT_LN2_D, INV_SQRT_PI_D = 8.852821681767784e-13, 0.6931471805599453, 0.8325546111576977, 0.5641895835477563
EXPCTE_D = float(H) * float(LS) / float(KB)        # kEXPCTE: a constexpr product and quotient of doubles
EXP_MIN = -708.0
# what csrc/lbl.hip documents per branch of voigt_k / voigt_far (relative)
CLAIM = dict(taylor=2.5e-12, asym11=2.6e-12, asym6=3.8e-12, weideman=3e-13, far=1.4e-11)
EPS_EXP_CORE = 1.7e-17 + 4e-16
EPS_EXP_RT = 7e-14
EPS_RCP_N1 = 2.2e-15
NX, NY, NA, N_SCALE = 10, 25, 10, 13
D_CUT = D_DV = 32 * U
SEAM = 1e-13
TAYLOR_YMAX = 0.13
ORDER_STEPS = (6.0e-6, 5.0e-4, 3.0e-3, 9.5e-3, 2.2e-2, 4.0e-2, 6.5e-2, 9.5e-2)
BRANCHES = ("taylor", "weideman", "asym11", "asym6", "far")

mp = mpmath.mp.clone()
mp.dps = DPS
mpf = mp.mpf


@dataclass
class Setup:
    """What the line-by-line path reads besides the profile.  press: barye, atm order; mass: amu, diam: cm, per species;
    dbs: per database dict(species index `sp`, temps[nt], isotopes [(mass, ratio, Z[nt])], wn, iso, elow, gf) -- the
    lines the engine keeps (within 500 cm-1 of the grid).  wn: the engine's LOCAL output points, i_off their first
    index on the full grid of wfull points wn_first + i wndelt.  grid: None, or dict(dgrid, lgrid, d_ln0, d_dln, l_ln0,
    l_dln) of the width-grid mode."""
    press: np.ndarray
    mass: np.ndarray
    diam: np.ndarray
    iH2: int
    iHe: int
    dbs: list
    nwidth: float
    ethresh: float
    wn: np.ndarray
    wn_first: float
    wndelt: float
    wfull: int
    i_off: int = 0
    osamp: int = 1
    grid: dict | None = None


@dataclass
class Result:
    value: list                 # mpf per output point
    bound: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    undecided: np.ndarray
    pairs: int = 0              # (line, sampling point) pairs evaluated
    by_branch: dict = field(default_factory=dict)

    @property
    def v(self):
        return np.array([float(x) for x in self.value])


def voigt_order(y):
    return 0 if not y <= TAYLOR_YMAX else 2 + sum(y > s for s in ORDER_STEPS)


def branch_of(x, y):
    """The branch voigt_k takes for the doubles (x, y), by its own comparisons."""
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    if r2 >= 1.0e4:
        return "far"
    if r2 >= 64.0:
        return "asym6" if r2 >= 289.0 else "asym11"
    return "taylor" if voigt_order(y) else "weideman"


def _near(a, b):
    return abs(a - b) <= SEAM * b


def branches_near(x, y):
    """branch_of, and the neighbour's too where (x, y) lies within SEAM of a seam."""
    out = {branch_of(x, y)}
    r2 = x * x + y * y
    for s, pair in ((1.0e4, ("far", "asym6")), (289.0, ("asym6", "asym11"))):
        if _near(r2, s):
            out |= set(pair)
    if _near(r2, 64.0):
        out |= {"asym11", "taylor" if voigt_order(y) else "weideman"}
    if r2 < 64.0 * (1 + SEAM) and _near(y, TAYLOR_YMAX):
        out |= {"taylor", "weideman"}
    return out


def round_of(branch, x, y):
    """K's own counted roundings per branch (module docstring)."""
    if branch == "far":
        return 12 * U + EPS_RCP_N1
    if branch in ("asym11", "asym6"):
        return (2 * (11 if branch == "asym11" else 6) + 10) * U + 3 * EPS_RCP_N1
    if branch == "weideman":
        return 80 * U
    return (7 * max(voigt_order(y), 2) + 2 * (2 * x * x + 1)) * U + EPS_EXP_RT + x * x * U


def eps_k(x, y):
    """Relative claim + roundings of the device's K at the doubles (x, y)."""
    return max(CLAIM[b] + round_of(b, x, y) for b in branches_near(x, y))


class Faddeeva:
    """K = Re w(x + i y) and its partial derivatives, cached per (x, y); `scale`: a branch whose K is multiplied by
    1 + 1e-10 (the mutants of tests/test_lbl_restate_cpu.py)."""

    def __init__(self, scale=None, cache=None):
        self.cache, self.scale, self.calls = ({} if cache is None else cache), scale, 0

    def __call__(self, x, y):
        key = (x, y)
        hit = self.cache.get(key)
        if hit is None:
            if y == 0:
                # on the real axis Re w = exp(-x^2) (K_y is only ever multiplied by y)
                e = mp.exp(-x * x)
                hit = self.cache[key] = (e, -2 * x * e, mpf(0))
            else:
                # mpmath delivers w to DPS digits of its MODULUS (~ 1 / (sqrt(pi) |z|) in the wings); the real part is
                # as small as max(exp(-x^2), y / (sqrt(pi) |z|^2)): that many digits more
                xf, yf = float(x), float(y)
                lg = max(-xf * xf / math.log(10.0), math.log10(yf) - math.log10(1.0 + xf * xf + yf * yf))
                with mp.workdps(DPS + max(0, int(-lg)) + 6):
                    z = mp.mpc(x, y)
                    w = mp.exp(-z * z) * mp.erfc(mp.mpc(y, -x))
                    wp = -2 * z * w + mp.mpc(0, 2) / mp.sqrt(mp.pi)
                    hit = self.cache[key] = (+w.real, +wp.real, -wp.imag)
            self.calls += 1
        if self.scale and branch_of(float(x), float(y)) == self.scale:
            return hit[0] * (1 + mpf("1e-10")), hit[1], hit[2]
        return hit


def _nearest_int_margin(t):
    """Distance of t from the nearest point where floor(t) steps, i.e. from an integer."""
    return float(abs(t - mp.nint(t)))


class Restatement:
    """One Setup; `mutant`: a name of MUTANTS (a deliberately wrong restatement, for the CPU tests)."""

    def __init__(self, su: Setup, mutant=None, fad=None):
        self.su, self.m = su, mutant
        scale = mutant[2:] if mutant and mutant.startswith("k_") else None
        if scale is not None:
            self.fad = Faddeeva(scale, None if fad is None else fad.cache)      # (the exact values are shared)
        else:
            self.fad = fad if fad is not None else Faddeeva()
        self.kb, self.amu, self.c = _c(KB), _c(AMU), _c(LS)
        self.ln2, self.sl2, self.isp, self.sig = mpf(LN2_D), mpf(SQRT_LN2_D), mpf(INV_SQRT_PI_D), mpf(SIGCTE)
        self.pi, self.expcte = mpf(PI_DOUBLE), mpf(EXPCTE_D)

    # ---- the state -------------------------------------------------------------------------------------------------
    def partition(self, temps, Z, T):
        nt = len(temps)
        if self.m == "z_nearest":
            return mpf(float(Z[int(np.argmin(np.abs(np.asarray(temps) - T)))]))
        if nt == 1 or T <= temps[0]:
            return mpf(float(Z[0]))
        if T >= temps[nt - 1]:
            return mpf(float(Z[nt - 1]))
        j = 0
        while j < nt - 2 and temps[j + 1] <= T:
            j += 1
        f = (mpf(T) - mpf(float(temps[j]))) / (mpf(float(temps[j + 1])) - mpf(float(temps[j])))
        return mpf(float(Z[j])) * (1 - f) + mpf(float(Z[j + 1])) * f

    def state(self, T, p, q, per_gram=False):
        """-> dict: dop, lor, scale (SIGCTE * scale) per isotope in database order (mpf), group per isotope, dv, and
        dv_margin (the smallest relative distance of a divisor's comparison from its threshold; inf without one)."""
        su = self.su
        T_, p_ = mpf(float(T)), mpf(float(p))
        dop, lor, scale, group = [], [], [], []
        for g, db in enumerate(su.dbs):
            sp = db["sp"]
            for (mass, ratio, Z) in db["isotopes"]:
                mi = mpf(float(mass)) * self.amu
                two_ln2 = 2 if self.m == "no_ln2" else 2 * self.ln2
                dop.append(mp.sqrt(two_ln2 * self.kb * T_ / mi) / self.c)
                s = mpf(0)
                for c in (su.iH2, su.iHe):
                    if c >= 0:
                        dd = (mpf(float(su.diam[sp])) + mpf(float(su.diam[c]))) / 2
                        s += mpf(float(q[c])) * dd * dd * mp.sqrt(1 / mi + 1 / (mpf(float(su.mass[c])) * self.amu))
                lor.append(mp.sqrt(2) / (self.c * mp.sqrt(self.pi * self.kb * T_)) * p_ * s)
                Zt = self.partition(db["temps"], Z, float(T))
                if per_gram:
                    sc = mpf(float(ratio)) / (Zt * mpf(float(su.mass[sp])) * self.amu)
                else:
                    sc = mpf(float(ratio)) * mpf(float(q[sp])) * p_ / (self.kb * T_) / Zt
                scale.append(self.sig * sc)
                group.append(g)
        dv, margin = 1, math.inf
        if su.osamp > 1:
            wmin = min(max(mpf(float(su.wn_first)) * d, a) for d, a in zip(dop, lor))
            dv = su.osamp
            for k in range(1, su.osamp + 1):
                if su.osamp % k:
                    continue
                ratio_ = mpf(float(su.wndelt)) / k / (wmin / 2)
                margin = min(margin, float(abs(ratio_ - 1)))
                if ratio_ <= 1:
                    dv = k
                    break
        return dict(T=T_, dop=dop, lor=lor, scale=scale, group=group, dv=dv, dv_margin=margin)

    def strengths(self, st, g):
        """Per line of database g: (S, eps_S) -- eps_S the relative error bound of the device's strength."""
        db = self.su.dbs[g]
        first = st["group"].index(g)
        out = []
        for nu0, iso, elow, gf in zip(db["wn"], db["iso"], db["elow"], db["gf"]):
            a = max(-self.expcte * mpf(float(elow)) / st["T"], mpf(EXP_MIN))
            b = max(-self.expcte * mpf(float(nu0)) / st["T"], mpf(EXP_MIN))
            eb = mp.exp(b)
            stim = 1 if self.m == "no_stim" else 1 - eb
            S = mpf(float(gf)) * st["scale"][first + int(iso)] * mp.exp(a) * stim
            eps = (N_SCALE + 4) * U + (abs(float(a)) * 3 * U + EPS_EXP_CORE) \
                + (abs(float(b)) * 3 * U + EPS_EXP_CORE) * float(eb / (1 - eb))
            out.append((S, eps))
        return out

    def kept(self, st):
        """Per database: [(line index, S, eps_S, kept, undecided)] of the lines that are kept or undecided, and smax."""
        su = self.su
        all_S = [self.strengths(st, g) for g in range(len(su.dbs))]
        smax = [max([s for s, _ in ss], default=mpf(0)) for ss in all_S]
        out = []
        for g, ss in enumerate(all_S):
            ref = max(smax) if self.m == "thresh_all" else smax[g]
            eps_max = max([e for s, e in ss if s == smax[g]], default=0.0)
            lines = []
            for j, (S, eps) in enumerate(ss):
                if not S > 0:
                    continue
                th = mpf(float(su.ethresh)) * ref
                keep = S >= th
                und = S != ref and float(abs(S / th - 1)) < eps + eps_max + 2 * U
                if keep or und:
                    lines.append((j, S, eps, bool(keep), bool(und)))
            out.append(lines)
        return out, smax

    # ---- sampling ---------------------------------------------------------------------------------------------------
    def fine_points(self, dv):
        """(first fine index, the points as doubles) covering the local block's reduction windows."""
        su = self.su
        h = dv // 2
        kmax = (su.wfull - 1) * dv
        ka, kb = max(su.i_off * dv - h, 0), min((su.i_off + len(su.wn) - 1) * dv + h, kmax)
        step = su.wndelt / dv
        return ka, [su.wn_first + float(k) * step for k in range(ka, kb + 1)]

    def reduce(self, ka, dv, val, bnd, minus, plus):
        su = self.su
        if dv == 1:
            o = su.i_off - ka
            n = len(su.wn)
            return val[o:o + n], bnd[o:o + n], minus[o:o + n], plus[o:o + n]
        h, kmax = dv // 2, (su.wfull - 1) * dv
        even = dv % 2 == 0 and self.m != "odd_for_even"
        if self.m == "odd_for_even" and dv % 2 == 0:
            h = (dv - 1) // 2
        out = ([], [], [], [])
        for i in range(len(su.wn)):
            c = (su.i_off + i) * dv
            acc, ws = [mpf(0), 0.0, 0.0, 0.0], mpf(0)
            for f in range(max(c - h, 0), min(c + h, kmax) + 1):
                w = mpf("0.5") if even and f in (c - h, c + h) and self.m != "ends_full" else mpf(1)
                ws += w
                acc[0] += w * val[f - ka]
                for n_, arr in ((1, bnd), (2, minus), (3, plus)):
                    acc[n_] += float(w) * arr[f - ka]
            v = acc[0] / ws
            out[0].append(v)
            out[1].append(acc[1] / float(ws) + (dv + 2) * U * float(v))
            out[2].append(acc[2] / float(ws))
            out[3].append(acc[3] / float(ws))
        return out

    # ---- one state ----------------------------------------------------------------------------------------------------
    def layer(self, T, p, q, per_gram=False, groups=None) -> Result:
        """The extinction of one state on the local output points, summed over `groups` (default: all databases)."""
        st = self.state(T, p, q, per_gram)
        dv = st["dv"]
        ka, pts = (self.su.i_off, [float(v) for v in self.su.wn]) if dv == 1 else self.fine_points(dv)
        n = len(pts)
        acc = dict(val=[mpf(0)] * n, bnd=[0.0] * n, minus=[0.0] * n, plus=[0.0] * n, cnt=[0] * n, pairs=0, br={})
        lines, _ = self.kept(st)
        for g, ls in enumerate(lines):
            if groups is not None and g not in groups:
                continue
            if self.su.grid is None:
                self._exact(st, g, ls, pts, acc)
            else:
                self._grid(st, g, ls, ka, dv, n, acc)
        bnd = [b + c * U * float(v) for b, c, v in zip(acc["bnd"], acc["cnt"], acc["val"])]
        val, bnd, minus, plus = self.reduce(ka, dv, acc["val"], bnd, acc["minus"], acc["plus"])
        bnd, minus, plus = np.array(bnd), np.array(minus), np.array(plus)
        v = np.array([float(x) for x in val])
        und = (minus > 0) | (plus > 0)
        if st["dv_margin"] < D_DV:
            und[:] = True
        return Result(list(val), bnd, v - bnd - minus, v + bnd + plus, und, acc["pairs"], acc["br"])

    def _exact(self, st, g, ls, pts, acc):
        su = self.su
        db = su.dbs[g]
        first = st["group"].index(g)
        P = np.asarray(pts)
        nw = mpf(float(su.nwidth))
        for (j, S, eps_S, keep, und_line) in ls:
            nu0 = float(db["wn"][j])
            i = first + int(db["iso"][j])
            aD, aL = mpf(nu0) * st["dop"][i], st["lor"][i]
            cut = nw * max(aD, aL)
            xs = self.sl2 / aD
            amp = S * self.sl2 * self.isp / aD
            aDy = mpf(float(su.wn_first)) * st["dop"][i] if self.m == "y_lowend" else aD
            y = aL * self.sl2 / aDy
            yf, cf = float(y), float(cut)
            a, b = np.searchsorted(P, [nu0 - cf * (1 + 2 * D_CUT), nu0 + cf * (1 + 2 * D_CUT)])
            for k in range(max(a - 1, 0), min(b + 1, len(P))):
                dx = abs(mpf(pts[k]) - mpf(nu0))
                inside = dx <= cut
                near = float(abs(dx / cut - 1)) < D_CUT
                if not inside and not near:
                    continue
                x = dx * xs
                K, Kx, Ky = self.fad(x, y)
                acc["pairs"] += 1
                xf = float(x)
                br = branch_of(xf, yf)
                acc["br"][br] = acc["br"].get(br, 0) + 1
                term = float(amp * K)
                floor = 2 * math.exp(min(yf * yf - xf * xf, 0.0)) * float(amp) if (xf * xf + yf * yf >= 64 * (1 - SEAM) and yf < 1) else 0.0
                sens = (float(abs(x * Kx)) * NX + float(abs(y * Ky)) * NY) * U * float(amp)
                eps = eps_k(xf, yf) + (NA + 1) * U + eps_S
                if inside and keep:
                    acc["val"][k] = acc["val"][k] + amp * K
                    acc["bnd"][k] += term * eps + sens + floor
                    acc["cnt"][k] += 1
                    if near or und_line:
                        acc["minus"][k] += term
                else:
                    acc["plus"][k] += term * (1 + eps) + sens + floor

    def _node(self, a, ln0, dln, grid):
        """(nearest index, undecided) of half-width a (mpf) on a width grid."""
        n = len(grid)
        if n <= 1 or not dln > 0:
            return 0, False
        if not a > 0:
            return 0, False                     # ln 0 = -inf: below the first node
        if self.m == "nearest_linear":
            return int(np.argmin(np.abs(np.asarray(grid) - float(a)))), False
        la = mp.log(a)
        t = (la - mpf(float(ln0))) / mpf(float(dln)) + mpf("0.5")
        tol = (NY * U + 4 * U * (abs(float(la)) + abs(ln0))) / dln + 2 * U * abs(float(t))
        und = _nearest_int_margin(t) < tol and -1 < float(t) < n + 1
        return int(min(max(mp.floor(t), 0), n - 1)), und

    def _profile(self, iD, iL, o, step):
        gr = self.su.grid
        gd, gl = mpf(float(gr["dgrid"][iD])), mpf(float(gr["lgrid"][iL]))
        x, y = self.sl2 * (o * mpf(step)) / gd, self.sl2 * gl / gd
        K, Kx, Ky = self.fad(x, y)
        xf, yf = float(x), float(y)
        amp = self.sl2 * self.isp / gd
        floor = 2 * math.exp(min(yf * yf - xf * xf, 0.0)) if (xf * xf + yf * yf >= 64 * (1 - SEAM) and yf < 1) else 0.0
        eps = eps_k(xf, yf) + 4 * U + float(abs(x * Kx) * 4 + abs(y * Ky) * 3) * U / max(float(K), 1e-300)
        return amp * K, eps, float(amp) * floor, branch_of(xf, yf)

    def _grid(self, st, g, ls, ka, dv, n, acc):
        su, gr = self.su, self.su.grid
        db = su.dbs[g]
        first = st["group"].index(g)
        step = su.wndelt / dv
        inv_step = mpf(dv) / mpf(float(su.wndelt))
        for (j, S, eps_S, keep, und_line) in ls:
            nu0 = float(db["wn"][j])
            i = first + int(db["iso"][j])
            iD, uD = self._node(mpf(nu0) * st["dop"][i], gr["d_ln0"], gr["d_dln"], gr["dgrid"])
            iL, uL = self._node(st["lor"][i], gr["l_ln0"], gr["l_dln"], gr["lgrid"])
            gmax = max(float(gr["dgrid"][iD]), float(gr["lgrid"][iL]))
            reach = mpf(float(su.nwidth)) * mpf(gmax) / mpf(step)
            K = int(mp.floor(reach)) - (1 if self.m == "reach_short" else 0)
            t = (mpf(nu0) - mpf(float(su.wn_first))) * inv_step + (0 if self.m == "kc_floor" else mpf("0.5"))
            kc = int(mp.floor(t))
            und = und_line or uD or uL or _nearest_int_margin(reach) < 4 * U * float(reach) \
                or _nearest_int_margin(t) < 4 * U * max(abs(float(t)), 1.0)
            lo, hi = max(kc - K, ka), min(kc + K, ka + n - 1)
            if und:
                # either placement: out of the lower end, back at the profile's peak over a reach one node wider
                # (a neighbouring node's widths differ by exp(dln) at most: so do the peak, ~ 1 / width, and the reach)
                wider = math.exp(max(gr["d_dln"], gr["l_dln"]))
                peak = float(S * self._profile(iD, iL, 0, step)[0]) * wider
                K2 = int(K * wider) + 2
                for k in range(max(kc - K2 - 1, ka), min(kc + K2 + 1, ka + n - 1) + 1):
                    acc["plus"][k - ka] += peak
            if not keep:
                continue
            for k in range(lo, hi + 1):
                P, eps_p, floor, br = self._profile(iD, iL, abs(k - kc), step)
                acc["pairs"] += 1
                acc["br"][br] = acc["br"].get(br, 0) + 1
                term = float(S * P)
                acc["val"][k - ka] = acc["val"][k - ka] + S * P
                acc["bnd"][k - ka] += term * (eps_p + eps_S + U) + float(S) * floor
                acc["cnt"][k - ka] += 1
                if und:
                    acc["minus"][k - ka] += term

    def extinction(self, prof, per_gram=False, layers=None):
        """prof [(S+1), L] -> list of Result per layer (atm order); `layers`: only these."""
        prof = np.asarray(prof, float).reshape(len(self.su.mass) + 1, -1)
        return {l: self.layer(prof[0, l], self.su.press[l], prof[1:, l], per_gram)
                for l in (range(prof.shape[1]) if layers is None else layers)}


MUTANTS = ("no_stim", "no_ln2", "z_nearest", "thresh_all", "ends_full", "odd_for_even", "nearest_linear", "kc_floor",
           "reach_short", "y_lowend") + tuple("k_" + b for b in BRANCHES)
