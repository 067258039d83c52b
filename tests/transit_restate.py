"""The transit column (csrc/transit_geom.hip) restated in mpmath at 50 digits -- TEST INFRASTRUCTURE ONLY.

It shares nothing with transit_geom.hip or oracle/rt_oracle.c beyond the definitions in the header comment of
transit_geom.hip.  Inputs are the doubles the kernels read, each taken exactly: the walker's layer records
(engine.prep_records), the table values at the records' offsets (from the case's files, through the oracle's readers),
the radii top to bottom, wn, toomuch, transparent, starrad; optionally ext[L, W] (atm order) for the line-by-line
form.  Layers and chords count from the top (k = 0 the top layer) throughout.

    e_k      = sum_t c_kt v_kt + ray_k nu^4 + grey_k (+ ext)                  extinction of layer k
    P_j      = e_{j-1} + e_j                                                   pair sums, j = 1 .. kend
    DS(k, j) = s_{j-1} - s_j,  s_j = sqrt(r_j^2 - r_k^2),  s_k = 0            j = 1 .. k
    tau_k    = sum_{j=1..k} P_j DS(k, j),  tau_0 = 0
    last     = the first k in 1 .. kend with tau_k > toomuch, else kend
    g_k      = exp(-tau_k) r_k,  g_0 = r_0
    M        = (r_0^2 - 2 sum_{k=1..last} (g_{k-1} + g_k) / 2 (r_{k-1} - r_k) - core) / R*^2,
    core     = transparent ? exp(-tau_last) r_last^2 : 0

The running error bounds (what a correct fp64 evaluation in the kernels' order of operations may differ by; first
order in u = 2^-53, every count rounded up, then 1e-6 of slack for the second order and for the bound's own fp64
sums).  DERIVED from the arithmetic below, never fitted to a device result:

  extinction.  Both kernels form nu^4 = (nu nu)(nu nu) (three roundings: 3 u on the Rayleigh term) and add the
    T = 2 M + 2 C + 2 (+ 1 with ext) terms in one chain, fused (rt_transit_mfma: one fma per term) or not (rt_transit:
    a product and an add).  A chain of T terms with rounded products is within (T + 1) u sum |terms|; with the 3 u of
    nu^4:  de_k <= (T + 4) u A_k,  A_k = sum_t |c v| + |ray nu^4| + |grey| + |ext|.
    The CIA planes are RESAMPLED tables: the engine and the oracle's reader each run a natural spline (or a linear
    interpolation) of the same file, so the values fed here are not bit for bit the device's.  That is an allowance
    on the INPUT, not on the kernel: 32 u of the file's linear-table terms, once more for its curvature table
    (both implementations solve the same diagonally dominant tridiagonal system; the curvature term is
    (a^3 - a) h^2 / 6 y'' with |a^3 - a| < 0.39, an error of k u |alpha| / h^2 in y'' is 0.07 k u of the linear term).
  pair sums.  One rounded add: dP_j <= de_{j-1} + de_j + u (A_{j-1} + A_j).
  chord table.  chord_table_fill: s = sqrt((r_j - r_k)(r_j + r_k)): difference, sum, product (3 u on the argument,
    1.5 u on its root) and the root itself, counted as one ulp (2 u): 3.5 u s.  Then one rounded difference:
    dDS(k, j) <= 3.5 u (s_{j-1} + s_j) + u DS(k, j)       (s_k = 0 exactly: the second root is not taken).
    With thin layers s_{j-1} + s_j is ~ 2 (k - j) + 1 times DS near the diagonal scale: the "4 (k - j) + const ulps"
    of cancellation, stated exactly.
  tau.  One accumulation chain per chord: the MFMA of row tile kt adds 16 kt + 16 products (zeros past the diagonal
    add exactly), the scalar kernel k fused ones, the oracle k rounded products and adds: at most
    n_k = 16 (k / 16 + 1) + 1 roundings on any term.
    dtau_k <= n_k u sum_j |P_j| DS(k, j) + sum_j (dP_j DS(k, j) + |P_j| dDS(k, j)).
  transmission.  The library exp of the scalar kernel and of the oracle is within one ulp (4e-16 is taken).  exp_rt
    of the matrix-tile kernel is within 4e-16 of ITS OWN FORMULA (tests/test_gpu_rt_math.py) -- a degree-9 interpolant
    that csrc/kernels.hpp states, and tests/test_rt_math_cpu.py holds, to 7.5e-14 + 2.4e-17 |n| of exp, n = the
    integer nearest x / ln2: |n| <= tau log2(e) + 1.  The reference here is exp itself, so that distance belongs to
    the matrix-tile kernel's bound (`exp_rt`): 4e-16 alone was an error of this derivation, found on paper after the
    first device run exceeded it under `transparent` by 1.5 - 3.4 bounds with the scalar kernel at 0.2 -- the figure
    is the header's, not the device's.  The argument's error passes through, d(exp) = dtau; one rounded product:
    dg_k <= g_k (4e-16 [+ 7.5e-14 + 2.4e-17 (1.4427 tau_k + 1)] + dtau_k (1 + dtau_k) + u)
    (g_0 = exp(-0) r_0 is held to the same).
  trapezoid.  r_{k-1} - r_k, g_{k-1} + g_k and their product round once each (the half is exact):
    dterm_k <= (dg_{k-1} + dg_k) / 2 (r_{k-1} - r_k) + 3 u term_k;
    `last` non-zero terms added in any order (the scalar chain; per lane over tiles, then a 16-lane tree) are within
    (last - 1) u sum term_k of their sum -- `last` u here.
  modulation.  r_0^2 rounds once, the two subtractions (the oracle: a square, three sums) once each on at most
    r_0^2 + 2 integ + core, the core's extra product once: 6 u (r_0^2 + 2 integ + core) + r_last dg_last + 2 dinteg;
    1 / R*^2 is a rounded square, a rounded reciprocal and the final product: 3 u |M|.
    With no absorber and `transparent` M cancels to 0: the bound is then ~ 12 u r_0^2 / R*^2, an ABSOLUTE bound in
    units of r_top^2 / R*^2, which is what a result near zero has to be held to.
"""
from __future__ import annotations

import mpmath
import numpy as np

DPS = 50
U = 2.0 ** -53
EXP_REL = 4e-16          # fp64 rounding of exp_rt's formula (tests/test_gpu_rt_math.py); one ulp of a library exp
EXP_RT_FIT, EXP_RT_LN2 = 7.5e-14, 2.4e-17     # exp_rt's interpolant from exp (csrc/kernels.hpp; tests/test_rt_math_cpu.py)
SQRT_REL = 2 * U         # one ulp
S_REL = 1.5 * U + SQRT_REL
CIA_ALLOW = 32 * U
SLACK = 1.0 + 1e-6
DECK_BIT = 1 << 30

_sqrt = np.frompyfunc(lambda x: mpmath.sqrt(x), 1, 1)
_exp = np.frompyfunc(lambda x: mpmath.exp(x), 1, 1)
_mp = np.frompyfunc(lambda x: mpmath.mpf(float(x)), 1, 1)
_fl = np.frompyfunc(float, 1, 1)


def mp_array(a):
    """Doubles -> object array of mpf, each taken exactly."""
    return _mp(np.asarray(a, float))


def to_float(a):
    return np.asarray(_fl(np.asarray(a, object)), float)


def kend_of(kstop: int) -> int:
    return int(kstop) & (DECK_BIT - 1)


class Chords:
    """The chord table of one walker's radii (doubles, top to bottom): ds[k] = DS(k, 0 .. k) as mpf (ds[k][0] = 0),
    dds[k] the bound on the device's entry, both as arrays of length k + 1."""

    def __init__(self, r):
        with mpmath.workdps(DPS):
            self.r = mp_array(r)
            L = len(self.r)
            r2 = self.r * self.r
            self.ds, self.dds, self.s = [], [], []
            for k in range(L):
                s = _sqrt(r2[:k + 1] - r2[k])
                s[k] = mpmath.mpf(0)
                d = np.empty(k + 1, object)
                d[0] = mpmath.mpf(0)
                d[1:] = s[:-1] - s[1:]
                sf = to_float(s)
                b = np.zeros(k + 1)
                b[1:] = (S_REL * (sf[:-1] + sf[1:]) + U * to_float(d[1:])) * SLACK
                self.s.append(s); self.ds.append(d); self.dds.append(b)

    def dense(self):
        """-> (DS[L, L] as floats rounded from the exact values, bound[L, L]); zero above the diagonal and in column 0."""
        L = len(self.r)
        d, b = np.zeros((L, L)), np.zeros((L, L))
        for k in range(L):
            d[k, :k + 1], b[k, :k + 1] = to_float(self.ds[k]), self.dds[k]
        return d, b

    def exact_minus(self, table):
        """|table[k, j] - DS(k, j)| at 50 digits, [L, L] (above the diagonal: |table|)."""
        L = len(self.r)
        out = np.abs(np.asarray(table, float)).copy()
        with mpmath.workdps(DPS):
            for k in range(L):
                out[k, :k + 1] = to_float(abs(mp_array(table[k, :k + 1]) - self.ds[k]))
        return out


def table_inputs(o, coef, idx, cols, wn=None):
    """The terms of the extinction of one walker's records on the columns `cols`, from the case's files through the
    oracle engine `o` (its readers: the opacity grid as the file holds it, the CIA planes resampled on the grid):
    -> (c[L, T] doubles, v[L, T, ncol] mpf, allow[L, T] relative input allowances), T = 2 M + 2 C + 2 in the records'
    order, the Rayleigh term's value being nu^4 (exact) and the grey term's 1."""
    coef, idx, cols = np.asarray(coef, float), np.asarray(idx), np.asarray(cols, int)
    L, M, W, Nt = coef.shape[0], len(o.opmol), len(o.wn), len(o.tgrid)
    Cn = (coef.shape[1] - 4 - 2 * M) // 2
    assert idx.shape == (L, 1 + Cn) and coef.shape[1] == 4 + 2 * M + 2 * Cn
    wn = np.asarray(o.wn if wn is None else wn, float)
    tabs, off = [], 0
    spline = bool(o.c.cia_spline)
    for f in range(len(o.cia_nt) if o.c.ncia else 0):
        nt = int(o.cia_nt[f])
        tabs.append((np.asarray(o.cia_alpha)[off:off + nt], 0))
        if spline:
            tabs.append((np.asarray(o.cia_y2)[off:off + nt], 1))
        off += nt
    assert len(tabs) == Cn, (len(tabs), Cn)
    poff = np.concatenate([[0], np.cumsum([max(len(t) - 1, 1) for t, _ in tabs])]).astype(int)
    T = 2 * M + 2 * Cn + 2
    c = coef[:, 2:].copy()
    v = np.zeros((L, T, len(cols)))
    allow = np.zeros((L, T))
    for k in range(L):
        if M:
            unit = M * W * 8
            assert idx[k, 0] % unit == 0, (k, idx[k, 0])
            p = int(idx[k, 0]) // unit
            for m in range(M):
                v[k, 2 * m] = o.kappa[p // Nt, p % Nt, m, cols]
                v[k, 2 * m + 1] = o.kappa[(p + 1) // Nt, (p + 1) % Nt, m, cols]
            assert p // Nt == (p + 1) // Nt == L - 1 - k, (k, p, Nt)
        for cc, (tab, kind) in enumerate(tabs):
            assert idx[k, 1 + cc] % (16 * W) == 0, (k, cc)
            j = int(idx[k, 1 + cc]) // (16 * W) - poff[cc]
            assert 0 <= j <= max(len(tab) - 2, 0), (k, cc, j)
            v[k, 2 * M + 2 * cc] = tab[j, cols]
            v[k, 2 * M + 2 * cc + 1] = tab[min(j + 1, len(tab) - 1), cols]
            if kind == 0:
                allow[k, 2 * M + 2 * cc: 2 * M + 2 * cc + 2] = CIA_ALLOW * (2 if spline else 1)
        v[k, T - 1] = 1.0
    with mpmath.workdps(DPS):
        vm = mp_array(v)
        nu = mp_array(wn[cols])
        vm[:, T - 2, :] = (nu * nu * nu * nu)[None, :]
    return c, vm, allow


def extinction(c, v, allow=None, ext=None):
    """-> (e[L, ncol] mpf, de[L, ncol], A[L, ncol]): the extinction, the bound on the kernels' and the magnitude sum.
    ext: [L, ncol] doubles, layers FROM THE TOP (the caller flips the atm order), or None."""
    with mpmath.workdps(DPS):
        t = mp_array(c)[:, :, None] * v
        e = t.sum(axis=1)
        mag = np.abs(to_float(t))
        A = mag.sum(axis=1)
        n = c.shape[1] + 4
        if ext is not None:
            e = e + mp_array(ext)
            A = A + np.abs(np.asarray(ext, float))
            n += 1
        de = n * U * A
        if allow is not None:
            de = de + (allow[:, :, None] * mag).sum(axis=1)
    return e, de * SLACK, A


class Column:
    pass


def columns(e, de, A, ch: Chords, kend, toomuch, transparent, starrad, exp_rt=False):
    """The transit columns of extinctions e[L, ncol] (mpf; de, A: extinction()) over the chords `ch` -> an object
    with tau[L, ncol] (mpf; rows past kend repeat row kend), dtau[L, ncol], P[L, ncol], last[ncol], M[ncol] (mpf),
    dM[ncol], and what modulation() needs to recompute M under a mutation.  exp_rt: the bound of the matrix-tile
    kernel, whose exponential is exp_rt (the module's docstring, "transmission")."""
    out = Column()
    with mpmath.workdps(DPS):
        L, nc = e.shape
        zero = mpmath.mpf(0)
        P = np.empty((L, nc), object); P[:] = zero
        dP = np.zeros((L, nc))
        P[1:kend + 1] = e[:kend] + e[1:kend + 1]
        dP[1:kend + 1] = de[:kend] + de[1:kend + 1] + U * (A[:kend] + A[1:kend + 1])
        absP = np.abs(to_float(P))
        tau = np.empty((L, nc), object); tau[:] = zero
        dtau = np.zeros((L, nc))
        for k in range(1, kend + 1):
            d = ch.ds[k]
            tau[k] = np.dot(d[1:], P[1:k + 1])
            df = to_float(d[1:])
            nk = 16 * (k // 16 + 1) + 1
            dtau[k] = (nk * U * (df @ absP[1:k + 1]) + df @ dP[1:k + 1] + ch.dds[k][1:] @ absP[1:k + 1]) * SLACK
        tau[kend + 1:] = tau[kend]
        dtau[kend + 1:] = dtau[kend]
        tm = mpmath.mpf(float(toomuch))
        last = np.full(nc, kend, int)
        for i in range(nc):
            for k in range(1, kend + 1):
                if tau[k, i] > tm:
                    last[i] = k
                    break
        out.e, out.P, out.tau, out.dtau, out.last, out.kend, out.ch = e, P, tau, dtau, last, kend, ch
        out.toomuch, out.transparent, out.starrad, out.exp_rt = float(toomuch), bool(transparent), float(starrad), bool(exp_rt)
        res = [modulation(out, i) for i in range(nc)]
        out.M = np.array([m for m, _ in res] + [None], object)[:-1]
        out.dM = np.array([b for _, b in res])
    return out


def modulation(col, i, last=None, tau=None, core=None):
    """(M, dM) of column i; `last`, `tau` ([L] mpf) and `core` (False: the core term left out) override the
    column's own -- the mutations of the sensitivity tests."""
    with mpmath.workdps(DPS):
        r = col.ch.r
        last = int(col.last[i] if last is None else last)
        tau = col.tau[:, i] if tau is None else tau
        dtau = col.dtau[:, i]
        g = _exp(-tau[:last + 1]) * r[:last + 1]
        gf = to_float(g)
        rel = EXP_REL + (EXP_RT_FIT + EXP_RT_LN2 * (1.4427 * to_float(tau[:last + 1]) + 1.0) if col.exp_rt else 0.0)
        dg = gf * (rel + dtau[:last + 1] * (1.0 + dtau[:last + 1]) + U) + to_float(r[:last + 1]) * 1e-300
        dr = r[:last] - r[1:last + 1]
        terms = (g[:-1] + g[1:]) / 2 * dr
        integ = terms.sum() if last else mpmath.mpf(0)
        tf, drf = to_float(terms), to_float(dr)
        dinteg = ((dg[:-1] + dg[1:]) / 2 * drf).sum() + 3 * U * tf.sum() + last * U * tf.sum()
        want_core = col.transparent if core is None else core
        c = g[last] * r[last] if want_core else mpmath.mpf(0)
        R2 = mpmath.mpf(col.starrad) ** 2
        M = (r[0] * r[0] - 2 * integ - c) / R2
        big = float(r[0]) ** 2 + 2 * float(integ) + float(c)
        dM = (6 * U * big + (float(r[last]) * dg[last] if want_core else 0.0) + 2 * dinteg) / float(R2) + 3 * U * abs(float(M))
    return M, dM * SLACK


def with_exp_rt(col):
    """The same columns under the matrix-tile kernel's bound."""
    import copy
    out = copy.copy(col)
    out.exp_rt = True
    out.dM = np.array([modulation(out, i)[1] for i in range(len(col.M))])
    return out


def mutants(col, i):
    """Exact M of column i under the mistakes the GPU tests have to be able to see -> {name: M}.  (a) the cut one
    chord early / late; (b) DS(k, k) dropped from every chord; (c) the pair sum of the tile-seam layers j = 16 kt taken
    from the wrong neighbour (e_j + e_{j+1}); (d) the core term left out under `transparent`.  A mutation the
    column cannot hold (no seam inside it, the cut at the column's end) is absent."""
    out = {}
    with mpmath.workdps(DPS):
        last, kend, ch = int(col.last[i]), col.kend, col.ch
        if last - 1 >= 1:
            out["a-"] = modulation(col, i, last=last - 1)[0]
        if last + 1 <= kend:
            out["a+"] = modulation(col, i, last=last + 1)[0]
        if kend >= 1:
            t = col.tau[:, i].copy()
            for k in range(1, kend + 1):
                t[k] = t[k] - col.P[k, i] * ch.ds[k][k]
            out["b"] = modulation(col, i, tau=t, last=_cut(t, kend, col.toomuch))[0]
        seams = [j for j in range(16, kend, 16)]
        if seams:
            t = col.tau[:, i].copy()
            for j in seams:
                dp = col.e[j + 1, i] - col.e[j - 1, i]
                for k in range(j, kend + 1):
                    t[k] = t[k] + dp * ch.ds[k][j]
            out["c"] = modulation(col, i, tau=t, last=_cut(t, kend, col.toomuch))[0]
        if col.transparent:
            out["d"] = modulation(col, i, core=False)[0]
    return out


def _cut(tau, kend, toomuch):
    tm = mpmath.mpf(float(toomuch))
    for k in range(1, kend + 1):
        if tau[k] > tm:
            return k
    return kend


def undecided(col, factor=1000.0):
    """The (k, i) at or above each column's cut whose tau is within factor x its bound of toomuch -- the inputs of a
    test must leave this empty (then `last` is the same for every evaluation within the bounds)."""
    bad = []
    tm = col.toomuch
    for i in range(col.tau.shape[1]):
        for k in range(1, int(col.last[i]) + 1):
            if abs(float(col.tau[k, i]) - tm) <= factor * col.dtau[k, i]:
                bad.append((k, i))
    return bad


def absdev(got, ref):
    """|got - ref| elementwise at 50 digits -> float array."""
    with mpmath.workdps(DPS):
        return to_float(abs(mp_array(got) - np.asarray(ref, object)))
