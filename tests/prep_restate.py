"""The layer preparation (csrc/prep.hpp, prep_body) restated in mpmath at 50 digits -- TEST INFRASTRUCTURE ONLY.

It shares nothing with prep.hpp or oracle/rt_oracle.c beyond the constants' values: the hydrostatic radii follow the
reference's makeatm.radpress (code/makeatm.py:183-263: the closest layer to the reference pressure, T and mu there
by linear interpolation in log10 p, the gravity carried from layer to layer as g r^2 = const), every weight is
written from its definition.  Inputs are the doubles the engine reads (each taken exactly); nothing is rounded before
the result.  Layers are in atm order (index 0 = bottom) throughout.

Results are DENSE per temperature plane: a layer's table weight is rho (1 - f) on plane j and rho f on plane j + 1,
zeros elsewhere.  `expand_records` brings the device's records (two weights + a plane offset) to the same form, so a
temperature exactly on a node may sit as f = 1 on plane j or f = 0 on plane j + 1, and a wrong plane cannot hide.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import mpmath
import numpy as np

DPS = 50
# the constants' values (csrc/kernels.hpp; oracle/rt_oracle.h)
H, LS, KB, AMU, AMAGAT = "6.6260755e-27", "2.99792458e10", "1.380658e-16", "1.66053886e-24", "2.68679e19"
RAY_SIGMA0, RAY_LAMBDA0, POL_H2, POL_HE = "2.52e-28", "7.5e-5", "0.8059e-24", "0.2051e-24"
PI_DOUBLE = 3.141592653589793          # the engine's pi is this double (flavour 2's 128 pi^5 / 3)
DECK_BIT = 1 << 30


def _c(text):
    """A constant as the engine holds it: the double nearest to the literal."""
    return mpmath.mpf(float(text))


@dataclass
class Setup:
    """What the preparation reads besides the profile.  press: barye, atm order.  cia: one (s1, s2, temps, kind) per
    cross-section TABLE (kind 0: linear weights; 1: the temperature spline's curvature terms -- a file read under
    `cia_interp spline` gives one table of each kind)."""
    press: np.ndarray
    mass: np.ndarray
    refpress: float
    refradius: float
    gsurf: float
    tgrid: np.ndarray
    opmol: list
    cia: list = field(default_factory=list)
    scat_flag: int = 0
    scat_value: float = 0.0
    iH2: int = -1
    iHe: int = -1
    has_cloud: bool = False
    cloudtop: float = 0.0
    cloud_ext: float = 0.0
    cloud_rup: float = 0.0
    cloud_rdown: float = 0.0


def is_ok(su: Setup, prof) -> bool:
    """The rule of the `ok` flag: every layer has 0 < T < 1e30 and a mean mass above 0, in the engine's own sums (a
    NaN fails every comparison)."""
    prof = np.asarray(prof, float).reshape(len(su.mass) + 1, -1)
    for l in range(prof.shape[1]):
        T = prof[0, l]
        mu = 0.0
        for s in range(len(su.mass)):
            mu += prof[s + 1, l] * su.mass[s]
        if not (T > 0.0) or not (T < 1e30) or not (mu > 0.0):
            return False
    return True


def reference_layer(su: Setup):
    """-> (ix, exact): the layer closest to the reference pressure (first minimum of |p - p0|, np.argmin), and whether
    it holds that pressure exactly."""
    d = [abs(mpmath.mpf(float(p)) - mpmath.mpf(float(su.refpress))) for p in su.press]
    ix = min(range(len(d)), key=lambda i: (d[i], i))
    return ix, float(su.press[ix]) == float(su.refpress)


def bracket(grid, t):
    """Largest j with grid[j] <= t, clamped to [0, n - 2]."""
    j = 0
    while j < len(grid) - 2 and grid[j + 1] <= t:
        j += 1
    return j


def restate(su: Setup, prof, refradius=None, cloudtop=None, scat_value=None):
    """-> dict of object arrays of mpf (atm order): radius[L], path[L] (r[l+1] - r[l]; 0 on the top layer), c2T[L],
    rho[L][M], table_weight[L][Nt][M], cia_weight: list per table of [L][nt], cia_scale[L] (n1 n2 per table: [L][C]),
    rayleigh[L], grey[L]; and the int kstop.  The three keyword values are a walker's own overrides."""
    with mpmath.workdps(DPS):
        return _restate(su, prof, refradius, cloudtop, scat_value)


def _restate(su, prof, refradius, cloudtop, scat_value):
    mp = mpmath.mpf
    S = len(su.mass)
    prof = np.asarray(prof, float).reshape(S + 1, -1)
    L = prof.shape[1]
    P = [mp(float(p)) for p in su.press]
    T = [mp(float(t)) for t in prof[0]]
    q = [[mp(float(prof[s + 1, l])) for l in range(L)] for s in range(S)]
    mass = [mp(float(m)) for m in su.mass]
    mu = [sum(q[s][l] * mass[s] for s in range(S)) for l in range(L)]
    kb, amu, amagat = _c(KB), _c(AMU), _c(AMAGAT)
    rgas = kb / amu
    R0 = mp(float(su.refradius if refradius is None else refradius))
    g0, p0 = mp(float(su.gsurf)), mp(float(su.refpress))

    # ---- radii, makeatm.py:229-258
    ix, exact = reference_layer(su)
    rad, g = [None] * L, [None] * L
    if exact:
        rad[ix], g[ix] = R0, g0
    else:
        # T and mu at p0: linear in log10 p between the two layers around it (makeatm.py:212-218); outside the
        # grid no pair of layers holds p0 and the closest layer's own values stand
        t0, m0 = T[ix], mu[ix]
        for i in range(L - 1):
            lo, hi = min(P[i], P[i + 1]), max(P[i], P[i + 1])
            if lo <= p0 <= hi:
                f = (mpmath.log10(p0) - mpmath.log10(P[i])) / (mpmath.log10(P[i + 1]) - mpmath.log10(P[i]))
                t0, m0 = T[i] + f * (T[i + 1] - T[i]), mu[i] + f * (mu[i + 1] - mu[i])
                break
        if P[ix] > p0:
            rad[ix] = R0 + (T[ix] / mu[ix] + t0 / m0) / 2 * (rgas * mpmath.log(p0 / P[ix]) / g0)
        else:
            rad[ix] = R0 - (T[ix] / mu[ix] + t0 / m0) / 2 * (rgas * mpmath.log(P[ix] / p0) / g0)
        g[ix] = g0 * R0 ** 2 / rad[ix] ** 2
    for i in range(ix - 1, -1, -1):
        rad[i] = rad[i + 1] - (T[i] / mu[i] + T[i + 1] / mu[i + 1]) / 2 * (rgas * mpmath.log(P[i] / P[i + 1]) / g[i + 1])
        g[i] = g[i + 1] * rad[i + 1] ** 2 / rad[i] ** 2
    for i in range(ix + 1, L):
        rad[i] = rad[i - 1] + (T[i] / mu[i] + T[i - 1] / mu[i - 1]) / 2 * (rgas * mpmath.log(P[i - 1] / P[i]) / g[i - 1])
        g[i] = g[i - 1] * rad[i - 1] ** 2 / rad[i] ** 2
    path = [rad[l + 1] - rad[l] if l + 1 < L else mp(0) for l in range(L)]

    # ---- per-layer terms
    c2 = _c(H) * _c(LS) / kb
    nd = [P[l] / (kb * T[l]) for l in range(L)]
    tg = [mp(float(t)) for t in su.tgrid]
    Nt, M = len(tg), len(su.opmol)
    rho = np.empty((L, max(M, 1)), object)
    tw = np.empty((L, Nt, max(M, 1)), object)
    tw.fill(mp(0))
    for l in range(L):
        if M == 0:
            rho[l, 0] = mp(0)
            continue
        j = bracket(tg, T[l])
        f = (T[l] - tg[j]) / (tg[j + 1] - tg[j])
        for m, s in enumerate(su.opmol):
            rho[l, m] = q[s][l] * mass[s] * amu * nd[l]
            tw[l, j, m] = rho[l, m] * (1 - f)
            tw[l, j + 1, m] = rho[l, m] * f
    cw, cs = [], np.empty((L, max(len(su.cia), 1)), object)
    for cc, (s1, s2, temps, kind) in enumerate(su.cia):
        ct = [mp(float(t)) for t in temps]
        nt = len(ct)
        w = np.empty((L, nt), object)
        w.fill(mp(0))
        for l in range(L):
            Tc = min(max(T[l], ct[0]), ct[-1])
            nn = (q[s1][l] * nd[l] / amagat) * (q[s2][l] * nd[l] / amagat)
            cs[l, cc] = nn
            if nt == 1:
                w[l, 0] = nn if kind == 0 else mp(0)
                continue
            j = bracket(ct, Tc)
            h = ct[j + 1] - ct[j]
            f = (Tc - ct[j]) / h
            if kind == 0:
                w[l, j], w[l, j + 1] = nn * (1 - f), nn * f
            else:
                a = 1 - f
                w[l, j], w[l, j + 1] = nn * (a ** 3 - a) * h * h / 6, nn * (f ** 3 - f) * h * h / 6
        cw.append(w)
    sv = mp(float(su.scat_value if scat_value is None else scat_value))
    ray = [mp(0)] * L
    if su.scat_flag == 1 and su.iH2 >= 0:
        ray = [mp(10) ** sv * _c(RAY_SIGMA0) * q[su.iH2][l] * nd[l] * _c(RAY_LAMBDA0) ** 4 for l in range(L)]
    elif su.scat_flag == 2:
        k0 = 128 * mp(PI_DOUBLE) ** 5 / 3
        ray = [k0 * ((_c(POL_H2) ** 2 * q[su.iH2][l] * nd[l] if su.iH2 >= 0 else 0)
                     + (_c(POL_HE) ** 2 * q[su.iHe][l] * nd[l] if su.iHe >= 0 else 0)) for l in range(L)]
    grey = [mp(0)] * L
    if su.cloud_ext > 0.0:
        up, down, ext = mp(float(su.cloud_rup)), mp(float(su.cloud_rdown)), mp(float(su.cloud_ext))
        grey = [mp(0) if rad[l] >= up else (ext if rad[l] <= down else ext * (up - rad[l]) / (up - down))
                for l in range(L)]
    # ---- the column's last layer, counted from the top: the first layer at or below the cloud top
    kstop = L - 1
    has_cloud = su.has_cloud or cloudtop is not None
    if has_cloud:
        ctop = float(su.cloudtop if cloudtop is None else cloudtop)
        for k in range(L):
            if float(su.press[L - 1 - k]) >= ctop:
                kstop = k | DECK_BIT
                break
    arr = lambda v: np.array(list(v) + [None], object)[:-1]
    return dict(radius=arr(rad), path=arr(path), c2T=arr([c2 / T[l] for l in range(L)]), rho=rho, table_weight=tw,
                cia_weight=cw, cia_scale=cs, rayleigh=arr(ray), grey=arr(grey), kstop=kstop, ref_idx=ix,
                ref_exact=exact)


def expand_records(su: Setup, coef, idx, W):
    """The device's records of one walker (layers from the top) in the restatement's dense form and atm order:
    dict of float arrays path[L], c2T[L], table_weight[L][Nt][M], cia_weight (list of [L][nt]), rayleigh[L],
    grey[L].  The plane is recovered from `idx`; a plane outside the table is an AssertionError."""
    coef, idx = np.asarray(coef, float), np.asarray(idx)
    L, Nt, M, Cn = coef.shape[0], len(su.tgrid), len(su.opmol), len(su.cia)
    assert coef.shape[1] == 4 + 2 * M + 2 * Cn and idx.shape == (L, 1 + Cn)
    out = dict(path=np.zeros(L), c2T=np.zeros(L), table_weight=np.zeros((L, Nt, max(M, 1))),
               cia_weight=[np.zeros((L, len(t[2]))) for t in su.cia], rayleigh=np.zeros(L), grey=np.zeros(L))
    poff = np.concatenate([[0], np.cumsum([max(len(t[2]) - 1, 1) for t in su.cia])]).astype(int)
    for k in range(L):
        l = L - 1 - k
        c = coef[k]
        out["path"][l], out["c2T"][l] = c[0], c[1]
        if M:
            unit = M * W * 8
            assert idx[k, 0] % unit == 0, (k, idx[k, 0])
            j = int(idx[k, 0]) // unit - l * Nt
            assert 0 <= j <= Nt - 2, (k, j)
            for m in range(M):
                out["table_weight"][l, j, m] += c[2 + 2 * m]
                out["table_weight"][l, j + 1, m] += c[3 + 2 * m]
        for cc in range(Cn):
            nt = len(su.cia[cc][2])
            assert idx[k, 1 + cc] % (W * 16) == 0, (k, cc, idx[k, 1 + cc])
            j = int(idx[k, 1 + cc]) // (W * 16) - poff[cc]
            assert 0 <= j <= max(nt - 2, 0), (k, cc, j)
            # (a single-temperature table: one pair plane holding its values twice)
            out["cia_weight"][cc][l, j] += c[2 + 2 * M + 2 * cc]
            out["cia_weight"][cc][l, min(j + 1, nt - 1)] += c[3 + 2 * M + 2 * cc]
        out["rayleigh"][l], out["grey"][l] = c[2 + 2 * M + 2 * Cn], c[3 + 2 * M + 2 * Cn]
    return out


def absdev(got, ref):
    """|got - ref| elementwise, the difference taken at 50 digits -> float array."""
    got, ref = np.asarray(got, float), np.asarray(ref, object)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    out = np.zeros(got.shape)
    with mpmath.workdps(DPS):
        for i in np.ndindex(*got.shape):
            out[i] = float(abs(mpmath.mpf(float(got[i])) - ref[i]))
    return out


def mag(ref):
    """|ref| as floats."""
    ref = np.asarray(ref, object)
    out = np.zeros(ref.shape)
    for i in np.ndindex(*ref.shape):
        out[i] = abs(float(ref[i]))
    return out


def ulp(x):
    """The spacing of doubles at |x| (array)."""
    return np.spacing(np.abs(np.asarray(x, float)))


def setup_from_oracle(o, cia_kinds=None, **kw) -> Setup:
    """A Setup from an oracle.rt_oracle.OracleEngine (its own readers of the same files): `cia_kinds` is the kinds of
    the engine's cross-section tables in order -- default one linear table per file, plus one curvature table per
    file when the oracle holds spline planes."""
    c = o.c
    files, off = [], 0
    for k in range(len(o.cia_nt) if c.ncia else 0):
        nt = int(o.cia_nt[k])
        files.append((int(o.cia_s1[k]), int(o.cia_s2[k]), np.array(o.cia_temp[off:off + nt])))
        off += nt
    cia = []
    for s1, s2, t in files:
        cia.append((s1, s2, t, 0))
        if c.cia_spline:
            cia.append((s1, s2, t, 1))
    su = Setup(press=np.array(o.press), mass=np.array(o.mass), refpress=c.refpress, refradius=c.refradius,
               gsurf=c.gsurf, tgrid=np.array(o.tgrid), opmol=[int(x) for x in o.opmol], cia=cia,
               scat_flag=c.scat_flag, scat_value=c.scat_value, iH2=c.scat_iH2, iHe=c.scat_iHe,
               has_cloud=bool(c.has_cloud), cloudtop=c.cloudtop, cloud_ext=c.cloud_ext, cloud_rup=c.cloud_rup,
               cloud_rdown=c.cloud_rdown)
    for k, v in kw.items():
        setattr(su, k, v)
    return su
