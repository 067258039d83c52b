"""The line-by-line kernels' Voigt function (csrc/lbl.hip voigt_k / voigt_far, through engine.voigt) at its seams,
against mpmath's w(z) = exp(-z^2) erfc(-i z) at 34 digits.

Every point is held to the claim lbl.hip documents for the branch it falls in plus that branch's counted roundings
(lbl_restate.eps_k: CLAIM, round_of -- the arguments are the doubles themselves here, so nothing else enters); beyond
|z| = 8 with y < 1 the series drop the exp(-z^2) term, so an absolute exp(-x^2) is allowed on top (at most 1 x
(exp(-x^2) + y / (sqrt(pi) x^2)), the two leading terms of K there; the second one is held relatively).  No other
number: scipy and the 1e-7 of the oracle comparison do not appear.

  table seams   x = k / 16 (k = 0 .. 128: the pieces of the Im w table, imw_row's local coordinate +-1/2) with both
                neighbours, and the mid-piece points, crossed with y on both sides of every step of voigt_order; the two
                sides of a seam differ by at most the two claims (and K_x times the two ulps between them)
  circles       r^2 = 64, 289, 1e4 at 16 angles from y = 1e-9 r to the y axis, the two neighbouring doubles between which
                x * x + y * y (rounded as the kernel rounds it) crosses; x just below 8 with r^2 >= 64 among them
  y = 0.13      across |z| < 8 on both sides: the hand-over from the expansion about the real axis to Weideman
  y -> 0        y = 0 and 1e-300 .. 1e-12: relative inside |z| = 8, exp(-x^2) beyond
  large y       1e4 .. 1e8 (a 100 bar layer)

The neighbours of a seam are one ulp from it: their reference is K + K_x ulp, from the derivative w' = -2 z w + 2 i /
sqrt(pi) that comes with the value (the next term is below 1e-30).

Measured on an MI355X (worst error / tolerance): Taylor 0.926, eleven-term series 0.978, six-term series 0.972 of the
corrected 3.8e-12 (3.7e-12 at x = 17, y -> 0; lbl.hip said 3e-13), Weideman 0.085, voigt_far 0.938 (MEASUREMENTS.md, row 31).
Pytest durations on an MI355X: 1.6 s for the module; the seams 0.9 s, the mid-piece points 0.5 s, the others below 0.1 s."""
import math

import numpy as np
import pytest

import lbl_restate as X

pytestmark = pytest.mark.gpu

STEPS = list(X.ORDER_STEPS) + [X.TAYLOR_YMAX]
Y_SIDES = [v for s in STEPS for v in (s, float(np.nextafter(s, 1.0)))]
_fad = X.Faddeeva()
_worst = {}


def _tol(x, y, K):
    r2 = x * x + y * y
    # (math.exp of the rounded square: 2 x^2 u of its own)
    floor = math.exp(-x * x) * (1 + (2 * x * x + 4) * X.U) if (r2 >= 64.0 * (1 - X.SEAM) and y < 1.0) else 0.0
    return X.eps_k(x, y) * K + floor


def _hold(x, y, ref, what):
    """engine.voigt on the doubles (x, y) against ref (floats of the exact values); prints the worst error / tolerance
    per branch, then asserts."""
    from bart_amd import engine
    x, y, ref = np.asarray(x, float), np.asarray(y, float), np.asarray(ref, float)
    got = engine.voigt(x, y)
    assert got.shape == x.shape and np.all(np.isfinite(got)) and np.all(got >= 0)
    tol = np.array([_tol(a, b, k) for a, b, k in zip(x, y, ref)])
    err = np.abs(got - ref)
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    br = np.array([X.branch_of(a, b) for a, b in zip(x, y)])
    for b in np.unique(br):
        m = br == b
        i = np.argmax(np.where(m, ratio, -1))
        rel = np.abs(got[m] / ref[m] - 1).max() if (ref[m] > 0).all() else float("nan")
        _worst[(what, b)] = float(ratio[i])
        print("%s %-8s %5d points, worst error / tolerance %.3f at x = %r, y = %r; worst relative error %.3g"
              % (what, b, m.sum(), ratio[i], x[i], y[i], rel))
    bad = ratio > 1
    assert not bad.any(), (what, list(zip(x[bad][:5], y[bad][:5], ratio[bad][:5], br[bad][:5])))
    return got


def _exact(x, y):
    K, Kx, _ = _fad(X.mpf(float(x)), X.mpf(float(y)))
    return K, Kx


def test_table_seams_both_sides_of_every_order_step():
    xs, ys, ref, seam = [], [], [], []
    for k in range(129):
        x0 = k / 16.0
        for y in Y_SIDES:
            K, Kx = _exact(x0, y)
            for xn in ([x0] if k == 0 else [float(np.nextafter(x0, 0.0)), x0]) + [float(np.nextafter(x0, 9.0))]:
                xs.append(xn); ys.append(y); ref.append(float(K + Kx * (X.mpf(xn) - X.mpf(x0))))
            if k:
                seam.append((len(xs) - 3, len(xs) - 2, float(abs(Kx))))
    got = _hold(xs, ys, ref, "seams")
    xs, ys, ref = np.array(xs), np.array(ys), np.array(ref)
    # the value just below a seam (the lower piece at t = +1/2) against the value on it (the upper piece at t = -1/2)
    for a, b, dk in seam:
        allowed = (X.eps_k(xs[a], ys[a]) + X.eps_k(xs[b], ys[b])) * ref[b] + dk * (xs[b] - xs[a]) + math.exp(-xs[b] ** 2) * (xs[b] >= 8)
        assert abs(got[a] - got[b]) <= allowed, (xs[a], xs[b], ys[a], got[a], got[b], allowed)


def test_mid_piece_points():
    xs, ys, ref = [], [], []
    for k in range(128):
        for y in Y_SIDES:
            xs.append((k + 0.5) / 16.0); ys.append(y); ref.append(float(_exact(xs[-1], y)[0]))
    _hold(xs, ys, ref, "mid-piece")


def _r2(x, y):
    return x * x + y * y          # (each product and the sum rounded, as voigt_k forms it without contraction)


def _straddle(x, y, R2, move_x):
    """The two neighbouring doubles (of x, or of y when x = 0) between which _r2 crosses R2: ((x, y) below, (x, y) at or
    above), by bisection on the doubles."""
    f = (lambda v: _r2(v, y)) if move_x else (lambda v: _r2(x, v))
    v = x if move_x else y
    lo, hi = v * (1 - 1e-6), v * (1 + 1e-6)
    assert f(lo) < R2 <= f(hi)
    while np.nextafter(lo, np.inf) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) < R2 else (lo, mid)
    return ((lo, y), (hi, y)) if move_x else ((x, lo), (x, hi))


def test_circles_both_sides():
    fr = [1e-9, 1e-7, 1e-5, 1e-3, 1e-2, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.8, 0.9, 0.97, 0.999, 1.0]
    xs, ys, ref = [], [], []
    below8 = 0
    for R2 in (64.0, 289.0, 1.0e4):
        r = math.sqrt(R2)
        for s in fr:
            y = r * s
            x = 0.0 if s == 1.0 else r * math.sqrt((1 - s) * (1 + s))
            for (a, b) in _straddle(x, y, R2, move_x=s < 0.9):
                xs.append(a); ys.append(b); ref.append(float(_exact(a, b)[0]))
            assert _r2(xs[-2], ys[-2]) < R2 <= _r2(xs[-1], ys[-1])
            below8 += R2 == 64.0 and xs[-1] < 8.0 and ys[-1] <= X.TAYLOR_YMAX
    # x just below 8 with r^2 >= 64 and a small y: routed away from the expansion about the real axis
    assert below8 >= 3
    for y in (1e-2, 0.13):
        x = float(np.nextafter(8.0, 0.0))
        assert _r2(x, y) >= 64.0 and X.branch_of(x, y) == "asym11"
        xs.append(x); ys.append(y); ref.append(float(_exact(x, y)[0]))
    _hold(xs, ys, ref, "circles")


def test_the_line_y_013():
    xs = list(np.linspace(0.0, 7.99, 160))
    pts = [(x, y) for x in xs for y in (X.TAYLOR_YMAX, float(np.nextafter(X.TAYLOR_YMAX, 1.0)))]
    assert {X.branch_of(*p) for p in pts} == {"taylor", "weideman"}
    _hold([p[0] for p in pts], [p[1] for p in pts], [float(_exact(*p)[0]) for p in pts], "y=0.13")


def test_y_zero_and_very_small_y():
    """y = 0 is reachable (no H2 and no He among the species: aL = 0).  Inside |z| = 8 the expansion is held to its
    relative claim; beyond, the series return y / (sqrt(pi) x^2) (1 + ...) -- exactly 0 at y = 0 -- where K = exp(-x^2)
    + that: held to exp(-x^2) absolutely plus the claim on the rest."""
    from bart_amd import engine
    xs = [0.0, 0.1, 1.0, 3.0, 5.0, 7.0, 7.99, 8.0, 8.5, 10.0, 16.9, 17.0, 20.0, 26.0, 50.0, 99.9, 100.0]
    ys = [0.0, 1e-300, 1e-200, 1e-100, 1e-50, 1e-30, 1e-20, 1e-15, 1e-12]
    pts = [(x, y) for x in xs for y in ys]
    _hold([p[0] for p in pts], [p[1] for p in pts], [float(_exact(*p)[0]) for p in pts], "y->0")
    far = np.array([x for x in xs if x >= 8.0])
    assert np.array_equal(engine.voigt(far, np.zeros(far.size)), np.zeros(far.size))     # (ti = 0, so si = 0)
    near = np.array([x for x in xs if x < 8.0])
    k0 = engine.voigt(near, np.zeros(near.size))
    assert np.all(np.abs(k0 / np.exp(-near * near) - 1) <= X.CLAIM["taylor"] + X.round_of("taylor", 8.0, 0.0))


def test_large_y():
    pts = [(x, y) for y in (1e4, 1e5, 1e6, 1e7, 1e8) for x in (0.0, 1.0, 100.0, 1e3, 1e4, 1e5, 1e6)]
    assert {X.branch_of(*p) for p in pts} == {"far"}
    _hold([p[0] for p in pts], [p[1] for p in pts], [float(_exact(*p)[0]) for p in pts], "large y")
