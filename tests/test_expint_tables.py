"""CPU: the Chebyshev tables of csrc/expint_coef.hpp and the row selection of csrc/step.hip's expint_e2, restated
with mpmath at 50 digits and held to the source's own claim against mpmath.expint(2, x): 6e-16 for x <= 1, 4e-16 above.

The header is read as data (numbers only).  The restatement evaluates the two forms exactly, so what it measures is
the tables' approximation error and the choice of row on either side of every half-octave boundary; the fp64 rounding
of the device's own evaluation comes on top of it and is held on the GPU (tests/test_gpu_step_edges.py), on the same
points (e2_points)."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bart_amd", "csrc", "expint_coef.hpp")
CUTOFF = 709.78271289338397        # expint_e2 returns 0.0 above it (step.hip)
SQRT_HALF = 0.70710678118654757    # the mantissa at which a half octave begins (step.hip)


def boundary(j):
    """The double nearest 2^(j/2)."""
    import mpmath
    with mpmath.workdps(50):
        return float(mpmath.mpf(2) ** (mpmath.mpf(j) / 2))


def e2_points():
    """The arguments both halves evaluate: the zero, subnormal and tiny ones, negative powers of two, either side
    of x = 1 (where the two forms meet) and of every half-octave boundary 2^(j/2) (where the table row changes), a
    seeded log-uniform sweep, and the cut-off with what lies beyond it."""
    pts = [0.0, 5e-324, 1e-300] + [2.0 ** -k for k in range(1, 61)]
    pts += [np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)]
    for j in range(20):
        b = boundary(j)
        pts += [np.nextafter(b, 0.0), b, np.nextafter(b, np.inf)]
    rng = np.random.default_rng(20261017)
    pts += list(np.exp(rng.uniform(np.log(1e-12), np.log(709.78), 4096)))
    pts += [CUTOFF, np.nextafter(CUTOFF, np.inf), 745.0, 1e308, np.inf, np.nan]
    return np.array(pts, np.float64)


def read_tables():
    """-> (small[13], large[20][19]) from the header's brace blocks; the declared sizes are checked."""
    text = re.sub(r"//[^\n]*", "", open(HEADER).read())
    size = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", text)}
    num = r"[-+]?\d+\.\d+e[-+]\d+"
    small = re.search(r"kE2Small\[kE2SmallTerms\] = \{([^}]*)\}", text).group(1)
    small = [float(v) for v in re.findall(num, small)]
    body = text[text.index("kE2Large[kE2LargeIntervals]"):]
    large = [[float(v) for v in re.findall(num, row)] for row in re.findall(r"\{([^{}]*)\}", body)]
    assert len(small) == size["kE2SmallTerms"] == 13
    assert len(large) == size["kE2LargeIntervals"] == 20
    assert all(len(r) == 2 + size["kE2LargeTerms"] == 19 for r in large)
    return small, large


def clenshaw(mp, c, t):
    b1 = b2 = mp.mpf(0)
    for k in range(len(c) - 1, 0, -1):
        b1, b2 = 2 * t * b1 + mp.mpf(c[k]) - b2, b1
    return t * b1 + mp.mpf(c[0]) - b2


def row_of(x):
    """The table row expint_e2 picks for x > 1: frexp and the comparison with sqrt(1/2), clamped to the last row."""
    m, e = math.frexp(x)
    return min(2 * (e - 1) + (1 if m >= SQRT_HALF else 0), 19)


def restated(mp, x, small, large):
    """expint_e2 in exact arithmetic on the double x (finite)."""
    if x > CUTOFF:
        return mp.mpf(0)
    if x == 0.0:
        return mp.mpf(1)
    X = mp.mpf(x)
    if x <= 1.0:
        return X * mp.log(X) + clenshaw(mp, small, 2 * X - 1)
    row = large[row_of(x)]
    return mp.exp(-X) * clenshaw(mp, row[2:], X * mp.mpf(row[0]) + mp.mpf(row[1]))


def test_row_selection_at_the_half_octave_boundaries():
    """The double nearest 2^(j/2) opens row j, its predecessor closes row j - 1, and each row's own map sends its
    interval onto [-1, 1] (a row off by one puts t outside it)."""
    _, large = read_tables()
    for j in range(20):
        b = boundary(j)
        if j:   # (x = 1 itself takes the other form)
            assert row_of(b) == j, (j, b)
            assert row_of(np.nextafter(b, 0.0)) == j - 1, (j, b)
        assert row_of(np.nextafter(b, np.inf)) == j, (j, b)
        lo, hi = 2.0 ** (j / 2), 2.0 ** ((j + 1) / 2)
        assert abs(lo * large[j][0] + large[j][1] + 1.0) < 1e-12 and abs(hi * large[j][0] + large[j][1] - 1.0) < 1e-12, j
    assert row_of(CUTOFF) == 18         # 512 <= x < 724.1: the last row but one is the last one used


def test_tables_against_mpmath_expint():
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    small, large = read_tables()
    x = e2_points()
    worst = {"small": (0.0, None), "large": (0.0, None)}
    for v in x[np.isfinite(x)]:
        v = float(v)
        got = restated(mp, v, small, large)
        if v > CUTOFF:
            # beyond the cut-off the function returns 0.0; the exact value there is below the smallest normal number
            assert got == 0 and mp.expint(2, mp.mpf(v)) < mp.mpf(2) ** -1022
            continue
        ref = mp.expint(2, mp.mpf(v)) if v > 0.0 else mp.mpf(1)
        err = float(abs(got / ref - 1))
        key = "small" if v <= 1.0 else "large"
        if err > worst[key][0]:
            worst[key] = (err, v)
    print("worst relative error of the exact restatement: x <= 1 %.3g at %r, x > 1 %.3g at %r"
          % (worst["small"] + worst["large"]))
    assert worst["small"][0] <= 6e-16, worst
    assert worst["large"][0] <= 4e-16, worst
    # x = 0 is a branch of its own; the table's value there is what the limit x -> 0 meets
    assert abs(clenshaw(mp, small, mp.mpf(-1)) - 1) <= 6e-16
