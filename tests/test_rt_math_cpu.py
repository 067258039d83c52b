"""CPU: the claims the comments of csrc/kernels.hpp and csrc/lbl.hip make about exp_rt, exp_core and exp_rt_fma3, held
against mpmath.exp at 50 digits through the exact restatement of tests/rtmath_restate.py.

The bounds are the header's figures with their last digit rounded up:

  exp_rt, interpolant on [-ln2/2, ln2/2] ... 7.5e-14 in the value, 1.45e-11 in the derivative (header: 7e-14, 1.4e-11)
  exp_rt, whole range ...................... 7.5e-14 + 2.4e-17 |n|               (header: 2.3e-17 per unit of n)
  exp_rt, expm1-relative at n = 0 .......... 2.0e-13: (p(r) - 1) / (e^r - 1) - 1, what the exact 1 + r terms buy
  exp_core, interpolant .................... 1.7e-17
  exp_core, whole range .................... 1.7e-17 + |n| |hi + lo - ln2|, the last factor from the constants

Figures are printed before they are asserted (run with -s).  The fp64 rounding of the device's own evaluation is
held on the GPU (tests/test_gpu_rt_math.py)."""
import math
import struct

import numpy as np

import rtmath_restate as rs

GRID = 8001


def _grid():
    return np.linspace(-rs.LN2 / 2, rs.LN2 / 2, GRID)


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _value_errors(mp, coef):
    """max over the grid of |p(r) / e^r - 1| -> (error, r)."""
    worst = (0.0, None)
    for r in _grid():
        R = mp.mpf(float(r))
        e = float(abs(rs.horner(mp, coef, R) / mp.exp(R) - 1))
        if e > worst[0]:
            worst = (e, float(r))
    return worst


def _expm1_errors(mp, coef, points):
    """max over the points (r != 0) of |(p(r) - 1) / (e^r - 1) - 1| -> (error, r)."""
    worst = (0.0, None)
    for r in points:
        if r == 0.0:
            continue
        R = mp.mpf(float(r))
        e = float(abs((rs.horner(mp, coef, R) - 1) / mp.expm1(R) - 1))
        if e > worst[0]:
            worst = (e, float(r))
    return worst


def test_constants_read_from_the_sources():
    k, l = rs.read_kernels_hpp(), rs.read_lbl_hip()
    # the two exp_rt tables are identical doubles, and so are the constants around them
    assert [_bits(a) for a in k["rt"]] == [_bits(b) for b in l["rt"]]
    assert _bits(k["log2e"]) == _bits(l["log2e"]) and _bits(k["ln2"]) == _bits(l["ln2"])
    # constant and linear coefficients of both interpolants: exactly 1
    assert k["rt"][-2:] == [1.0, 1.0] and k["core"][-2:] == [1.0, 1.0]
    # the constants are the doubles nearest what they stand for
    mp = rs.mp50()
    assert k["log2e"] == float(1 / mp.log(2)) and k["ln2"] == float(mp.log(2)) == rs.LN2
    assert k["shift"] == 1.5 * 2.0 ** 52
    # ln2_hi ends in at least 11 zero bits: n * ln2_hi is exact for |n| <= 1022 < 2^10 (and then some)
    m = _bits(k["ln2_hi"]) & ((1 << 52) - 1)
    trailing = (m & -m).bit_length() - 1
    print("ln2_hi: %d trailing zero mantissa bits; hi + lo - ln2 = %.3g" %
          (trailing, float(mp.mpf(k["ln2_hi"]) + mp.mpf(k["ln2_lo"]) - mp.log(2))))
    assert trailing >= 11
    assert abs(k["ln2_lo"]) < 2.0 ** -31         # lo is what hi leaves, not a second copy
    # the range ends give the n the exponent field must hold: -1021 .. 1010 (exp_rt), 1023 at exp_core's end
    assert rs.n_of(rs.X_MIN, k["log2e"]) == -1021 and rs.n_of(rs.X_MAX_RT, k["log2e"]) == 1010
    assert rs.n_of(rs.X_MAX_CORE, k["log2e"]) == 1023


def test_n_is_the_shifters_integer():
    """n_of against the fp64 sequence itself where numpy can state it: fma(x, log2e, shift) - shift differs from
    (x * log2e + shift) - shift only when the product's own rounding crosses a tie, which the exact rule decides; on
    the points the two agree but for such crossings, and the exact rule is within 1/2 of the exact product always."""
    from fractions import Fraction
    k = rs.read_kernels_hpp()
    x = rs.rt_points()
    two_step = (x * k["log2e"] + k["shift"]) - k["shift"]
    differ = 0
    for v, t in zip(x, two_step):
        n = rs.n_of(float(v), k["log2e"])
        exact = Fraction(float(v)) * Fraction(k["log2e"])
        assert abs(exact - n) <= Fraction(1, 2)
        if n != int(t):
            # only where the product lies within its own rounding (2^-43 at most, below 2^10) of a tie
            differ += 1
            assert abs(abs(exact - n) - Fraction(1, 2)) < Fraction(1, 2 ** 42), v
    print("n: exact rule and two-step fp64 differ on %d of %d points, all of them at a tie" % (differ, x.size))
    # where n steps: the point below (k + 1/2) ln2 and the point above it take n = k and k + 1
    steps = np.array(rs.half_ln2_steps())
    ns = [rs.n_of(float(v), k["log2e"]) for v in steps]
    assert len(steps) > 3 * 2000 and all(b - a in (0, 1) for a, b in zip(ns, ns[1:]))
    assert min(ns) == -1021 and max(ns) == 1023


def test_exp_rt_interpolant_value_and_derivative():
    mp, k = rs.mp50(), rs.read_kernels_hpp()
    wv, wd = (0.0, None), (0.0, None)
    for r in _grid():
        R = mp.mpf(float(r))
        e = mp.exp(R)
        ev = float(abs(rs.horner(mp, k["rt"], R) / e - 1))
        ed = float(abs(rs.horner_deriv(mp, k["rt"], R) / e - 1))
        if ev > wv[0]:
            wv = (ev, float(r))
        if ed > wd[0]:
            wd = (ed, float(r))
    print("exp_rt interpolant: value %.4g at r = %r, derivative %.4g at r = %r" % (wv + wd))
    assert wv[0] <= 7.5e-14, wv
    assert wd[0] <= 1.45e-11, wd


def test_exp_rt_on_the_whole_range():
    mp = rs.mp50()
    x, vals = rs.restated_on_points("exp_rt")
    worst, worst_excess = (0.0, None, 0), -1.0
    for v, (got, n) in zip(x, vals):
        err = float(abs(got / mp.exp(mp.mpf(float(v))) - 1))
        bound = 7.5e-14 + 2.4e-17 * abs(n)
        worst_excess = max(worst_excess, err / bound)
        if err > worst[0]:
            worst = (err, float(v), n)
    print("exp_rt restated, %d points: worst %.4g at x = %r (n = %d); largest error / bound %.3f"
          % ((x.size,) + worst + (worst_excess,)))
    assert worst_excess <= 1.0, worst


def test_exp_rt_expm1_relative_at_n0():
    """exp(x) - 1 for x < ln2/2 -- the Planck denominator of a hot, far-infrared column; differences of
    transmittances of thin layers see the same thing -- lives on the interpolant's exact 1 + r."""
    mp, k = rs.mp50(), rs.read_kernels_hpp()
    worst = _expm1_errors(mp, k["rt"], _grid())
    print("exp_rt (p(r) - 1) / (e^r - 1) - 1 on the n = 0 grid: %.4g at r = %r" % worst)
    assert worst[0] <= 2.0e-13, worst
    # and on the range points that reduce with n = 0: down to |r| = 1e-12 the bound holds as it stands
    x = rs.rt_points()
    small = [float(v) for v in x if 1e-12 <= abs(v) < rs.LN2 / 2]
    worst = _expm1_errors(mp, k["rt"], small)
    print("... on the %d range points with 1e-12 <= |x| < ln2/2: %.4g at x = %r" % ((len(small),) + worst))
    assert worst[0] <= 2.0e-13, worst


def test_exp_core_interpolant_and_range():
    mp, k = rs.mp50(), rs.read_kernels_hpp()
    worst = _value_errors(mp, k["core"])
    print("exp_core interpolant: %.4g at r = %r" % worst)
    assert worst[0] <= 1.7e-17, worst
    dln2 = float(abs(mp.mpf(k["ln2_hi"]) + mp.mpf(k["ln2_lo"]) - mp.log(2)))
    x, vals = rs.restated_on_points("exp_core")
    worst, worst_excess = (0.0, None, 0), -1.0
    for v, (got, n) in zip(x, vals):
        err = float(abs(got / mp.exp(mp.mpf(float(v))) - 1))
        worst_excess = max(worst_excess, err / (1.7e-17 + abs(n) * dln2))
        if err > worst[0]:
            worst = (err, float(v), n)
    print("exp_core restated, %d points: worst %.4g at x = %r (n = %d); |hi + lo - ln2| = %.3g; largest error / bound "
          "%.3f" % ((x.size,) + worst + (dln2, worst_excess)))
    assert worst_excess <= 1.0, worst


def test_mutation_an_unconstrained_constant_or_linear_term_is_caught():
    """What the exact 1 + r buys, stated as a failure of the expm1-relative bound near r = 2^-20.  One ulp on the
    CONSTANT coefficient is an absolute 2.2e-16 under e^r - 1 = 9.5e-7: 2.3e-10.  One ulp on the LINEAR coefficient is
    2.2e-16 relative to e^r - 1 at every r and cannot reach 2e-13 anywhere (printed); an unconstrained fit's linear term
    is off by the fit's own error, 1e-12 for the degree-8 one the header mentions, and that is caught."""
    mp, k = rs.mp50(), rs.read_kernels_hpp()
    near = [2.0 ** -20 * f for f in (0.5, 0.75, 1.0, 1.5, 2.0)] + [-(2.0 ** -20)]
    assert _expm1_errors(mp, k["rt"], near)[0] <= 2.0e-13
    for up in (True, False):
        c = list(k["rt"])
        c[-1] = float(np.nextafter(1.0, 2.0 if up else 0.0))
        e = _expm1_errors(mp, c, near)
        print("constant coefficient one ulp %s: %.4g at r = %r" % (("up" if up else "down",) + e))
        assert e[0] > 2.0e-13 and e[0] > 1e-10
        c = list(k["rt"])
        c[-2] = float(np.nextafter(1.0, 2.0 if up else 0.0))
        print("linear coefficient one ulp %s: %.4g at r = %r" % (("up" if up else "down",) + _expm1_errors(mp, c, near)))
        c[-2] = 1.0 + (1e-12 if up else -1e-12)
        e = _expm1_errors(mp, c, near)
        print("linear coefficient off by 1e-12 %s: %.4g at r = %r" % (("up" if up else "down",) + e))
        assert e[0] > 2.0e-13


def mutate_digit(v, digit, step):
    """v with its `digit`-th significant decimal digit moved by `step` (one unit of that digit's place)."""
    exp10 = math.floor(math.log10(abs(v)))
    return v + step * 10.0 ** (exp10 - digit + 1)


def test_mutation_a_coefficient_wrong_in_its_12th_digit_is_caught():
    """The sixth entry of the cf table (the coefficient of r^3, 0.1666...) one unit up or down in its 12th significant
    digit: an odd power, so one end of the interval gets worse whichever way it goes.  (An even power moves both ends
    the same way, and one of the two directions then LOWERS the largest error: such a coefficient is not the place to
    show that a 12th-digit error is caught.)"""
    mp, k = rs.mp50(), rs.read_kernels_hpp()
    assert _value_errors(mp, k["rt"])[0] <= 7.5e-14
    for step in (1, -1):
        c = list(k["rt"])
        c[6] = mutate_digit(c[6], 12, step)
        assert abs(abs(c[6] - k["rt"][6]) - 1e-12) < 1e-15            # one unit of the 12th digit of 0.1666...
        e = _value_errors(mp, c)
        print("coefficient %r -> %r: value error %.4g at r = %r" % ((k["rt"][6], c[6]) + e))
        assert e[0] > 7.5e-14
