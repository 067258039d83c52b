"""The elementary functions of the RT kernels -- exp_rt_n / exp_rt and exp_core of csrc/kernels.hpp, exp_rt_fma3 of
csrc/lbl.hip -- restated with mpmath at 50 digits.

The sources are read as data (numbers only): the interpolants' coefficients, log2(e), the one-step ln2 of exp_rt and
the hi / lo pair of exp_core.  The restatement does in exact arithmetic what the device does in fp64:

  n = the integer nearest x * log2e_d, ties to even     (what the FMA with the 1.5 * 2^52 shifter delivers: the sum
                                                          is rounded once, at a magnitude whose unit is 1)
  r = x - n * ln2_d                 (exp_rt)             the header's constants, nothing rounded
  r = x - n * hi - n * lo           (exp_core)
  p(r) by Horner, then * 2^n

so what it measures against mpmath.exp is the approximation error of the interpolant and of the rounded ln2; the
fp64 rounding of the device's own evaluation comes on top and is held on the GPU (tests/test_gpu_rt_math.py), on the
same points (rt_points)."""
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS_HPP = os.path.join(ROOT, "bart_amd", "csrc", "kernels.hpp")
LBL_HIP = os.path.join(ROOT, "bart_amd", "csrc", "lbl.hip")

X_MIN, X_MAX_RT, X_MAX_CORE = -708.0, 700.0, 709.0     # kExpMin; the Planck exponent's clamp; exp_core's stated end
LN2 = 0.6931471805599453
NUM = r"[-+]?\d+\.\d*(?:e[-+]?\d+)?"


def mp50():
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    return mp


def _body(text, head):
    """The text of the function whose definition contains `head`, up to the closing brace in column 0."""
    i = text.index(head)
    return text[i:text.index("\n}\n", i)]


def _strip(path):
    return re.sub(r"//[^\n]*", "", open(path).read())


def _rt_table(body, lead):
    """-> the ten coefficients, highest degree first: the Horner chain's start value, then cf[9]."""
    first = re.search(lead + r" = (" + NUM + r");", body).group(1)
    cf = re.search(r"cf\[9\] = \{([^}]*)\}", body).group(1)
    out = [float(first)] + [float(v) for v in re.findall(NUM, cf)]
    assert len(out) == 10, out
    return out


def read_kernels_hpp():
    """-> dict: rt (10 coefficients, highest degree first), core (12), log2e, ln2 (exp_rt's one-step constant),
    ln2_hi, ln2_lo (exp_core's pair), shift."""
    text = _strip(KERNELS_HPP)
    rt = _body(text, "void exp_rt_n(")
    core = _body(text, "double exp_core(")
    out = {"rt": _rt_table(rt, r"q\[a\]")}
    lead = re.search(r"double p = (" + NUM + r");", core).group(1)
    out["core"] = [float(lead)] + [float(v) for v in re.findall(r"p = fma\(p, r, (" + NUM + r")\);", core)]
    assert len(out["core"]) == 12, out["core"]
    l2e_rt = re.search(r"fma\(x\[a\], (" + NUM + r"), kExpShift\)", rt).group(1)
    l2e_core = re.search(r"fma\(x, (" + NUM + r"), kExpShift\)", core).group(1)
    assert float(l2e_rt) == float(l2e_core)
    out["log2e"] = float(l2e_rt)
    out["ln2"] = -float(re.search(r"fma\(t\[a\] - kExpShift, (" + NUM + r"), x\[a\]\)", rt).group(1))
    out["ln2_hi"] = -float(re.search(r"fma\(n, (" + NUM + r"), x\)", core).group(1))
    out["ln2_lo"] = -float(re.search(r"fma\(n, (" + NUM + r"), r\)", core).group(1))
    out["shift"] = float(re.search(r"kExpShift = (" + NUM + r");", text).group(1))
    return out


def read_lbl_hip():
    """-> dict: rt (the ten coefficients of exp_rt_fma3), log2e, ln2."""
    body = _body(_strip(LBL_HIP), "double exp_rt_fma3(")
    return {"rt": _rt_table(body, r"double q"),
            "log2e": float(re.search(r"fma\(x, (" + NUM + r"), kExpShift\)", body).group(1)),
            "ln2": -float(re.search(r"fma\(t - kExpShift, (" + NUM + r"), x\)", body).group(1))}


def n_of(x, log2e):
    """The integer nearest x * log2e_d, ties to even, from the exact product of the two doubles."""
    return round(Fraction(x) * Fraction(log2e))     # (round() of a Fraction rounds half to even)


def horner(mp, coef, r):
    p = mp.mpf(coef[0])
    for c in coef[1:]:
        p = p * r + mp.mpf(c)
    return p


def horner_deriv(mp, coef, r):
    """p'(r): Horner on the differentiated polynomial (degree * coefficient is formed in mpmath, not in fp64)."""
    deg = len(coef) - 1
    p = mp.mpf(0)
    for i, c in enumerate(coef[:-1]):
        p = p * r + mp.mpf(c) * (deg - i)
    return p


def exp_rt_restated(mp, x, k, coef=None):
    """-> (value, n): exp_rt in exact arithmetic on the double x; `coef` replaces the header's table."""
    n = n_of(x, k["log2e"])
    r = mp.mpf(x) - n * mp.mpf(k["ln2"])
    return mp.ldexp(horner(mp, coef or k["rt"], r), n), n


def exp_core_restated(mp, x, k):
    n = n_of(x, k["log2e"])
    r = mp.mpf(x) - n * mp.mpf(k["ln2_hi"]) - n * mp.mpf(k["ln2_lo"])
    return mp.ldexp(horner(mp, k["core"], r), n), n


def half_ln2_steps():
    """The doubles nearest (k + 1/2) ln2 inside [-708, 709] -- where n steps -- each with both neighbours."""
    mp = mp50()
    pts = []
    for k in range(-1030, 1031):
        b = float((mp.mpf(k) + mp.mpf(1) / 2) * mp.log(2))
        if X_MIN <= b <= X_MAX_CORE:
            pts += [np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)]
    return [p for p in pts if X_MIN <= p <= X_MAX_CORE]


_points = None


def rt_points():
    """The arguments both halves evaluate, all inside [-708, 709] (exp_rt takes those up to 700)."""
    global _points
    if _points is None:
        pts = [0.0, 5e-324, -5e-324, 1e-300, -1e-300]
        pts += [s * 2.0 ** -k for k in range(1, 61) for s in (1.0, -1.0)]
        pts += [X_MIN, X_MAX_RT, X_MAX_CORE]
        pts += half_ln2_steps()
        rng = np.random.default_rng(20261020)
        mag = np.exp(rng.uniform(np.log(1e-12), np.log(700.0), (2, 4096)))
        pts += list(mag[0]) + list(-mag[1])
        pts += list(rng.uniform(X_MIN, X_MAX_RT, 8192))
        _points = np.array(pts, np.float64)
        _points.setflags(write=False)
    return _points


_restated = {}


def restated_on_points(which):
    """[(x, restated value as mpf, n)] of 'exp_rt' on the points up to 700 or of 'exp_core' on all of them; computed
    once per process and shared (not to be modified)."""
    if which not in _restated:
        mp, k = mp50(), read_kernels_hpp()
        x = rt_points()
        if which == "exp_rt":
            x = x[x <= X_MAX_RT]
            _restated[which] = (x, [exp_rt_restated(mp, float(v), k) for v in x])
        else:
            _restated[which] = (x, [exp_core_restated(mp, float(v), k) for v in x])
    return _restated[which]
