"""CPU: the effective sample size of the resident sampler (bart_amd/csrc/ess_core.hpp) through a stand-alone host
program (tests/ess_core_host.cpp, its own main, built here with g++ and the address / undefined-behaviour sanitizers)
that runs the very functions the device kernels run.  Held against tests/ess_restate.py: the header's order restated in
plain Python doubles, bit for bit, and the lagged sums against exact rationals within the textbook bound of a
recursive sum."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ess_restate as er  # noqa: E402


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return er.build_host(tmp_path_factory.mktemp("ess_core"))


@pytest.mark.parametrize("c", er.CASES, ids=lambda c: c["id"])
def test_host_build_is_the_restatement(host, c):
    """Means, lagged sums, tau, ess, truncated and reached: the restatement's bits (ess_restate.same: NaNs at the same
    places, every other value byte for byte)."""
    chain, step, r0, r1, maxlag = er.case(c)
    n, free = r1 - r0, step > 0
    h = er.reference(host, c)
    tau, ess, trunc, acf, means, reached = er.statistic(chain, step, r0, r1, maxlag, 10.0)
    K = min(maxlag if maxlag else 1024, n - 1)
    assert h["acf"].shape == (c["nch"], c["npars"], K + 1)                      # (4 096 clamps to n - 1)
    assert er.same(h["mean"], means) and er.same(h["acf"], acf)
    assert er.same(h["tau"], tau) and er.same(h["ess"], ess)
    assert er.same(h["truncated"], trunc) and h["reached"] == reached
    # fixed and shared columns: zeros out
    assert free.any() and not free.all()
    for key in ("tau", "truncated", "acf", "mean"):
        assert not h[key][:, ~free].any(), key
    assert not h["ess"][~free].any()
    if "constant" in c:
        j = c["constant"]
        # S_0 = 0: non-finite, truncated, and never "reached", whatever the target
        assert not h["acf"][:, j].any() and np.all(np.isnan(h["tau"][:, j])) and math.isnan(h["ess"][j])
        assert np.all(h["truncated"][:, j] == 1) and h["reached"] == 0
        assert host(chain, step, r0, r1, maxlag, 0.0)["reached"] == 0
    else:
        assert np.all(h["acf"][:, free, 0] > 0.0) and np.all(np.isfinite(h["tau"][:, free]))
    # the target decides: with nothing truncated, just below the smallest ess is reached, just above is not
    if not h["truncated"][:, free].any() and "constant" not in c:
        low = float(h["ess"][free].min())
        if low > 0.0:
            assert host(chain, step, r0, r1, maxlag, low * (1 - 1e-12))["reached"] == 1
            assert host(chain, step, r0, r1, maxlag, low * (1 + 1e-12))["reached"] == 0
        else:                                        # (a handful of rows can give tau < 0: kept as computed, no clamp)
            assert host(chain, step, r0, r1, maxlag, 0.0)["reached"] == 0
    elif "constant" not in c:
        assert host(chain, step, r0, r1, maxlag, 0.0)["reached"] == 0       # (truncated: not reached at any target)


def test_no_test_below_four_rows(host):
    chain, step, r0, _, _ = er.case(er.CASES[0])
    h = host(chain, step, r0, r0 + 3, 2, 0.0)
    assert h["reached"] == 0 and h["acf"].shape == (1, 7, 3)
    assert not any(h[k].any() for k in ("tau", "ess", "truncated", "acf", "mean"))
    r = er.statistic(chain, step, r0, r0 + 3, 2, 0.0)
    assert r[5] == 0 and not any(v.any() for v in r[:5])
    # no free parameter: nothing to reach
    assert host(chain, np.zeros(7), r0, r0 + 4, 2, 0.0)["reached"] == 0


def test_lagged_sums_against_exact_rationals(host):
    """n = 300, a radius-like column 97 000 + small integers / 8.  The exact sums take the differences about THE SAME
    rounded mean the core produced, so only the summation is judged:
        |S_k - exact| <= gamma sum_r |d_r d_{r+k}|,  gamma = (n + 2) u / (1 - (n + 2) u),  u = 2^-53,
    the textbook bound of a recursive sum of n rounded products of rounded differences (Higham, Accuracy and Stability
    of Numerical Algorithms, section 4.2: n - 1 additions, one rounding of the product, one of each difference).
    Derived, not tuned."""
    n, r0 = 300, 2
    rng = np.random.default_rng(41)
    walk = np.cumsum(rng.integers(-3, 4, size=(2, n + r0 + 1)), axis=1)                    # small integers, correlated
    chain = np.zeros((2, n + r0 + 1, 3))
    chain[:, :, 1] = 97000.0 + walk / 8.0
    chain[:, :, 0] = rng.normal(size=chain.shape[:2])
    step = np.array([0.1, 0.1, 0.0])
    h = host(chain, step, r0, r0 + n, 299, 0.0)
    assert h["acf"].shape == (2, 3, 300)
    u = Fraction(1, 2 ** 53)
    gamma = (n + 2) * u / (1 - (n + 2) * u)
    worst = Fraction(0)
    for i in range(2):
        for j in (0, 1):
            col = chain[i, :, j].tolist()
            for k, (want, scale) in enumerate(er.exact_sums(col, r0, r0 + n, float(h["mean"][i, j]), 299)):
                err = abs(Fraction(float(h["acf"][i, j, k])) - want)
                assert err <= gamma * scale, (i, j, k, float(err), float(gamma * scale))
                if scale:
                    worst = max(worst, err / scale)
    print("lagged sums against exact rationals: worst error %.3g of sum |d d|; bound gamma = %.3g"
          % (float(worst), float(gamma)))


AR_SEED = 5   # checked here: with this seed the plain-Python restatement ALONE gives tau within 20 % of 3 and of 1


def _series(kind):
    rng = np.random.default_rng(AR_SEED)
    e = rng.normal(size=65536)
    if kind == "iid":
        return e
    x = np.empty_like(e)
    x[0] = e[0] / math.sqrt(1 - 0.25)
    for r in range(1, e.size):
        x[r] = 0.5 * x[r - 1] + e[r]
    return x


@pytest.mark.parametrize("kind,want", [("ar1", (1 + 0.5) / (1 - 0.5)), ("iid", 1.0)])
def test_definition_on_known_series(host, kind, want):
    """A first-order autoregression of coefficient 0.5 has tau = (1 + 0.5) / (1 - 0.5) = 3, an independent series
    tau = 1.  At n = 65 536 the window's asymptotic standard error is about 3 %, so 20 % is more than six of them.
    64 lags: the sequence turns non-positive long before."""
    x = _series(kind)
    chain = np.ascontiguousarray(x.reshape(1, -1, 1))
    step = np.array([0.1])
    col = x.tolist()
    m = er.mean(col, 0, len(col))
    tau_r, trunc_r = er.tau_of(er.lagged_sums(col, 0, len(col), m, 64), 64)
    print("%s: tau %.4f by the restatement (wanted: %.1f)" % (kind, tau_r, want))
    assert trunc_r == 0 and abs(tau_r - want) <= 0.2 * want                                # the restatement alone
    h = host(chain, step, 0, len(col), 64, 1000.0)
    assert h["truncated"][0, 0] == 0 and abs(h["tau"][0, 0] - want) <= 0.2 * want
    assert h["tau"][0, 0] == tau_r and h["ess"][0] == len(col) / tau_r and h["reached"] == 1


def test_truncated_is_never_reached(host):
    """A ramp: every pair of autocorrelations stays positive out to maxlag = 8, so the sequence is cut short, the
    entry is marked, and the target is not reached whatever it is."""
    chain = np.ascontiguousarray(np.arange(64.0).reshape(1, -1, 1))
    step = np.array([0.1])
    for target in (0.0, 1e-300, 1.0):
        h = host(chain, step, 0, 64, 8, target)
        assert np.all(h["acf"][0, 0] > 0.0) and h["truncated"][0, 0] == 1 and h["reached"] == 0
    tau, ess, trunc, acf, _, reached = er.statistic(chain, step, 0, 64, 8, 0.0)
    assert trunc[0, 0] == 1 and reached == 0 and er.same(h["tau"], tau) and er.same(h["acf"], acf)
    assert math.isfinite(h["ess"][0]) and h["ess"][0] > 0.0           # (finite and positive: truncation alone decides)
