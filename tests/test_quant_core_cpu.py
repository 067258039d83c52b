"""CPU: the exact order statistics and the percentile rule (bart_amd/csrc/quant_core.hpp) through a stand-alone host
program (tests/quant_core_host.cpp, its own main, built here with g++ and the address / undefined-behaviour sanitizers)
that runs the very functions the device kernels run.  Selection is held to np.sort bit for bit; the percentile rule to
np.percentile: the header states numpy's own expression (_lerp), so the interpolated values are asserted EQUAL, which
is inside the 2-ulp bound the GPU tests use."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quant_restate as qr  # noqa: E402


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return qr.build_host(tmp_path_factory.mktemp("quant_core"))


def test_key_map_round_trips_and_orders_like_np_sort(host):
    rng = np.random.default_rng(3)
    vals = np.concatenate([qr.SPECIALS, rng.normal(size=40), -rng.random(10) * 1e-310, [1.0, -1.0, 2.5e300]])
    rng.shuffle(vals)
    out = host("keys", vals).view(np.uint64)
    keys, back = out[:vals.size], out[vals.size:]
    # the inverse gives every value back bit for bit, NaN (np.nan: a clear sign bit) included
    assert np.array_equal(back, vals.view(np.uint64))
    # the key order is np.sort's order (stable: the two zeros have distinct keys, -0 first; np.sort may swap them)
    by_key = vals[np.argsort(keys, kind="stable")]
    assert qr.same_bits(by_key, np.sort(vals))
    assert np.isnan(by_key[-1]) and by_key[-2] == np.inf and by_key[0] == -np.inf
    z = np.array([0.0, -0.0])
    kz = host("keys", z).view(np.uint64)[:2]
    assert kz[1] < kz[0]


def test_nan_of_either_sign_sorts_behind_inf(host):
    """A NaN with its sign bit set would, flipped like a negative number, land below -inf; the header clears the sign
    first.  The inverse gives the payload back with a clear sign bit."""
    neg_nan = np.array([0xfff8000000000001, 0x7ff8000000000001, 0xfff0000000000001], np.uint64).view(np.double)
    vals = np.concatenate([neg_nan, [np.inf, -np.inf, 0.0]])
    out = host("keys", vals).view(np.uint64)
    keys, back = out[:6], out[6:]
    assert np.all(keys[:3] > keys[3]) and keys[4] < keys[5] < keys[3]
    assert np.array_equal(back[:3], vals.view(np.uint64)[:3] & np.uint64(0x7fffffffffffffff))
    assert np.array_equal(back[3:], vals.view(np.uint64)[3:])


@pytest.mark.parametrize("n", [2, 3, 64, 257])
def test_selection_is_np_sort_bit_for_bit(host, n):
    x = qr.adversarial_columns(n, seed=n)
    for ranks in ([0], [n - 1], [0, n - 1], [n // 2] * 16, list(np.random.default_rng(n).integers(0, n, 16))):
        got = host_sel = qr.host_select(host, x, ranks)
        assert qr.same_bits(got, qr.sorted_ranks(x, ranks)), ranks
        assert host_sel.shape == (len(ranks), x.shape[1])


def test_selection_nan_column_and_mask(host):
    n = 65
    x = qr.adversarial_columns(n, seed=11)
    x[::3, 2] = np.nan
    ranks = [0, 5, n - 1, n - 2, 30]
    got = qr.host_select(host, x, ranks)
    assert qr.same_bits(got, qr.sorted_ranks(x, ranks))
    assert np.isnan(got[2, 2]) and np.isnan(got[3, 2]) and not np.isnan(got[0, 2])
    ok = (np.arange(n) % 2 == 0)
    m = int(ok.sum())
    ranks = [0, m - 1, m // 2]
    got = qr.host_select(host, x, ranks, ok)
    assert qr.same_bits(got, qr.sorted_ranks(x, ranks, ok))
    assert qr.same_bits(got, qr.host_select(host, x[ok], ranks))
    # a rank at or above the rows that count: NaN
    assert np.all(np.isnan(qr.host_select(host, x, [m], ok)))
    assert np.all(np.isnan(qr.host_select(host, x, [0], np.zeros(n))))


def test_one_row(host):
    x = np.array([[1.5, -0.0, np.nan]])
    assert qr.same_bits(qr.host_select(host, x, [0, 0]), np.vstack([x, x]))


@pytest.mark.parametrize("n", [1, 2, 3, 10, 1000])
def test_percentile_rule_is_np_percentile(host, n):
    """On arange(n) the percentile IS the virtual index: lo + w must be np.percentile's value, lo its floor."""
    out = host("rule", np.array([[n, q] for q in qr.PERCENTS]).ravel()).reshape(-1, 3)
    for (lo, hi, w), q in zip(out, qr.PERCENTS):
        v = float(np.percentile(np.arange(n, dtype=np.double), q))
        assert lo == np.floor((n - 1) * (q / 100.0)) and hi == min(lo + 1, n - 1) and 0.0 <= w < 1.0
        assert lo + w == pytest.approx(v, abs=1e-9 * max(1, n))
        if n > 1:
            assert w == (n - 1) * (q / 100.0) - lo
        else:
            assert (lo, hi, w) == (0, 0, 0)


@pytest.mark.parametrize("n", [1, 2, 3, 10, 1000])
def test_interpolated_value_equals_np_percentile(host, n):
    """The header reproduces numpy's expression, so equality is asserted (and the 2-ulp bound with it)."""
    rng = np.random.default_rng(100 + n)
    x = np.concatenate([rng.normal(size=(n, 3)) * [1.0, 1e-200, 1e200], 1500.0 + 700.0 * rng.random((n, 2))], axis=1)
    s = np.sort(x, axis=0)
    rule = host("rule", np.array([[n, q] for q in qr.PERCENTS]).ravel()).reshape(-1, 3)
    for (lo, hi, w), q in zip(rule, qr.PERCENTS):
        a, b = s[int(lo)], s[int(hi)]
        trip = np.stack([a, b, np.full_like(a, w)], axis=1).ravel()
        got = host("lerp", np.concatenate([[a.size], trip]))
        want = np.percentile(x, q, axis=0)
        assert qr.within_two_ulp(got, want, a, b)
        assert np.array_equal(got, want), (n, q)
