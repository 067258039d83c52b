"""CPU: the binning rule, the range and the highest-density region of bart_amd/csrc/hist_core.hpp through a stand-alone
host program (tests/hist_core_host.cpp, its own main, built here with g++ and the address / undefined-behaviour
sanitizers) that runs the very functions the device kernels run.  Counts are held to np.histogram and np.histogram2d
as integers, the range to np.nanmin / np.nanmax bit for bit, the region to a restatement on Python integers: there is
no tolerance in this file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hist_restate as hr  # noqa: E402


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return hr.build_host(tmp_path_factory.mktemp("hist_core"))


def _case(nbins, nrows, seed, families=hr.FAMILIES):
    """Three selected columns out of five, out of order, one per edge family."""
    cols = [3, 0, 4][:len(families)]
    edges = np.stack([hr.edges_of(f, nbins) for f in families])
    return hr.matrix_for(edges, nrows, 5, cols, seed), cols, edges


@pytest.mark.parametrize("nbins", [1, 2, 7, 20, 128])
def test_counts_equal_numpy(host, nbins):
    """Every edge, its two neighbours, the infinities, NaN, both zeros with an edge at 0.0, a value below and one
    above: h1 is np.histogram's, h2 np.histogram2d's, out the numpy comparisons', and every row is accounted for."""
    nrows = 3 * (nbins + 1) + 7 + 150
    x, cols, edges = _case(nbins, nrows, seed=nbins)
    for s in range(3):                       # the special values are all there
        col = x[:, cols[s]]
        assert all((col == v).any() for v in hr.special_values(edges[s]) if not np.isnan(v)) and np.isnan(col).any()
        assert (np.signbit(col) & (col == 0.0)).any() and (~np.signbit(col) & (col == 0.0)).any()
    h1, out, h2 = hr.host_marginals(host, x, cols, edges)
    w1, wout, w2 = hr.numpy_counts(x, cols, edges)
    assert np.array_equal(h1, w1) and np.array_equal(out, wout) and np.array_equal(h2, w2)
    assert np.all(out >= 1)
    assert np.all(h1.sum(axis=1) + out.sum(axis=1) == nrows)
    assert h2.shape == (3, nbins, nbins)


def test_uniform_edges_equal_numpy_with_a_range(host):
    """edges = np.linspace(lo, hi, n + 1) against numpy's own bins=n, range=(lo, hi), 1-D and 2-D."""
    rng = np.random.default_rng(5)
    for trial in range(20):
        lo = float(rng.normal() * 10.0 ** rng.integers(-3, 4))
        hi = lo + float(rng.random() * 10.0 ** rng.integers(-3, 4)) + 1e-9
        n = int(rng.integers(1, 40))
        e = np.linspace(lo, hi, n + 1)
        edges = np.stack([e, e])
        x = hr.matrix_for(edges, 3 * (n + 1) + 60, 2, [0, 1], seed=trial)
        h1, out, h2 = hr.host_marginals(host, x, [0, 1], edges)
        fin = np.isfinite(x).all(axis=1)
        for s in range(2):
            v = x[:, s][np.isfinite(x[:, s])]
            assert np.array_equal(h1[s], np.histogram(v, bins=n, range=(lo, hi))[0].astype(np.uint64)), (trial, s)
        want = np.histogram2d(x[fin, 0], x[fin, 1], bins=n, range=[[lo, hi], [lo, hi]])[0]
        assert np.array_equal(h2[0], want.astype(np.uint64)), trial


def test_mask_equals_the_compacted_matrix(host):
    x, cols, edges = _case(20, 300, seed=2)
    ok = np.random.default_rng(2).random(300) < 0.7
    got = hr.host_marginals(host, x, cols, edges, ok)
    want = hr.numpy_counts(x, cols, edges, ok)
    compact = hr.host_marginals(host, np.ascontiguousarray(x[ok]), cols, edges)
    for g, w, c in zip(got, want, compact):
        assert np.array_equal(g, w) and np.array_equal(g, c)
    assert np.all(got[0].sum(axis=1) + got[1].sum(axis=1) == ok.sum())
    none = hr.host_marginals(host, x, cols, edges, np.zeros(300))
    assert all(not a.any() for a in none)


def test_the_test_can_tell_a_uniform_estimate_from_the_rule(host):
    """On log-spaced edges a binning that trusts the uniform estimate is wrong, and these inputs show it; on np.linspace
    edges even it is nearly right, which is why the log family is in every test."""
    e = hr.edges_of("log", 20)
    x = hr.column_for(e, 400, seed=1).reshape(-1, 1)
    want = hr.numpy_counts(x, [0], e[None])[0][0]
    assert not np.array_equal(hr.wrong_uniform_only(x[:, 0], e), want)
    assert np.array_equal(hr.host_marginals(host, x, [0], e[None], pairs=False)[0][0], want)


def test_range_is_nanmin_nanmax_bit_for_bit(host):
    rng = np.random.default_rng(8)
    n = 200
    x = rng.normal(size=(n, 6)) * 10.0 ** rng.integers(-300, 300, (n, 6))
    x[rng.random((n, 6)) < 0.1] = np.nan
    x[::7, 1], x[3::7, 1] = np.inf, -np.inf
    x[5::9, 2], x[6::9, 2] = -0.0, 0.0                      # both zeros inside the range
    x[:, 4] = np.nan                                        # no finite value
    x[:, 5] = np.where(np.arange(n) % 2 == 0, -0.0, 0.0)    # nothing but the two zeros
    cols = [5, 1, 4, 2, 0]
    for ok in (None, rng.random(n) < 0.6):
        lohi, nfin = hr.host_range(host, x, cols, ok)
        want, wn = hr.numpy_range(x, cols, ok)
        assert np.array_equal(nfin, wn)
        # bit for bit, NaN pair included; the column of zeros by value here and by the header's own rule below
        assert np.array_equal(lohi[1:].view(np.uint64), want[1:].view(np.uint64))
        assert np.array_equal(lohi[0], want[0]) and np.signbit(lohi[0, 0]) and not np.signbit(lohi[0, 1])
        assert np.isnan(lohi[2]).all() and nfin[2] == 0
    lohi, nfin = hr.host_range(host, x, cols, np.zeros(n))
    assert np.isnan(lohi).all() and not nfin.any()


HPD_CASES = {
    "ties: the lower index wins": ([5, 9, 9, 5, 9, 1], (0.3, 0.5, 0.7, 0.9)),
    "one bin": ([17], (0.01, 0.6827, 1.0)),
    "all-zero counts": ([0, 0, 0, 0], (0.6827, 1.0)),
    "bimodal": ([1, 30, 40, 2, 0, 1, 35, 38, 3, 0], (0.6827, 0.9545)),
    "p N lands on a cumulative count": ([50, 25, 15, 10], (0.5, 0.75, 0.9, 1.0)),
    "empty bins between": ([0, 4, 0, 0, 4, 0, 2], (0.4, 0.8, 1.0)),
}


@pytest.mark.parametrize("name", list(HPD_CASES))
def test_hpd_against_python_integers(host, name):
    counts, ps = HPD_CASES[name]
    for p in ps:
        mask, thr, inc, runs = hr.host_hpd(host, counts, p)
        wmask, wthr, winc, wruns = hr.hpd_restate(counts, p)
        assert np.array_equal(mask, wmask) and (thr, inc, runs) == (wthr, winc, wruns), (name, p)
        N = sum(counts)
        assert inc == sum(c for c, m in zip(counts, mask) if m) and float(inc) >= p * N
        if N:
            assert thr == min(c for c, m in zip(counts, mask) if m)


def test_hpd_properties(host):
    """The cases by what they are about: the tie, p = 1, the bimodal runs, the exact landing."""
    mask, thr, inc, runs = hr.host_hpd(host, [5, 9, 9, 5, 9, 1], 0.3)
    assert list(np.nonzero(mask)[0]) == [1, 2] and (thr, inc, runs) == (9, 18, 1)       # 9 < 11.4, 18 >= 11.4
    for counts in ([0, 4, 0, 0, 4, 0, 2], [3, 0, 0], [0, 0, 7], list(np.random.default_rng(1).integers(0, 3, 50))):
        mask, thr, inc, runs = hr.host_hpd(host, counts, 1.0)
        # p = 1: every non-empty bin, and never an empty one
        assert np.array_equal(mask, np.asarray(counts) > 0) and inc == sum(counts) and thr >= 1
    mask, _, _, runs = hr.host_hpd(host, [1, 30, 40, 2, 0, 1, 35, 38, 3, 0], 0.6827)
    assert runs == 2 and list(np.nonzero(mask)[0]) == [2, 6, 7]              # 40 + 38 + 35 = 113 >= 0.6827 * 150
    mask, thr, inc, runs = hr.host_hpd(host, [50, 25, 15, 10], 0.75)
    assert list(mask) == [True, True, False, False] and (thr, inc, runs) == (25, 75, 1)  # 75 >= 0.75 * 100 exactly
    mask, thr, inc, runs = hr.host_hpd(host, [0, 0, 0], 0.5)
    assert not mask.any() and (thr, inc, runs) == (0, 0, 0)


def test_edges_check(host):
    as_int = lambda v: int(v.view(np.int64)[0])
    assert as_int(host("edges", [3, 0.0, 1.0, 2.0, 3.0])) == -1
    assert as_int(host("edges", [3, 0.0, 1.0, 1.0, 3.0])) == 2
    assert as_int(host("edges", [3, 0.0, 2.0, 1.0, 3.0])) == 2
    assert as_int(host("edges", [2, 0.0, 1.0, np.inf])) == 2
    assert as_int(host("edges", [2, np.nan, 1.0, 2.0])) == 0
    assert as_int(host("edges", [1, -0.0, 0.0])) == 1
