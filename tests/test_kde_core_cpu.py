"""CPU: the kernel-density rule and the credible region of bart_amd/csrc/kde_core.hpp through a stand-alone host
program (tests/kde_core_host.cpp, its own main, built here with g++ and the address / undefined-behaviour sanitizers)
that runs the very functions the device kernels run, with std::exp for the exponential.  Densities and moments are
held to an mpmath restatement under the bound derived in tests/kde_restate.py, to scipy.stats.gaussian_kde under that
bound plus scipy's own distance from mpmath on the same case, the region to a restatement on Python floats bit for
bit.  And the refusals of bartrt_kde / bartrt_kde_dev / bartrt_hpd_pdf, which need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kde_restate as kr  # noqa: E402

EINVAL = -1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return kr.build_host(tmp_path_factory.mktemp("kde_core"))


@pytest.fixture(scope="module")
def tile(host):
    T = int(host("tile", [0.0])[0])
    assert T >= 256 and T % kr.MOMENT_ROWS == 0 and T // kr.MOMENT_ROWS == kr.LEAVES_PER_TILE
    return T


@pytest.fixture(scope="module")
def cases(tile):
    return kr.make_cases(tile)


CASE_NAMES = list(kr.make_cases(2048))


def _check_case(name, case, got, T, eps_exp):
    pdf, stat, nonfinite = got
    for s, c in enumerate(case["cols"]):
        idx = kr.named_indices(case["grid"][s], stat[s, 1])
        ref = kr.exact_column(case["x"], c, case["grid"][s], idx, case["bw"], case["ok"], T, eps_exp)
        kr.assert_column(name, s, ref, pdf[s], stat[s], nonfinite[s], idx)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cases_within_the_bound_of_mpmath(host, tile, cases, name):
    case = cases[name]
    got = kr.host_kde(host, case["x"], case["cols"], case["grid"], case["bw"], case["ok"])
    _check_case(name, case, got, tile, kr.EPS_EXP_HOST)


def test_what_the_cases_hold(host, tile, cases):
    """The contents the cases are named for are there: non-finite values counted, degenerate columns NaN beside a good
    one, far points exactly zero."""
    c = cases["2T+3 rows x 128 points, masked, inf and NaN in the data"]
    _, stat, nonfinite = kr.host_kde(host, c["x"], c["cols"], c["grid"], c["bw"], c["ok"])
    assert np.all(nonfinite >= 1) and np.all(stat[:, 0] + nonfinite == c["ok"].sum())
    c = cases["a constant column and an n = 1 column beside a good one"]
    pdf, stat, _ = kr.host_kde(host, c["x"], c["cols"], c["grid"], c["bw"])
    assert np.isnan(pdf[0]).all() and stat[0, 2] == 0.0 and np.isnan(stat[0, 3]) and stat[0, 1] == 2.5
    assert np.isnan(pdf[1]).all() and stat[1, 0] == 1 and stat[1, 1] == 4.25 and np.isnan(stat[1, 2:]).all()
    assert np.isfinite(pdf[2]).all() and pdf[2].max() > 0.1
    c = cases["a mask that removes all but one row"]
    pdf, stat, _ = kr.host_kde(host, c["x"], c["cols"], c["grid"], c["bw"], c["ok"])
    assert np.isnan(pdf).all() and np.all(stat[:, 0] == 1) and np.isnan(stat[:, 3]).all()
    c = cases["grid points so far out that every term is dropped"]
    pdf, _, _ = kr.host_kde(host, c["x"], c["cols"], c["grid"], c["bw"])
    assert np.all(pdf[0, ::2] == 0.0) and np.all(pdf[0, 1::2] > 0.0)


@pytest.mark.parametrize("bw", ["scott", "silverman", 0.3])
@pytest.mark.parametrize("kind", ["normal", "bimodal", "radius"])
def test_against_scipy(host, tile, kind, bw):
    """scipy.stats.gaussian_kde(col, bw_method)(grid): our distance from it is at most our derived bound plus scipy's own
    distance from the mpmath values on the same case.  The bimodal column's 68 % region has two runs.  The radius-like
    column's std: a raw-moment variance (E x^2 - mean^2, condition 1e9) would lose every digit; the shifted two-pass
    leaves and the merges of the rule leave rounding errors of the accumulation only, which for 2 T + 3 rows walk
    randomly over 256 additions a leaf and one addition a merge: a few ulp (the worst case is std_bound, asserted in
    the cases above), here held to 8."""
    from scipy.stats import gaussian_kde
    nrows = 2 * tile + 3
    col = kr._column(kind, nrows, np.random.default_rng(20))
    x = col.reshape(-1, 1)
    grid = kr._grid_for(col, 128)[None]
    pdf, stat, _ = kr.host_kde(host, x, [0], grid, bw)
    idx = kr.named_indices(grid[0], stat[0, 1])
    ref = kr.exact_column(x, 0, grid[0], idx, bw, None, tile, kr.EPS_EXP_HOST)
    kr.assert_column("scipy/" + kind, 0, ref, pdf[0], stat[0], 0, idx)
    sp = gaussian_kde(col, bw_method=bw)(grid[0])
    own = np.abs(sp[idx] - ref["pdf"])
    print("scipy's distance from mpmath:", own, "ours from scipy:", np.abs(pdf[0, idx] - sp[idx]))
    assert np.all(np.abs(pdf[0, idx] - sp[idx]) <= ref["pdf_bound"] + own)
    sp_h = gaussian_kde(col, bw_method=bw).factor * np.std(col, ddof=1)
    assert abs(stat[0, 3] - sp_h) <= ref["h_bound"] + abs(sp_h - ref["h"])
    if kind == "bimodal":
        mask, thr, inc, runs = kr.host_hpd(host, pdf[0], 0.6827)
        assert runs == 2 and not mask[np.argmin(np.abs(grid[0] - 1.5))]
    if kind == "radius":
        ulp = np.spacing(ref["std"])
        print("std: %d ulp from mpmath" % round(abs(stat[0, 2] - ref["std"]) / ulp))
        assert abs(stat[0, 2] - ref["std"]) <= 8 * ulp
        raw = np.sqrt(max(np.mean(col * col) - np.mean(col) ** 2, 0.0))
        assert abs(raw - ref["std"]) > 1e6 * ulp             # (what the rule avoids)


HPD_CASES = {
    "ties: the lower index wins": ([0.5, 0.9, 0.9, 0.5, 0.9, 0.1], (0.3, 0.5, 0.7, 0.9)),
    "a single point": ([0.17], (0.01, 0.6827, 1.0)),
    "p = 1": ([0.0, 0.4, 0.0, 0.0, 0.4, 0.0, 0.2], (1.0,)),
    "bimodal": ([0.01, 0.3, 0.4, 0.02, 0.0, 0.01, 0.35, 0.38, 0.03, 0.0], (0.6827, 0.9545)),
    "a NaN": ([0.1, float("nan"), 0.3], (0.5, 1.0)),
    "a negative value": ([0.1, -0.2, 0.3], (0.5,)),
    "total == 0": ([0.0, 0.0, 0.0, 0.0], (0.6827, 1.0)),
    "sums that round": ([0.1, 0.2, 0.3, 0.7, 1e-17, 0.1, 0.1, 0.1], (0.1, 0.5, 0.9, 1.0)),
}


@pytest.mark.parametrize("name", list(HPD_CASES))
def test_hpd_pdf_is_the_restatement_bit_for_bit(host, name):
    pdf, ps = HPD_CASES[name]
    for p in ps:
        mask, thr, inc, runs = kr.host_hpd(host, pdf, p)
        wmask, wthr, winc, wruns = kr.region_restate(pdf, p)
        assert np.array_equal(mask, wmask) and runs == wruns, (name, p)
        assert np.array([thr, inc]).tobytes() == np.array([wthr, winc]).tobytes(), (name, p)


def test_hpd_pdf_properties(host):
    mask, thr, inc, runs = kr.host_hpd(host, [0.5, 0.9, 0.9, 0.5, 0.9, 0.1], 0.3)
    assert list(np.nonzero(mask)[0]) == [1, 2] and thr == 0.9 and runs == 1
    mask, thr, inc, runs = kr.host_hpd(host, [0.17], 0.5)
    assert mask.all() and (thr, inc, runs) == (0.17, 0.17, 1)
    pdf = [0.0, 0.4, 0.0, 0.0, 0.4, 0.0, 0.2]
    mask, thr, inc, runs = kr.host_hpd(host, pdf, 1.0)
    assert np.array_equal(mask, np.asarray(pdf) > 0) and runs == 3          # p = 1: every point with density, no other
    mask, _, _, runs = kr.host_hpd(host, HPD_CASES["bimodal"][0], 0.6827)
    assert runs == 2 and list(np.nonzero(mask)[0]) == [2, 6, 7]
    for pdf in ([0.1, float("nan"), 0.3], [0.0, 0.0], [0.1, -0.2]):
        mask, thr, inc, runs = kr.host_hpd(host, pdf, 0.5)
        assert not mask.any() and (thr, inc, runs) == (0.0, 0.0, 0)


def test_the_histogram_region_is_unchanged(tmp_path_factory):
    """hist::hpd now runs the code it shares with the density's region: the same integers as before."""
    import hist_restate as hr
    run = hr.build_host(tmp_path_factory.mktemp("hist_core_again"))
    rng = np.random.default_rng(4)
    for counts in ([5, 9, 9, 5, 9, 1], [0, 0, 0], [17], list(rng.integers(0, 50, 40)), [2 ** 52, 2 ** 52 + 1, 3]):
        for p in (0.3, 0.6827, 1.0):
            mask, thr, inc, runs = hr.host_hpd(run, counts, p)
            wmask, wthr, winc, wruns = hr.hpd_restate(counts, p)
            assert np.array_equal(mask, wmask) and (thr, inc, runs) == (wthr, winc, wruns)


# ---- refusals: no device is needed, the arguments are checked first -------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from bart_amd import build, transit_module as trm
    build.build()
    return trm.lib()


def _raw(lib, dev, nrows=20, ld=4, cols=(1, 3), ngrid=5, grid=None, rule=0, factor=0.0, null=()):
    """bartrt_kde / _dev with pre-filled outputs (host memory for both: a refused call touches nothing and dereferences
    none of it): -> (rc, message, pdf, stat, nonfinite)."""
    from bart_amd import transit_module as trm
    nsel = len(cols)
    ns, ng = max(nsel, 1), max(min(ngrid, 1025), 1)
    c = np.ascontiguousarray(cols if nsel else [0], np.int32)
    g = np.tile(np.linspace(0.0, 1.0, ng), (ns, 1)) if grid is None else np.ascontiguousarray(grid, np.double)
    x = np.random.default_rng(0).random((20, 4))
    pdf, stat, nonfinite = np.full((ns, ng), 7.0), np.full((ns, 4), 7.0), np.full(ns, 7, np.uint64)
    arg = lambda name, a: None if name in null else trm._ptr(a)
    args = [arg("x", x), nrows, ld, None, nsel, arg("cols", c), ngrid, arg("grid", g), rule, factor, arg("pdf", pdf),
            arg("stat", stat), arg("nonfinite", nonfinite)]
    rc = lib.bartrt_kde_dev(*args, None) if dev else lib.bartrt_kde(*args)
    return rc, lib.bartrt_last_error().decode(), pdf, stat, nonfinite


def _bad_grid(v):
    g = np.tile(np.linspace(0.0, 1.0, 5), (2, 1))
    g[1, 3] = v
    return g


NULL_XC, NULL_REST = "null buffer (x, cols)", "null buffer (grid, pdf, stat, nonfinite)"
# what the message says after "kde: " / "kde_dev: ": the whole text for the NULL cases (True), its beginning otherwise
REFUSALS = {
    "no column": (dict(cols=()), "nsel = 0 is outside 1..64", False),
    "65 columns": (dict(cols=tuple(range(4)) * 16 + (0,)), "nsel = 65 is outside 1..64", False),
    "a negative column": (dict(cols=(1, -1)), "cols[1] = -1 is outside 0..ld - 1 (ld = 4)", True),
    "a column at ld": (dict(cols=(4, 1)), "cols[0] = 4 is outside 0..ld - 1 (ld = 4)", True),
    "ld below the largest column + 1": (dict(ld=3), "cols[1] = 3 is outside 0..ld - 1 (ld = 3)", True),
    "no grid point": (dict(ngrid=0), "ngrid = 0 is outside 1..1024", True),
    "1025 grid points": (dict(ngrid=1025), "ngrid = 1025 is outside 1..1024", True),
    "an infinite grid value": (dict(grid=_bad_grid(np.inf)), "grid[1][3] is not finite", True),
    "a NaN grid value": (dict(grid=_bad_grid(np.nan)), "grid[1][3] is not finite", True),
    "no row": (dict(nrows=0), "nrows = 0 is outside 1..2147483647", True),
    "2^31 rows": (dict(nrows=2 ** 31), "nrows = 2147483648 is outside 1..2147483647", True),
    "x is NULL": (dict(null=("x",)), NULL_XC, True),
    "cols is NULL": (dict(null=("cols",)), NULL_XC, True),
    "grid is NULL": (dict(null=("grid",)), NULL_REST, True),
    "pdf is NULL": (dict(null=("pdf",)), NULL_REST, True),
    "stat is NULL": (dict(null=("stat",)), NULL_REST, True),
    "nonfinite is NULL": (dict(null=("nonfinite",)), NULL_REST, True),
    "an unknown rule": (dict(rule=3), "bw_rule = 3 is none of", False),
    "a negative rule": (dict(rule=-1), "bw_rule = -1 is none of", False),
    "rule 2 with factor 0": (dict(rule=2, factor=0.0), "bw_factor = 0.000000 is not a finite number above 0", True),
    "rule 2 with a negative factor": (dict(rule=2, factor=-0.5), "bw_factor = -0.500000 is not a finite number above 0", True),
    "rule 2 with a NaN factor": (dict(rule=2, factor=float("nan")), "bw_factor = ", False),
}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_name_the_argument_and_touch_nothing(lib, case, dev):
    kw, text, whole = REFUSALS[case]
    rc, msg, pdf, stat, nonfinite = _raw(lib, dev, **kw)
    pre = "kde_dev: " if dev else "kde: "
    assert rc == EINVAL and msg.startswith(pre), msg
    said = msg[len(pre):]
    assert said == text if whole else said.startswith(text), msg
    assert np.all(pdf == 7.0) and np.all(stat == 7.0) and np.all(nonfinite == 7)


def test_hpd_pdf_refusals_and_the_call_itself(lib):
    from bart_amd import engine, transit_module as trm
    for pdf, p, name in (([0.1, 0.2], 0.0, "p"), ([0.1, 0.2], 1.5, "p"), ([0.1, 0.2], float("nan"), "p"), ([], 0.5, "n =")):
        with pytest.raises(trm.TransitError, match=name):
            engine.hpd_pdf(pdf, p)
    d = C.c_double()
    i = C.c_int()
    m = np.zeros(2, np.uint8)
    v = np.array([0.1, 0.2])
    for args in ((None, 2, 0.5, trm._ptr(m), C.byref(d), C.byref(d), C.byref(i)),
                 (trm._ptr(v), 2, 0.5, None, C.byref(d), C.byref(d), C.byref(i)),
                 (trm._ptr(v), 2, 0.5, trm._ptr(m), None, C.byref(d), C.byref(i)),
                 (trm._ptr(v), 2, 0.5, trm._ptr(m), C.byref(d), C.byref(d), None)):
        assert lib.bartrt_hpd_pdf(*args) == EINVAL and "null buffer" in lib.bartrt_last_error().decode()
    for pdf in HPD_CASES.values():
        for p in pdf[1]:
            mask, thr, inc, runs = engine.hpd_pdf(pdf[0], p)
            wmask, wthr, winc, wruns = kr.region_restate(pdf[0], p)
            assert np.array_equal(mask, wmask) and runs == wruns
            assert np.array([thr, inc]).tobytes() == np.array([wthr, winc]).tobytes()
    rows = C.c_long()
    assert lib.bartrt_kde_tile(C.byref(rows)) == 0 and rows.value >= 256
    assert lib.bartrt_kde_tile(None) == EINVAL and lib.bartrt_kde_chunk(None) == EINVAL
    assert lib.bartrt_kde_set_chunk(-1) == EINVAL and "kde_set_chunk" in lib.bartrt_last_error().decode()


# ---- the command line: the two refusals come before anything is read or initialised ---------------------------------
@pytest.mark.parametrize("argv, says", [
    (["--marginals-kde"], "--marginals-kde adds to the file --marginals writes"),
    (["--marginals-kde", "--marginals-kde-points", "64"], "--marginals-kde adds to the file --marginals writes"),
    (["--marginals", "m.npz", "--marginals-kde", "--marginals-kde-points", "0"], "--marginals-kde-points is a number of grid points: 1 .. 1024"),
    (["--marginals", "m.npz", "--marginals-kde", "--marginals-kde-points", "1025"], "--marginals-kde-points is a number of grid points: 1 .. 1024"),
])
def test_retrieve_refuses_kde_options_that_do_not_fit(tmp_path, capsys, argv, says):
    from bart_amd import retrieve
    with pytest.raises(SystemExit) as stop:
        retrieve.main(["-c", str(tmp_path / "absent.cfg")] + argv)
    assert stop.value.code == 2 and says in capsys.readouterr().err


def test_retrieve_takes_kde_options_that_fit(tmp_path, capsys):
    """With --marginals and 1 .. 1024 points the options pass: the run then stops at the configuration that is not
    there, not at an option."""
    from bart_amd import retrieve
    for points in ("1", "1024"):
        with pytest.raises(BaseException) as stop:
            retrieve.main(["-c", str(tmp_path / "absent.cfg"), "--marginals", "m.npz", "--marginals-kde",
                           "--marginals-kde-points", points])
        assert "marginals-kde" not in capsys.readouterr().err and "marginals-kde" not in str(stop.value)
