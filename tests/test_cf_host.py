"""CPU: the host side of the batched contribution functions (bart_amd.cf) against what the reference's
own code/cf.py computes (tests/golden/cf_golden.npz, tests/golden/make_cf_golden.py), the tests'
restatement of its arithmetic (tests/cf_restate.py), and the C entry points without a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cf_restate  # noqa: E402

G = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(G, "cf_golden.npz"))
    files = [os.path.join(G, "cf_filters", str(n)) for n in g["filters"]]
    return g, files


def _rel(a, b):
    """largest deviation per row, relative to the row's largest |value| (rows = all but the last axis)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    scale = np.max(np.abs(b), axis=-1, keepdims=True)
    return float(np.max(np.abs(a - b) / np.where(scale > 0, scale, 1.0)))


def test_filter_windows_follow_filter_cf(gold):
    from bart_amd import cf
    g, files = gold
    idx0, npts, resp, trapz = cf.filter_windows(g["wns"], files)
    assert idx0.dtype == np.int32 and npts.dtype == np.int32 and resp.size == npts.sum()
    # fcf3 runs past the grid's upper edge: its window ends on the last sample
    assert idx0[2] + npts[2] == g["wns"].size
    # fcf1 and fcf2 overlap
    assert idx0[1] < idx0[0] + npts[0]
    w = (idx0, npts, resp, trapz)
    assert _rel(cf.band_average(g["cf"], w).T, g["filt_cf"]) < 1e-12
    assert _rel(cf.band_average(g["cf"], w).T, g["filt_cf_n"]) < 1e-12
    assert _rel(cf.normalize(cf.band_average(g["cf"], w).T), g["filt_cf_norm"]) < 1e-12
    assert _rel(cf.band_average(g["transmit"], w).T, g["filt_tr"]) < 1e-12
    # the drivers' results: atm layer order
    assert _rel(cf.band_average(g["transmit"], w).T[:, ::-1], g["transmittance"]) < 1e-12
    assert _rel(cf.band_average(g["cf"], w).T[:, ::-1], g["cf_cf"]) < 1e-12
    assert _rel(cf.normalize(cf.band_average(g["cf"], w).T)[:, ::-1], g["cf_cf_norm"]) < 1e-12


def test_restatement_reproduces_planck_and_cf_eq(gold):
    g, _ = gold
    bb = cf_restate.planck(g["temp"][::-1], g["wns"])
    assert _rel(bb, g["planck"]) < 1e-13
    assert _rel(cf_restate.contribution(g["temp"], g["p_bar"], g["tau"], g["wns"]), g["cf"]) < 1e-12
    assert np.all(g["cf"][0] == 0.0)


def test_normalize_keeps_a_constant_row_with_a_warning():
    from bart_amd import cf
    x = np.array([[[0.0, 2.0, 1.0], [3.0, 3.0, 3.0]]])
    with pytest.warns(UserWarning, match="is 0"):
        y = cf.normalize(x)
    assert np.array_equal(y[0, 0], [0.0, 1.0, 0.5]) and np.array_equal(y[0, 1], x[0, 1])


def test_filter_outside_the_grid_raises(gold, tmp_path):
    from bart_amd import cf, synth
    g, files = gold
    out = str(tmp_path / "far.dat")
    synth.write_filter(out, np.linspace(1e4 / 2100.0, 1e4 / 2000.0, 11), np.ones(11))   # 2000-2100 cm-1
    with pytest.raises(ValueError, match="no sample"):
        cf.filter_windows(g["wns"], files[:1] + [out])
    one = str(tmp_path / "one.dat")                 # a single sample inside: trapz(resp) would be 0
    synth.write_filter(one, np.linspace(1e4 / 1100.6, 1e4 / 1099.6, 11), np.ones(11))
    with pytest.raises(ValueError, match="one sample"):
        cf.filter_windows(g["wns"], [one])


def test_plots_are_refused(tmp_path):
    from bart_amd import cf
    with pytest.raises(NotImplementedError, match="plot"):
        cf.cf(str(tmp_path), "x.atm", [], plot=True)
    with pytest.raises(NotImplementedError, match="plot"):
        cf.transmittance(str(tmp_path), "x.atm", [], plot=True)


def test_entry_points_without_an_engine_fail_cleanly():
    """No engine (and on this host no device): every new C entry point returns an error code."""
    from bart_amd import build, transit_module as trm
    build.build()
    lib = trm.lib()
    trm.free_memory()
    idx0 = np.array([0], np.int32)
    npts = np.array([4], np.int32)
    resp = np.ones(4)
    prof = np.ones(8)
    band = np.zeros(8)
    ok = np.zeros(1, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    codes = [lib.bartrt_cf_setup(1, p(idx0), p(npts), p(resp)),
             lib.bartrt_cf_setup(0, None, None, None),
             lib.bartrt_cf_batch(p(prof), 1, 8, 0, p(band), None, p(ok)),
             lib.bartrt_cf_batch(None, 1, 8, 1, None, None, None),
             lib.bartrt_cf_batch_dev(None, 1, 0, None, None, None, None)]
    assert all(c in (-1, -3) for c in codes), codes      # BARTRT_EINVAL / BARTRT_ENODEV
    assert b"not initialised" in lib.bartrt_last_error()
