"""Batched contribution functions and band transmittance on the GPU (include/bartrt.h, bartrt_cf_*;
bart_amd.engine.contribution / transmittance; bart_amd.cf) against the CPU oracle's optical depth of the
same case written with `toomuch 1e100`, passed through the tests' restatement of code/cf.py
(tests/cf_restate.py) and the band weights of bart_amd.cf.filter_windows.  Every comparison is relative
to the row's largest |value| (per walker and filter; per walker and wavenumber for the full output): TOL is 1e-9 of
that maximum.  The kernels are held tightly -- to an exact column under a derived bound -- in tests/test_gpu_cf_exact.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cf_restate  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "bart_amd", "transit")
TOL = 1e-9
ENOTSUP = -4


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    scale = np.max(np.abs(b), axis=-1, keepdims=True)
    return float(np.max(np.abs(a - b) / np.where(scale > 0, scale, 1.0)))


def walkers(case, n, seed=3):
    rng = np.random.default_rng(seed)
    L = len(case.press_bar)
    out = []
    for _ in range(n):
        t = case.temp0 + rng.uniform(-300, 600) + 150 * np.sin(np.linspace(0, rng.uniform(1, 6), L) + rng.uniform(0, 6))
        t = np.clip(t, 410.0, 2990.0)
        ab = case.abund0.copy()
        for s in range(2, ab.shape[1]):
            ab[:, s] *= 10 ** rng.uniform(-2, 1)
        q = 1 - ab[:, 2:].sum(1)
        ab[:, 1] = 0.85 / 0.15 * q / (1 + 0.85 / 0.15)
        ab[:, 0] = q / (1 + 0.85 / 0.15)
        out.append(case.profiles(t, ab).ravel())
    return np.array(out)


def write_filters(d, wn):
    """Four filters on the grid: two that overlap, one past the grid's upper edge, a narrow one."""
    from bart_amd import synth
    lo, hi = wn[0], wn[-1]
    spec = [(lo + 50.3, lo + 200.0, "hat"), (lo + 150.0, lo + 400.7, "ramp"), (hi - 80.0, hi + 100.0, "hat"),
            (lo + 10.0, lo + 30.0, "ramp")]
    out = []
    for j, (a, b, shape) in enumerate(spec):
        wl = np.linspace(1e4 / b, 1e4 / a, 31)
        x = np.linspace(0.0, 1.0, wl.size)
        p = os.path.join(d, "f%d.dat" % j)
        synth.write_filter(p, wl, np.sin(np.pi * x) ** 2 if shape == "hat" else 0.2 + 0.8 * x)
        out.append(p)
    return out


def inf_cfg(case, d):
    """The case's configuration with toomuch 1e100 (what cf.cf_tconfig writes for the reference's rerun)."""
    from bart_amd import synth
    keys = dict(case.keys)
    keys["toomuch"] = "1e100"
    p = os.path.join(d, "inf.cfg")
    synth.write_tcfg(p, keys)
    return p


def oracle_band(o, case, prof, windows, kind):
    """-> (band [nf, L], full [W, L]), atm layer order, from the oracle's tau (layers from the top)."""
    from bart_amd import cf
    _, tau, _ = o.run(prof, want_tau=True)
    L = len(case.press_bar)
    if kind == "cf":
        v = cf_restate.contribution(prof[:L], case.press_bar, tau.T, o.wn)
    else:
        v = np.exp(-tau.T)
    return cf.band_average(v, windows).T[:, ::-1], v.T[:, ::-1]


@pytest.fixture(scope="module")
def cfcase(small_case, tmp_path_factory):
    from bart_amd import cf
    d = str(tmp_path_factory.mktemp("cf"))
    files = write_filters(d, small_case.wn)
    return small_case, files, cf.filter_windows(small_case.wn, files), inf_cfg(small_case, d)


@pytest.mark.parametrize("cut", ["slant", "vertical"])
@pytest.mark.parametrize("integ", [0, 1, 2])
def test_contribution_eclipse_rules_and_cuts(cfcase, integ, cut):
    """W = 777 (not a multiple of 64), four molecules + H2-H2 CIA, the engine's own toomuch of 10 under either
    cut: the result is that of an infinite toomuch under the integration rule in force."""
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    case, files, win, cfg = cfcase
    profs = walkers(case, 7, seed=10 + integ)
    engine.init(case.tcfg)
    try:
        trm.set_integ(integ)
        trm.set_cut(cut)
        got, norm = engine.contribution(profs, files)
        o = orc.OracleEngine(cfg, integ=integ)
        for w in range(len(profs)):
            ref, _ = oracle_band(o, case, profs[w], win, "cf")
            assert _rel(got[w], ref) < TOL
        from bart_amd import cf
        assert np.array_equal(norm, cf.normalize(got))
        assert got.shape == (7, 4, 100) and np.all(np.isfinite(got))
    finally:
        trm.free_memory()


@pytest.mark.parametrize("n", [1, 64])
def test_contribution_batch_sizes(cfcase, n):
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    case, files, win, cfg = cfcase
    profs = walkers(case, n, seed=40 + n)
    engine.init(case.tcfg)
    try:
        got = engine.contribution(profs, win, normalize=False)
        o = orc.OracleEngine(cfg)
        for w in range(0, n, 9):
            assert _rel(got[w], oracle_band(o, case, profs[w], win, "cf")[0]) < TOL
    finally:
        trm.free_memory()


def test_cloud_deck_and_rayleigh(cfcase):
    """Engine-wide cloud top and scattering, as run_transit_batch takes them: below the deck tau repeats."""
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    case, files, win, cfg = cfcase
    profs = walkers(case, 5, seed=77)
    engine.init(case.tcfg)
    try:
        trm.set_cloudtop(-1.5)
        trm.set_scattering(2, 0.0)
        got = engine.contribution(profs, win, normalize=False)
        tr = engine.transmittance(profs, win)
        o = orc.OracleEngine(cfg)
        o.set_cloudtop(-1.5)
        o.set_scattering(2, 0.0)
        for w in range(len(profs)):
            assert _rel(got[w], oracle_band(o, case, profs[w], win, "cf")[0]) < TOL
            assert _rel(tr[w], oracle_band(o, case, profs[w], win, "tr")[0]) < TOL
        deep = case.press_bar >= 10 ** -1.5      # atm order (bottom first): the deck's layer and those below it
        below = np.zeros_like(deep)
        below[:-1] = deep[:-1] & deep[1:]
        assert below.sum() > 10 and np.all(got[:, :, below] == 0.0)
    finally:
        trm.free_memory()


def test_several_molecules_and_cia_tables(tmp_path):
    from bart_amd import cf, engine, synth, transit_module as trm
    from oracle import rt_oracle as orc
    case = synth.make_case(str(tmp_path), nlayers=61, nwave=555, opmol=("H2O", "CO", "CH4"), cia=2, seed=5)
    files = write_filters(str(tmp_path), case.wn)
    win = cf.filter_windows(case.wn, files)
    cfg = inf_cfg(case, str(tmp_path))
    profs = walkers(case, 3, seed=8)
    engine.init(case.tcfg)
    try:
        got = engine.contribution(profs, files, normalize=False)
        o = orc.OracleEngine(cfg)
        for w in range(len(profs)):
            assert _rel(got[w], oracle_band(o, case, profs[w], win, "cf")[0]) < TOL
    finally:
        trm.free_memory()


def test_transmittance_eclipse_and_full_output(cfcase):
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    case, files, win, cfg = cfcase
    profs = walkers(case, 3, seed=91)
    engine.init(case.tcfg)
    try:
        band, full = engine.transmittance(profs, win, full=True)
        cband, cfull = engine.contribution(profs, win, normalize=False, full=True)
        o = orc.OracleEngine(cfg)
        for w in range(len(profs)):
            rb, rf = oracle_band(o, case, profs[w], win, "tr")
            assert _rel(band[w], rb) < TOL and _rel(full[w], rf) < TOL
            rb, rf = oracle_band(o, case, profs[w], win, "cf")
            assert _rel(cband[w], rb) < TOL and _rel(cfull[w], rf) < TOL
        assert full.shape == (3, 777, 100)
    finally:
        trm.free_memory()


def test_transit_engine_transmittance_and_enotsup(tmp_path):
    from bart_amd import cf, engine, synth, transit_module as trm
    from oracle import rt_oracle as orc
    case = synth.make_case(str(tmp_path), nlayers=80, nwave=333, extra_keys={"solution": "transit", "starrad": 1.145})
    files = write_filters(str(tmp_path), case.wn)
    win = cf.filter_windows(case.wn, files)
    cfg = inf_cfg(case, str(tmp_path))
    profs = walkers(case, 4, seed=12)
    engine.init(case.tcfg)
    try:
        band, full = engine.transmittance(profs, files, full=True)
        o = orc.OracleEngine(cfg)
        for w in range(len(profs)):
            rb, rf = oracle_band(o, case, profs[w], win, "tr")
            assert _rel(band[w], rb) < TOL and _rel(full[w], rf) < TOL
        out = np.zeros((4, 4, 80))
        p = np.ascontiguousarray(profs)
        assert trm.lib().bartrt_cf_batch(trm._ptr(p), 4, p.shape[1], 0, trm._ptr(out), None, None) == ENOTSUP
        assert b"eclipse" in trm.lib().bartrt_last_error()
    finally:
        trm.free_memory()


def test_sharded_engine_is_not_supported(cfcase):
    from bart_amd import engine, transit_module as trm
    case, files, win, cfg = cfcase
    idx0, npts, resp, _ = win
    engine.init(case.tcfg, shard=(0, 2))
    try:
        rc = trm.lib().bartrt_cf_setup(len(idx0), trm._ptr(idx0), trm._ptr(npts), trm._ptr(resp))
        assert rc == ENOTSUP and b"sharded" in trm.lib().bartrt_last_error()
    finally:
        trm.free_memory()


def test_bits_do_not_depend_on_the_batch(cfcase, monkeypatch):
    """A profile alone and at position 5 of a batch of 13 give the same bits; two runs give the same bits;
    chunks of one walker (a workspace cap below one walker's share) give the same bits."""
    from bart_amd import engine, transit_module as trm
    case, files, win, cfg = cfcase
    profs = walkers(case, 13, seed=55)
    engine.init(case.tcfg)
    try:
        alone = engine.contribution(profs[5:6], win, normalize=False)
        batch = engine.contribution(profs, win, normalize=False)
        again = engine.contribution(profs, win, normalize=False)
        assert np.array_equal(alone[0], batch[5]) and np.array_equal(batch, again)
        monkeypatch.setenv("BARTRT_CF_WORKSPACE_BYTES", "1")     # one walker per chunk
        small = engine.contribution(profs, win, normalize=False)
        assert np.array_equal(small, batch)
    finally:
        trm.free_memory()


def test_ten_thousand_posterior_samples(cfcase):
    from bart_amd import engine, transit_module as trm
    case, files, win, cfg = cfcase
    base = walkers(case, 7, seed=66)
    profs = base[np.arange(10000) % 7]
    engine.init(case.tcfg)
    try:
        one = engine.transmittance(base, win)
        got = engine.transmittance(profs, win)
        assert got.shape == (10000, 4, 100)
        assert np.array_equal(got, one[np.arange(10000) % 7])
    finally:
        trm.free_memory()


def test_bad_profile_is_flagged_and_leaves_its_neighbours(cfcase):
    from bart_amd import engine, transit_module as trm
    case, files, win, cfg = cfcase
    profs = walkers(case, 6, seed=31)
    bad = profs.copy()
    bad[2, 7] = np.nan
    engine.init(case.tcfg)
    try:
        good = engine.contribution(profs, win, normalize=False)
        got, ok = engine.contribution(bad, win, normalize=False, want_ok=True)
        assert list(ok) == [1, 1, 0, 1, 1, 1]
        keep = [0, 1, 3, 4, 5]
        assert np.array_equal(got[keep], good[keep]) and np.all(np.isnan(got[2]))
        with pytest.raises(trm.TransitError, match="non-finite"):
            engine.contribution(bad, win, normalize=False)       # ok == NULL: the call fails
    finally:
        trm.free_memory()


def test_a_cf_call_disturbs_nothing(cfcase):
    """run_transit_batch spectra, get_tau after a single-profile call and the radii of the latest run are the same
    bits whether or not a CF call ran in between."""
    from bart_amd import engine, transit_module as trm
    case, files, win, cfg = cfcase
    profs = walkers(case, 9, seed=17)
    engine.init(case.tcfg)
    try:
        n = trm.get_no_samples()
        spec_a = engine.run_batch(profs)
        trm.run_transit(profs[3], n)
        rad_a = np.zeros(100)
        trm.check(trm.lib().bartrt_get_radius(trm._ptr(rad_a), 100))
        tau_a, last_a = engine.get_tau()
        engine.contribution(profs[::-1], win)
        engine.transmittance(profs[:2], win, full=True)
        rad_b = np.zeros(100)
        trm.check(trm.lib().bartrt_get_radius(trm._ptr(rad_b), 100))
        tau_b, last_b = engine.get_tau()
        assert np.array_equal(tau_a, tau_b) and np.array_equal(last_a, last_b) and np.array_equal(rad_a, rad_b)
        engine.contribution(profs[1:4], win)
        assert np.array_equal(engine.run_batch(profs), spec_a)
    finally:
        trm.free_memory()


def test_device_form_matches_the_host_form(cfcase):
    import torch
    from bart_amd import engine, transit_module as trm
    case, files, win, cfg = cfcase
    profs = walkers(case, 5, seed=23)
    engine.init(case.tcfg)
    try:
        host = engine.contribution(profs, win, normalize=False)
        engine.cf_setup(win)
        d = torch.tensor(profs, dtype=torch.float64, device="cuda")
        ok = torch.zeros(5, dtype=torch.uint8, device="cuda")
        band = engine.contribution_dev(d, d_ok=ok)
        tr = engine.transmittance_dev(d)
        torch.cuda.synchronize()
        assert np.array_equal(band.cpu().numpy(), host) and ok.cpu().numpy().tolist() == [1] * 5
        assert np.array_equal(tr.cpu().numpy(), engine.transmittance(profs, win))
    finally:
        trm.free_memory()


def _cf_tconfig(date_dir):
    """code/cf.py:36-64, cf_tconfig: bestFit_tconfig.cfg -> cf_tconfig.cfg (toomuch 1e100, savefiles yes)."""
    lines = open(os.path.join(date_dir, "bestFit_tconfig.cfg")).readlines()
    for i, ln in enumerate(lines):
        key = ln.split()[0]
        if key == "toomuch":
            lines[i] = "toomuch 1e100\n"
        elif key == "verb":
            lines[i] = "verb 0\n"
        elif key == "outspec":
            lines[i] = "outspec ./cf-flux.dat\n"
    with open(os.path.join(date_dir, "cf_tconfig.cfg"), "w") as f:
        f.writelines(lines)
        f.writelines("savefiles yes")


def _read_tau_dat(path, nlayers):
    """code/cf.py:68-94, readTauDat -> tau [L][W] (from the top), wns."""
    lines = open(path).readlines()
    while lines[0].startswith("#") or not lines[0].strip():
        lines.pop(0)
    tau = np.array([ln.split() for ln in lines[1:-1:3]], float).T
    wns = np.array([float(ln.split()[1]) for ln in lines[0:-1:3]])
    assert tau.shape[0] == nlayers
    return tau, wns


def test_dropin_against_the_cli_tau_dat(tmp_path):
    """BART.py:626-644 end to end: the product's `transit` on a cf_tconfig.cfg written as cf.cf_tconfig writes
    it, its tau.dat through the restatement, against bart_amd.cf.cf / .transmittance on the same directory
    (which run nothing and write no tau.dat).  tau.dat holds 12 digits: 1e-6."""
    from bart_amd import cf, synth
    d = str(tmp_path)
    case = synth.make_case(d, nlayers=50, nwave=300, extra_keys={"outspec": os.path.join(d, "spec.dat")})
    os.replace(case.tcfg, os.path.join(d, "bestFit_tconfig.cfg"))
    files = write_filters(d, case.wn)
    _cf_tconfig(d)
    r = subprocess.run([CLI, "-c", "cf_tconfig.cfg"], cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    tau, wns = _read_tau_dat(os.path.join(d, "tau.dat"), 50)
    os.remove(os.path.join(d, "tau.dat"))
    win = cf.filter_windows(wns, files)
    from bart_amd import hostio
    _, p_bar, temp, _ = hostio.readatm(os.path.join(d, "synth.atm"))
    v = cf_restate.contribution(temp, p_bar, tau, wns)
    ref = cf.band_average(v, win).T[:, ::-1]
    ref_tr = cf.band_average(np.exp(-tau), win).T[:, ::-1]
    got, norm = cf.cf(d + "/", "synth.atm", files, plot=False)
    tr = cf.transmittance(d + "/", "synth.atm", files, plot=False)
    assert not os.path.exists(os.path.join(d, "tau.dat"))
    assert got.shape == (4, 50) and _rel(got, ref) < 1e-6 and _rel(tr, ref_tr) < 1e-6
    assert _rel(norm, cf.normalize(ref)) < 1e-6
