"""Posterior contribution functions / band transmittance on the GPU: per-walker radius, cloud top and scattering
inside one batch (include/bartrt.h, bartrt_cf_batch_over), parameters in (bartrt_cf_params) and the drop-in behind
the reference's posterior figure (bart_amd.cf.posterior), against the CPU oracle run walker by walker under the
walker's own settings with `toomuch 1e100`, through tests/cf_restate.py and bart_amd.cf.band_average.  Every
comparison is relative to the row's largest |value|, at 1e-9 (the conventions of tests/test_gpu_cf.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cf_restate  # noqa: E402,F401
from test_gpu_cf import _rel, inf_cfg, oracle_band, walkers, write_filters  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9
EINVAL, ENOTSUP = -1, -4
NAN = float("nan")
G = os.path.join(HERE, "golden")


# ---- inputs (their conditions are asserted with the oracle alone, before anything runs on the GPU) --------------
def overrides(case, n=8, seed=4):
    """n walkers' (radius km, log10 cloud-top bar, Rayleigh value): every radius within +-10 % of the cfg's and at
    least 2 % away from it, cloud tops inside the column, above its top layer (1e-5 bar) and absent (NaN), Rayleigh
    values of their own (1e3 to 1e5 times the H2 cross-section: an eclipse column hardly feels its reference radius
    -- the hydrostatic steps go with g r^2 = g0 R0^2 -- so a walker without a cloud is told apart by its scattering)."""
    rng = np.random.default_rng(seed)
    r0 = float(case.keys["refradius"])
    rad = r0 * (1.0 + rng.choice([-1.0, 1.0], n) * rng.uniform(0.02, 0.10, n))
    cloud = np.array([-1.3, NAN, -6.2, 0.4, NAN, -3.1, -5.7, -2.2])[np.arange(n) % 8]
    ray = rng.uniform(3.0, 5.0, n)
    return np.column_stack([rad, cloud, ray])


def oracle_under(o, over3):
    """The oracle under one walker's settings (a NaN cloud top: no cloud, the state the cfg leaves)."""
    o.set_radius(over3[0])
    o.c.has_cloud, o.c.cloudtop = 0, 0.0
    if over3[1] == over3[1]:
        o.set_cloudtop(over3[1])
    o.set_scattering(1, over3[2])


def assert_overrides_matter(o, case, profs, over, win, kind, engine_wide):
    """For every walker the oracle under its own settings and under the engine-wide ones differ by more than 1e-3
    of the row maximum in at least one band: an ignored override cannot pass."""
    refs = []
    for w in range(len(profs)):
        oracle_under(o, over[w])
        refs.append(oracle_band(o, case, profs[w], win, kind))
        oracle_under(o, engine_wide)
        wide = oracle_band(o, case, profs[w], win, kind)[0]
        scale = np.maximum(np.max(np.abs(refs[-1][0]), axis=-1), np.max(np.abs(wide), axis=-1))
        assert np.max(np.max(np.abs(refs[-1][0] - wide), axis=-1) / scale) > 1e-3, w
    return refs


@pytest.fixture(scope="module")
def cfcase(small_case, tmp_path_factory):
    from bart_amd import cf
    d = str(tmp_path_factory.mktemp("cfp"))
    files = write_filters(d, small_case.wn)
    return small_case, files, cf.filter_windows(small_case.wn, files), inf_cfg(small_case, d)


def _batch_over(profs, over, kind, nf, L, W, full=True):
    from bart_amd import transit_module as trm
    p = np.ascontiguousarray(profs)
    band, fout = np.zeros((len(p), nf, L)), np.zeros((len(p), W, L)) if full else None
    ov = None if over is None else np.ascontiguousarray(over, np.double)
    trm.check(trm.lib().bartrt_cf_batch_over(trm._ptr(p), len(p), p.shape[1], trm._ptr(ov) if ov is not None else None,
                                             kind, trm._ptr(band), trm._ptr(fout) if full else None, None))
    return band, fout


# ---- 1. overrides against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("cut", ["slant", "vertical"])
@pytest.mark.parametrize("integ", [0, 1, 2])
def test_overrides_eclipse_against_the_oracle(cfcase, integ, cut):
    """W = 777, four molecules + H2-H2 CIA, eight walkers each under its own radius, cloud top and Rayleigh value
    (flag 1): band and full of bartrt_cf_batch_over against the oracle run per walker with its own setters."""
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    case, files, win, cfg = cfcase
    profs = walkers(case, 8, seed=20 + integ)
    over = overrides(case, 8, seed=4 + integ)
    wide = (float(case.keys["refradius"]), NAN, 0.5)
    o = orc.OracleEngine(cfg, integ=integ)
    refs = assert_overrides_matter(o, case, profs, over, win, "cf", wide)
    engine.init(case.tcfg)
    try:
        trm.set_integ(integ)
        trm.set_cut(cut)
        trm.set_scattering(1, wide[2])
        engine.cf_setup(win)
        for kind, name in ((0, "cf"), (1, "tr")):
            band, full = _batch_over(profs, over, kind, 4, 100, 777)
            for w in range(len(profs)):
                if name == "tr":
                    oracle_under(o, over[w])
                rb, rf = refs[w] if name == "cf" else oracle_band(o, case, profs[w], win, "tr")
                print("eclipse integ %d %s walker %d: band %.3g full %.3g" % (integ, name, w, _rel(band[w], rb), _rel(full[w], rf)))
                assert _rel(band[w], rb) < TOL and _rel(full[w], rf) < TOL
        # the Python front end passes the same array on
        assert np.array_equal(engine.contribution(profs, win, normalize=False, over=over),
                              _batch_over(profs, over, 0, 4, 100, 777, full=False)[0])
    finally:
        trm.free_memory()


def test_radius_alone_on_the_eclipse_engine(cfcase):
    """An eclipse column feels its reference radius through (r / R0)^2 along the column only, and the walkers above
    carry a cloud top or a Rayleigh value as well: here the radius is the ONLY override (-10 % and +10 %), and the
    oracle's own result moves by more than 1e-3 of the row maximum with it -- an ignored radius cannot pass."""
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    case, files, win, cfg = cfcase
    profs = walkers(case, 2, seed=21)
    r0 = float(case.keys["refradius"])
    over = np.array([[0.9 * r0, NAN, NAN], [1.1 * r0, NAN, NAN]])
    o = orc.OracleEngine(cfg)
    refs = assert_overrides_matter(o, case, profs, np.column_stack([over[:, 0], over[:, 1], [0.5, 0.5]]), win, "cf",
                                   (r0, NAN, 0.5))
    engine.init(case.tcfg)
    try:
        trm.set_scattering(1, 0.5)
        engine.cf_setup(win)
        band, full = _batch_over(profs, over, 0, 4, 100, 777)
        for w in range(2):
            print("radius alone, walker %d: band %.3g full %.3g" % (w, _rel(band[w], refs[w][0]), _rel(full[w], refs[w][1])))
            assert _rel(band[w], refs[w][0]) < TOL and _rel(full[w], refs[w][1]) < TOL
    finally:
        trm.free_memory()


def test_overrides_transit_against_the_oracle(tmp_path):
    """Transit engine: the chord depths are those of each walker's own hydrostatic radii."""
    from bart_amd import cf, engine, synth, transit_module as trm
    from oracle import rt_oracle as orc
    case = synth.make_case(str(tmp_path), nlayers=80, nwave=333, extra_keys={"solution": "transit", "starrad": 1.145})
    files = write_filters(str(tmp_path), case.wn)
    win = cf.filter_windows(case.wn, files)
    cfg = inf_cfg(case, str(tmp_path))
    profs = walkers(case, 8, seed=12)
    over = overrides(case, 8, seed=9)
    wide = (float(case.keys["refradius"]), NAN, 0.5)
    o = orc.OracleEngine(cfg)
    refs = assert_overrides_matter(o, case, profs, over, win, "tr", wide)
    engine.init(case.tcfg)
    try:
        trm.set_scattering(1, wide[2])
        engine.cf_setup(win)
        band, full = _batch_over(profs, over, 1, 4, 80, 333)
        for w in range(len(profs)):
            print("transit walker %d: band %.3g full %.3g" % (w, _rel(band[w], refs[w][0]), _rel(full[w], refs[w][1])))
            assert _rel(band[w], refs[w][0]) < TOL and _rel(full[w], refs[w][1]) < TOL
        assert np.array_equal(engine.transmittance(profs, win, over=over), band)
    finally:
        trm.free_memory()


# ---- 2. null overrides are today's call ------------------------------------------------------------------------
def test_null_overrides_are_the_plain_call(cfcase):
    from bart_amd import engine, transit_module as trm
    case, files, win, cfg = cfcase
    profs = walkers(case, 6, seed=61)
    engine.init(case.tcfg)
    try:
        trm.set_cloudtop(-1.0)
        for kind, fn in ((0, engine.contribution), (1, engine.transmittance)):
            kw = {"normalize": False} if kind == 0 else {}
            band0, full0 = fn(profs, win, full=True, **kw)
            band1, full1 = _batch_over(profs, None, kind, 4, 100, 777)
            assert np.array_equal(band0, band1) and np.array_equal(full0, full1)
            # ... and a row of NaN is the engine-wide setting too
            band2, full2 = _batch_over(profs, np.full((6, 3), NAN), kind, 4, 100, 777)
            assert np.array_equal(band0, band2) and np.array_equal(full0, full2)
    finally:
        trm.free_memory()


# ---- 3. independence and repeatability --------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_neighbours_or_the_chunks(cfcase, monkeypatch):
    import torch
    from bart_amd import engine, transit_module as trm
    case, files, win, cfg = cfcase
    profs = walkers(case, 13, seed=55)
    over = overrides(case, 13, seed=2)
    other = overrides(case, 13, seed=3)
    other[5] = over[5]
    engine.init(case.tcfg)
    try:
        trm.set_scattering(1, 0.0)
        alone = engine.contribution(profs[5:6], win, normalize=False, over=over[5:6])
        batch = engine.contribution(profs, win, normalize=False, over=over)
        neigh = engine.contribution(profs, win, normalize=False, over=other)
        again = engine.contribution(profs, win, normalize=False, over=over)
        assert np.array_equal(alone[0], batch[5]) and np.array_equal(neigh[5], batch[5])
        assert np.array_equal(batch, again) and not np.array_equal(neigh[4], batch[4])
        d_prof, d_over = torch.from_numpy(profs).cuda(), torch.from_numpy(over).cuda()
        one = engine.contribution_dev(d_prof, over=d_over)
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy(), batch)
        monkeypatch.setenv("BARTRT_CF_WORKSPACE_BYTES", "1")     # one walker per chunk
        assert np.array_equal(engine.contribution(profs, win, normalize=False, over=over), batch)
        small = engine.contribution_dev(d_prof, over=d_over)
        torch.cuda.synchronize()
        assert np.array_equal(small.cpu().numpy(), batch)
    finally:
        trm.free_memory()


# ---- 4. parameters in -------------------------------------------------------------------------------------------
def worker_case(d, solution):
    """A worker-shaped case whose cfg fits a cloud top and a Rayleigh value (and, transit, the radius):
    -> (case, cfg path, WorkerConfig, pmin, pmax) with params = T(p) [5], extras, log10 CH4 factor."""
    from bart_amd import BARTfunc, synthcfg
    transit = solution == "transit"
    extra = {"solution": "transit", "starrad": 1.145} if transit else None
    r0 = float("%.2f" % (1.35 * 7.1492e7 * 1e-3))      # synth.make_case's refradius (km) for the default planet
    mid = [-2.0, 0.0, 1.0, 0.0, 0.98] + ([r0] if transit else []) + [-2.0, 1.0, -0.5]
    case, cfg = synthcfg.make_worker_case(d, nwave=601, nlayers=60, params=mid, nfilters=4, solution=solution,
                                          extra_keys=extra)
    with open(cfg, "a") as f:
        f.write("cloudtop = -2.0\nscattering = rayleigh\n")
        f.write("stepsize = " + " ".join(["0.01", "0.01", "0.0", "0.01", "0.01"] + (["50.0"] if transit else [])
                                         + ["0.1", "0.0", "0.1"]) + "\n")
    r0 = float(case.keys["refradius"])
    # The cloud top's lower bound.  Transit (transmittance only): anywhere in the column.  Eclipse: the contribution
    # function of a wavenumber is B (exp(-tau[k-1]) - exp(-tau[k])) / dlnp, and below a deck tau repeats, so a deck at
    # low pressure leaves a row whose every entry is a difference of two numbers within tau_deck of 1.  Each
    # exponential is rounded to half an ulp of 1 (5.5e-17) in the oracle and in the engine alike, so two correct
    # evaluations of that row differ by up to 1.1e-16 / tau_deck of its maximum: the 1e-9 of this suite is a statement
    # about the code only while the row's largest difference is well above 1.1e-7.  With the deck below 10^-1.5 bar the
    # oracle's own rows keep it above 1e-6 at every wavenumber (the test asserts 5e-7, on the oracle's tau alone); decks high in
    # the column, above it and absent are the overrides test's, on a grid whose rows stay conditioned.
    pmin = [-2.6, -0.6, 0.5, 0.0, 0.80] + ([0.9 * r0] if transit else []) + [-5.5 if transit else -1.5, -1.0, -2.0]
    pmax = [-1.6, 0.6, 1.2, 1.0, 1.60] + ([1.1 * r0] if transit else []) + [1.0, 3.0, 4.25]
    return case, cfg, BARTfunc.WorkerConfig.from_cfg(cfg), np.array(pmin), np.array(pmax)


def draw_rows(pmin, pmax, n=64, seed=8):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(pmin + (pmax - pmin) * rng.random((n, len(pmin))))


def ptargs_of(wcfg):
    """BARTfunc.py:204-208 from the TEP file, as bart_amd.BARTfunc.Worker forms them."""
    from bart_amd import hostio
    tep = hostio.TepFile(wcfg.tep_name)
    v = lambda k: float(tep.getvalue(k)[0])
    rplanet, mplanet = v("Rp") * hostio.Rjup, v("Mp") * hostio.Mjup
    return [v("Rs") * hostio.Rsun, v("Ts"), wcfg.tint, v("a") * hostio.AU, 100.0 * hostio.G_NEWTON * mplanet / rplanet ** 2]


def pyhalf_rows(case, wcfg, rows, nextra, conditions=True):
    """oracle/pyhalf.py's profile and status of every row (the extras cut out)."""
    from oracle import pyhalf
    ptargs = ptargs_of(wcfg)
    out = [pyhalf.step_profiles(np.r_[p[:5], p[5 + nextra:]], case.press_bar, case.abund0, case.species,
                                wcfg.molfit, ptargs, wcfg.Tmin, wcfg.Tmax) for p in rows]
    status = np.array([s for _, s in out])
    # the conditions on the inputs: both kinds of rejection occur, and at most a quarter of the rows is rejected
    if conditions:
        assert (status == 1).any() and (status == 2).any() and (status != 0).sum() <= len(rows) // 4, status
    return out, status


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_parameters_in_against_the_oracle_chain(tmp_path, solution):
    import torch
    from bart_amd import BARTfunc, cf, engine, transit_module as trm
    from oracle import rt_oracle as orc
    case, cfg, wcfg, pmin, pmax = worker_case(str(tmp_path), solution)
    nextra = 3 if solution == "transit" else 2
    rows = draw_rows(pmin, pmax)
    halves, status_ref = pyhalf_rows(case, wcfg, rows, nextra)
    win = cf.filter_windows(case.wn, wcfg.filters)
    o = orc.OracleEngine(inf_cfg(case, str(tmp_path)))
    w = BARTfunc.Worker(wcfg, carry=False)
    try:
        assert (w.nradfit, w.ncloud, w.nray) == ((1, 1, 1) if solution == "transit" else (0, 1, 1))
        _, st_step = engine.step_batch(rows, w.nfilters)
        kinds = [("tr", engine.transmittance_from_params, engine.transmittance_from_params_dev)]
        if solution == "eclipse":
            kinds.append(("cf", lambda p, f, full: engine.contribution_from_params(p, f, normalize=False, full=full),
                          engine.contribution_from_params_dev))
        for name, host, dev in kinds:
            band, full, status = host(rows, win, full=True)
            assert np.array_equal(status, st_step) and np.array_equal(status, status_ref)
            for r in range(len(rows)):
                if status[r]:
                    assert np.all(np.isnan(band[r]))
                    continue
                ex = rows[r, 5:5 + nextra]
                oracle_under(o, (ex[0] if nextra == 3 else float(case.keys["refradius"]), ex[-2], ex[-1]))
                rb, rf = oracle_band(o, case, halves[r][0].ravel(), win, name)
                if name == "cf":
                    # the condition on the inputs (worker_case): no row of the oracle's own contribution function
                    # is a difference of transmittances closer than 5e-7
                    _, tau, _ = o.run(halves[r][0].ravel(), want_tau=True)
                    assert np.abs(np.diff(np.exp(-tau), axis=1)).max(axis=1).min() >= 5e-7, r
                print("%s %s row %d: band %.3g full %.3g" % (solution, name, r, _rel(band[r], rb), _rel(full[r], rf)))
                assert _rel(band[r], rb) < TOL and _rel(full[r], rf) < TOL
            d_band, d_full, d_status = dev(torch.from_numpy(rows).cuda(), full=True)
            torch.cuda.synchronize()
            assert np.array_equal(d_status.cpu().numpy(), status)
            assert np.array_equal(d_band.cpu().numpy(), band, equal_nan=True)
            good = status == 0
            assert np.array_equal(d_full.cpu().numpy()[good], full[good])
        if solution == "eclipse":
            # the transmittance has no such conditioning: decks anywhere in the column, and above it, on this engine too
            lo = pmin.copy()
            lo[5] = -5.5
            high = draw_rows(lo, pmax, n=32, seed=9)
            assert (high[:, 5] < -1.5).sum() >= 10 and (high[:, 5] < -5.0).any()
            hh, hst = pyhalf_rows(case, wcfg, high, nextra, conditions=False)
            band, full, status = engine.transmittance_from_params(high, win, full=True)
            assert np.array_equal(status, hst) and (hst == 0).sum() >= 16
            for r in np.nonzero(hst == 0)[0]:
                oracle_under(o, (float(case.keys["refradius"]), high[r, 5], high[r, 6]))
                rb, rf = oracle_band(o, case, hh[r][0].ravel(), win, "tr")
                print("eclipse tr high-deck row %d: band %.3g full %.3g" % (r, _rel(band[r], rb), _rel(full[r], rf)))
                assert _rel(band[r], rb) < TOL and _rel(full[r], rf) < TOL
    finally:
        w.close()


# ---- 5. every T(p) model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pttype,code,key", [
    ("iso", 1, "iso"), ("madhu_noinv", 2, "noinv"), ("madhu_inv", 3, "inv"),
    ("adiabatic", 4, "adiab"), ("piette", 5, "piette")])
def test_every_pt_model_runs_through_the_parameter_call(demo_case, tmp_path, pttype, code, key):
    """The golden file's parameter draws (tests/test_gpu_step.py) under the bounds 400-3000 K: statuses as the pinned
    restatement's, accepted rows against the oracle chain.  ("line" is the model of the test above.)"""
    from bart_amd import cf, engine, transit_module as trm
    from oracle import pyhalf, rt_oracle as orc
    c = demo_case
    wg, ptg = np.load(os.path.join(G, "wine_golden.npz")), np.load(os.path.join(G, "pt_golden.npz"))
    files = write_filters(str(tmp_path), c.wn)
    win = cf.filter_windows(c.wn, files)
    o = orc.OracleEngine(inf_cfg(c, str(tmp_path)))
    params = np.ascontiguousarray(ptg[key + "_params"])
    if key == "adiab":      # (every golden draw of this model leaves 400-3000 K on this pressure grid)
        params = np.vstack([[[1500.0, 1.05, 0.0], [1200.0, 1.03, -1.0]], params])
    ref = [pyhalf.step_profiles(p, c.press_bar, c.abund0, c.species, [], None, 400.0, 3000.0, pttype=pttype)
           for p in params]
    st_ref = np.array([s for _, s in ref])
    keep = np.r_[np.nonzero(st_ref == 0)[0][:4], np.nonzero(st_ref != 0)[0][:2]].astype(int)
    assert (st_ref[keep] == 0).any()
    params = np.ascontiguousarray(params[keep])
    engine.init(c.tcfg)
    try:
        engine.step_setup(None, 400.0, 3000.0, c.abund0, [], wg["demo_idx0"], wg["demo_npts"],
                          wg["demo_nifilter"], wg["demo_istarfl"], float(wg["rprs"]), pttype=code)
        band, status = engine.contribution_from_params(params, win, normalize=False)
        assert np.array_equal(status, st_ref[keep])
        for r, k in enumerate(keep):
            if status[r]:
                assert np.all(np.isnan(band[r]))
            else:
                rb = oracle_band(o, c, ref[k][0].ravel(), win, "cf")[0]
                print("%s row %d: %.3g" % (pttype, r, _rel(band[r], rb)))
                assert _rel(band[r], rb) < TOL
    finally:
        trm.free_memory()


# ---- 6. state is left alone -------------------------------------------------------------------------------------
def test_a_parameter_call_disturbs_nothing(tmp_path):
    from bart_amd import BARTfunc, cf, engine, transit_module as trm
    case, cfg, wcfg, pmin, pmax = worker_case(str(tmp_path), "eclipse")
    rows = draw_rows(pmin, pmax, n=9, seed=5)
    win = cf.filter_windows(case.wn, wcfg.filters)
    profs = walkers(case, 4, seed=17)
    w = BARTfunc.Worker(wcfg, carry=False)
    try:
        n, L = trm.get_no_samples(), engine.nlayers()
        trm.set_cloudtop(-0.5)
        trm.set_radius(0.97 * float(case.keys["refradius"]))
        spec_a = trm.run_transit(profs[1], n)
        batch_a = engine.run_batch(profs)
        trm.run_transit(profs[3], n)
        rad_a = np.zeros(L)
        trm.check(trm.lib().bartrt_get_radius(trm._ptr(rad_a), L))
        tau_a, last_a = engine.get_tau()
        engine.step_set_carry(True)                     # no effect on the parameter call
        b1, s1 = engine.transmittance_from_params(rows, win)
        engine.step_set_carry(False)
        b2, s2 = engine.transmittance_from_params(rows, win)
        assert np.array_equal(b1, b2, equal_nan=True) and np.array_equal(s1, s2)
        engine.contribution_from_params(rows[:3], win)
        rad_b = np.zeros(L)
        trm.check(trm.lib().bartrt_get_radius(trm._ptr(rad_b), L))
        tau_b, last_b = engine.get_tau()
        assert np.array_equal(tau_a, tau_b) and np.array_equal(last_a, last_b) and np.array_equal(rad_a, rad_b)
        # the engine-wide setters still act on the next run as before
        assert np.array_equal(trm.run_transit(profs[1], n), spec_a)
        assert np.array_equal(engine.run_batch(profs), batch_a)
    finally:
        w.close()


# ---- 7. errors --------------------------------------------------------------------------------------------------
def test_errors(tmp_path):
    from bart_amd import BARTfunc, cf, engine, transit_module as trm
    lib = trm.lib()
    case, cfg, wcfg, pmin, pmax = worker_case(str(tmp_path / "e"), "eclipse")
    rows = draw_rows(pmin, pmax, n=3)
    win = cf.filter_windows(case.wn, wcfg.filters)
    band, st = np.zeros((3, 4, 60)), np.zeros(3, np.int32)
    call = lambda p, kind=1: lib.bartrt_cf_params(trm._ptr(p), 3, p.shape[1], kind, trm._ptr(band), None, trm._ptr(st))
    engine.init(case.tcfg)
    try:
        engine.cf_setup(win)
        assert call(rows) == EINVAL and b"step_setup" in lib.bartrt_last_error()
    finally:
        trm.free_memory()
    w = BARTfunc.Worker(wcfg, carry=False)
    try:
        assert call(rows) == EINVAL and b"cf_setup" in lib.bartrt_last_error()
        engine.cf_setup(win)
        assert call(rows) == 0
        assert call(np.ascontiguousarray(rows[:, :-1])) == EINVAL and b"npars" in lib.bartrt_last_error()
        bad = np.full((3, 3), NAN)
        bad[1, 0] = -5.0
        p = walkers(case, 3)
        assert lib.bartrt_cf_batch_over(trm._ptr(p), 3, p.shape[1], trm._ptr(bad), 1, trm._ptr(band), None, None) == EINVAL
        assert b"radius" in lib.bartrt_last_error()
        # the device form cannot look at the radii: it flags the walker and computes the others
        import torch
        d_p, d_ok = torch.from_numpy(p).cuda(), torch.ones(3, dtype=torch.uint8, device="cuda")
        plain = engine.transmittance_dev(d_p)
        got = engine.transmittance_dev(d_p, d_ok=d_ok, over=torch.from_numpy(bad).cuda())
        torch.cuda.synchronize()
        assert d_ok.cpu().numpy().tolist() == [1, 0, 1] and bool(torch.isnan(got[1]).all())
        assert torch.equal(got[[0, 2]], plain[[0, 2]])
    finally:
        w.close()
    case, cfg, wcfg, pmin, pmax = worker_case(str(tmp_path / "t"), "transit")
    rows = draw_rows(pmin, pmax, n=3)
    w = BARTfunc.Worker(wcfg, carry=False)
    try:
        engine.cf_setup(cf.filter_windows(case.wn, wcfg.filters))
        assert call(rows, 0) == ENOTSUP and b"eclipse" in lib.bartrt_last_error()
        p = walkers(case, 3)
        over = np.full((3, 3), NAN)
        assert lib.bartrt_cf_batch_over(trm._ptr(p), 3, p.shape[1], trm._ptr(over), 0, trm._ptr(band), None, None) == ENOTSUP
        assert call(rows, 1) == 0
    finally:
        w.close()


# ---- 8. the drop-in ---------------------------------------------------------------------------------------------
def test_posterior_dropin(tmp_path):
    """A synthetic output.npy in MC3's [nchains, nfree, niter] layout, fixed parameters in the cfg, burn-in dropped:
    cf.posterior against contribution_from_params on the hand-expanded parameters and numpy's percentiles."""
    from bart_amd import BARTfunc, cf, engine
    case, cfg, wcfg, pmin, pmax = worker_case(str(tmp_path), "eclipse")
    params, stepsize = cf._mcmc_vectors(cfg)
    free = np.nonzero(stepsize)[0]
    assert 0 < len(free) < len(params)
    nchains, niter, burnin = 3, 15, 4
    rng = np.random.default_rng(21)
    chains = pmin[free, None] + (pmax - pmin)[free, None] * rng.random((nchains, len(free), niter))
    np.save(str(tmp_path / "output.npy"), chains)
    hand = np.tile(params, (nchains * (niter - burnin), 1))
    hand[:, free] = np.concatenate([chains[c, :, burnin:].T for c in range(nchains)])
    res = cf.posterior(str(tmp_path / "output.npy"), cfg, wcfg.filters, burnin, chunk=7)
    assert res["kind"] == "contribution" and np.array_equal(res["samples"], hand)
    w = BARTfunc.Worker(wcfg, carry=False)
    try:
        band, status = engine.contribution_from_params(hand, wcfg.filters, normalize=False)
    finally:
        w.close()
    assert np.array_equal(res["band"], band, equal_nan=True) and np.array_equal(res["status"], status)
    good = band[status == 0]
    assert 0 < len(good)
    assert np.array_equal(res["median"], np.median(good, axis=0))
    for k, q in (("lo1", 15.87), ("hi1", 84.13), ("lo2", 2.28), ("hi2", 97.72)):
        assert np.array_equal(res[k], np.percentile(good, q, axis=0))
    # the layout bart_amd.retrieve writes: [nchains, nsteps, npars]
    own = hand.reshape(nchains, niter - burnin, len(params))
    own = np.concatenate([np.zeros((nchains, burnin, len(params))), own], axis=1)
    res2 = cf.posterior(own, cfg, wcfg.filters, burnin)
    assert np.array_equal(res2["band"], band, equal_nan=True) and np.array_equal(res2["median"], res["median"])
    tr = cf.posterior(own, cfg, wcfg.filters, burnin, thinning=3, kind="transmittance")
    assert tr["kind"] == "transmittance" and len(tr["band"]) == nchains * 4
