"""GPU: the per-step kernels of csrc/step.hip (step_profiles, step_prep_profiles, step_bandflux, step_bandflux_blocks)
at the shapes where their code takes another path, against references that share nothing with them:

  expint_e2 ......... mpmath.expint(2, x) on the points of tests/test_expint_tables.py
  band integration .. math.fsum over the trapezoid terms (exact sum, rounded once), windows from 0 to 4100 samples
  energy balance .... the same exact sum, the threshold placed 1e-12 on either side of each walker's own output
  profiles .......... oracle/pyhalf.py at 5 ... 320 layers (two-lanes-per-layer limit at 128, second trip of the
                      strided loops above 256), 16 species, 16 fitted molecules, the bounds' and rejections' edges
  deep columns ...... the fused launch above 64 kB of LDS, against the oracle chain
  Piette ............ grids on which two of its eight nodes fall on one layer are refused

Every engine is a synth.make_case with one table molecule on a 650 K temperature grid unless the test says otherwise.
Figures are printed before they are asserted (run with -s)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")

TINY_NORMAL = 2.0 ** -1022
SUBNORMAL_UNIT = 2.0 ** -1074


@pytest.fixture(scope="module")
def ptg():
    return np.load(os.path.join(G, "pt_golden.npz"))


def _case(path, **kw):
    from bart_amd import synth
    kw.setdefault("opmol", ("CH4",))
    kw.setdefault("tempdelt", 650.0)
    kw.setdefault("cia", False)
    kw.setdefault("nwave", 16)
    return synth.make_case(str(path), **kw)


# ---- 3a: expint_e2 ------------------------------------------------------------------------------------------------
def test_expint_e2_against_mpmath():
    """Bounds: the table generator's stated worst case (6e-16 for x <= 1, 4e-16 above; held on the CPU by
    tests/test_expint_tables.py) plus one ulp (2.2e-16) for the device's log resp. exp: 8.2e-16 / 6.2e-16 relative where
    the exact value is a normal number; where it is subnormal, 4 units of 2^-1074 (exp's half unit, scaled by
    F(x) < 1).  Beyond the cut-off 0.0, NaN for NaN.
    Measured on an MI355X (printed below; MEASUREMENTS.md): 6.13e-16 for x <= 1 (at 0.8938), 4.48e-16 above (at 236.1),
    0.145 units in the subnormal range."""
    import mpmath
    from bart_amd import engine
    from test_expint_tables import CUTOFF, e2_points
    x = e2_points()
    got = engine.expint_e2(x)
    assert got.shape == x.shape
    worst = {"small": (0.0, None), "large": (0.0, None), "subnormal": (0.0, None)}
    with mpmath.workdps(50):
        for v, g in zip(x, got):
            v, g = float(v), float(g)
            if math.isnan(v):
                assert math.isnan(g)
                continue
            if v > CUTOFF:
                assert g == 0.0, (v, g)
                continue
            ref = mpmath.expint(2, mpmath.mpf(v)) if v > 0 else mpmath.mpf(1)
            if ref >= TINY_NORMAL:
                key, err = ("small" if v <= 1.0 else "large"), float(abs(mpmath.mpf(g) / ref - 1))
            else:
                key, err = "subnormal", float(abs(mpmath.mpf(g) - ref) / SUBNORMAL_UNIT)
            if err > worst[key][0]:
                worst[key] = (err, v)
    print("expint_e2 worst: x <= 1 %.3g (at %r), x > 1 %.3g (at %r), subnormal range %.3g units of 2^-1074 (at %r)"
          % (worst["small"] + worst["large"] + worst["subnormal"]))
    assert worst["small"][0] <= 8.2e-16, worst
    assert worst["large"][0] <= 6.2e-16, worst
    assert worst["subnormal"][0] <= 4.0, worst
    assert engine.expint_e2(np.zeros(0)).size == 0
    assert engine.expint_e2(0.0) == 1.0 and engine.expint_e2(np.inf) == 0.0


# ---- 3b / 3c: band integration and energy balance --------------------------------------------------------------------
SIZES = (0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 1026, 2048, 2049)
RPRS = 0.11
E_FAC = 4.0 * (1.35 * 7.1492e7 * 100.0) ** 2      # pyhalf.energy_out: 4 (Rp * 100)^2, Rp in metres


def _windows(W):
    """Every size that fits (and the whole grid), once from the grid's first sample and once ending on its last."""
    idx0, npts = [], []
    for n in [s for s in SIZES if s <= W] + [W]:
        idx0 += [0, W - n]
        npts += [n, n]
    return np.array(idx0, np.int32), np.array(npts, np.int32)


def _trapz_terms(y, wn):
    return np.diff(wn) * (y[1:] + y[:-1]) / 2.0


def _exact_bands(spec, wn, idx0, npts, gwt):
    """math.fsum over the terms pyhalf.bandflux adds, per (walker, window): the exact sum, rounded once."""
    out = np.zeros((len(spec), len(idx0)))
    off = 0
    for f, (i0, n) in enumerate(zip(idx0, npts)):
        for w in range(len(spec)):
            out[w, f] = math.fsum(_trapz_terms(spec[w, i0:i0 + n] * gwt[off:off + n], wn[i0:i0 + n]))
        off += n
    return out


class BandCase:
    """One engine on a grid of W samples with _windows(W) set up, four seeded spectra, and both band kernels."""

    def __init__(self, tmp_path, W, solution):
        import torch
        from bart_amd import engine, transit_module as trm
        self.torch, self.engine, self.trm = torch, engine, trm
        c = _case(tmp_path, nlayers=8, nwave=W, wnlow=1200.0, wndelt=0.5)
        engine.init(c.tcfg)
        try:
            self._setup(c, W, solution)
        except BaseException:
            trm.free_memory()
            raise

    def _setup(self, c, W, solution):
        import torch
        engine, trm = self.engine, self.trm
        assert trm.get_no_samples() == W
        self.W, self.wn = W, trm.get_waveno_arr(W)
        self.idx0, self.npts = _windows(W)
        rng = np.random.default_rng([W, solution])
        tot = int(self.npts.sum())
        nif, star = 10.0 ** rng.uniform(-3, 3, tot), 10.0 ** rng.uniform(2, 8, tot)
        self.gwt = nif * (RPRS * RPRS) / star if solution == 0 else nif     # step_setup's fold, in double
        engine.step_setup(None, 0.0, 1e9, c.abund0, [], self.idx0, self.npts, nif, star, RPRS, solution=solution,
                          pttype=1)
        # walkers of different brightness: their energy outputs lie far apart
        self.spec = 10.0 ** rng.uniform(-3, 3, (4, W)) * np.array([1.0, 0.25, 4.0, 16.0])[:, None]
        self.d_spec = torch.from_numpy(self.spec).cuda()
        self.ref = _exact_bands(self.spec, self.wn, self.idx0, self.npts, self.gwt)
        self.e_out = np.array([math.fsum(_trapz_terms(s, self.wn)) for s in self.spec]) * E_FAC

    def run(self, status):
        """-> (band, status) of step_bandflux and of step_bandflux_blocks on three ranks' blocks."""
        from test_gpu_step_blocks import _slots
        torch, engine, trm = self.torch, self.engine, self.trm
        nf, out = len(self.idx0), []
        st = torch.tensor(status, dtype=torch.int32, device="cuda")
        band = torch.full((4, nf), float("nan"), dtype=torch.float64, device="cuda")
        trm.check(trm.lib().bartrt_step_bandflux_dev(
            C.c_void_p(self.d_spec.data_ptr()), 4, C.c_void_p(st.data_ptr()), C.c_void_p(band.data_ptr()),
            engine._stream_ptr()))
        st3 = torch.tensor(status, dtype=torch.int32, device="cuda")
        band3 = engine.step_bandflux_blocks_dev(_slots(self.d_spec, 3), 3, st3, nf)
        torch.cuda.synchronize()
        return (band, st), (band3, st3)


@pytest.mark.parametrize("solution", [0, 2])
@pytest.mark.parametrize("W", [1025, 2049, 2050, 4100])
def test_band_integration_against_the_exact_sum(tmp_path, W, solution):
    """rtol 1e-13 (test_bandflux_matches_reference_golden's): the kernel adds n positive terms in (n / 256 + 8)
    roundings per lane and tree level, about 5e-15 at n = 4100.  Measured on an MI355X: 2.2e-16 at the most, on every grid (one unit in the last place)."""
    bc = BandCase(tmp_path, W, solution)
    try:
        (band, st), (band3, st3) = bc.run([0, 1, 2, 3])
        got = band.cpu().numpy()
        good = [0, 3]                                   # an incoming 3 is evaluated like a 0
        nz = bc.ref[good] > 0
        dev = np.abs(got[good][nz] / bc.ref[good][nz] - 1.0).max()
        print("W %d solution %d: %d windows, largest deviation from the exact sum %.3g" % (W, solution, len(bc.idx0), dev))
        assert np.all(got[1] == -1.0) and np.all(got[2] == -1.0)
        assert st.cpu().tolist()[1:3] == [1, 2]
        np.testing.assert_allclose(got[good], bc.ref[good], rtol=1e-13, atol=0.0)
        assert np.all(got[good][:, bc.npts < 2] == 0.0)     # no trapezoid: exactly zero
        assert bc.torch.equal(band3, band) and bc.torch.equal(st3, st)
    finally:
        bc.trm.free_memory()


@pytest.mark.parametrize("W", [2049, 2050, 4100])
def test_energy_balance_threshold(tmp_path, W):
    """E = fsum(trapezoid terms) * e_fac per walker.  With e_in a factor 1 + 1e-12 above walker k's E that walker and
    every dimmer one pass (status 0, the band fluxes of the exact sum), the brighter ones are rejected (status 3, rows of
    -1.0); a factor 1 - 1e-12 below it, walker k is rejected too.  1e-12 is 200 times the summation error bound."""
    bc = BandCase(tmp_path, W, 0)
    try:
        E = bc.e_out
        assert np.all(np.abs(E[:, None] / E[None, :] - 1.0)[~np.eye(4, dtype=bool)] > 0.5)
        for k in range(4):
            for fac, k_passes in ((1.0 + 1e-12, True), (1.0 - 1e-12, False)):
                e_in = E[k] * fac
                want = np.where(E > e_in, 3, 0)
                assert want[k] == (0 if k_passes else 3)
                bc.engine.step_set_ebalance(True, e_in, E_FAC)
                for name, (band, st) in zip(("full", "blocks"), bc.run([0, 0, 0, 0])):
                    got, status = band.cpu().numpy(), st.cpu().numpy()
                    assert list(status) == list(want), (name, W, k, fac, list(status), list(want))
                    assert np.all(got[want == 3] == -1.0)
                    np.testing.assert_allclose(got[want == 0], bc.ref[want == 0], rtol=1e-13, atol=0.0)
    finally:
        bc.trm.free_memory()


# ---- 3d: profiles ------------------------------------------------------------------------------------------------------
# 5 layers is the smallest column tried: engine.init accepts it
LAYERS = (5, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320)
MODELS = (("madhu_noinv", 2, "noinv"), ("madhu_inv", 3, "inv"), ("adiabatic", 4, "adiab"), ("piette", 5, "piette"))
# two adiabats whose pole lies below the grid (the golden draws put it near 17 bar: rejected for T < 0)
ADIABATS = np.array([[1500.0, 1.3, 2.0], [900.0, 1.15, 2.5]])


def _piette_nodes_distinct(press_bar_atm):
    p = np.asarray(press_bar_atm)[::-1]
    ii = [int(np.argmin(p))] + [int(np.argmin(np.abs(p - v))) for v in (0.01, 0.1, 1, 3.2, 10, 32)] + [int(np.argmax(p))]
    return len(set(ii)) == 8


def _profiles_dev(params, nspecies):
    import torch
    from bart_amd import engine
    prof, st = engine.step_profiles_dev(torch.from_numpy(np.ascontiguousarray(params)).cuda())
    torch.cuda.synchronize()
    return prof.cpu().numpy().reshape(len(params), nspecies + 1, -1), st.cpu().numpy()


def _compare(params, prof, st, c, molfit, ptargs, tmin=0.0, tmax=1e9, **kw):
    """Device profiles and statuses of every parameter vector against pyhalf.step_profiles -> accepted count."""
    from oracle import pyhalf
    nok = 0
    for w in range(len(params)):
        ref, rst = pyhalf.step_profiles(params[w], c.press_bar, c.abund0, c.species, list(molfit), ptargs, tmin, tmax, **kw)
        assert st[w] == rst, (w, st[w], rst, kw)
        if rst == 0:
            np.testing.assert_allclose(prof[w, 0], ref[0], rtol=1e-12)
            np.testing.assert_allclose(prof[w, 1:], ref[1:], rtol=1e-13)
            nok += 1
    return nok


@pytest.mark.parametrize("L", LAYERS)
def test_profiles_at_layer_count(tmp_path, ptg, L):
    """Every T(p) model at this layer count: the line model (two lanes per layer up to 128 layers, one beyond) with the
    golden parameters and a fitted abundance, with the Thorngren internal temperature, both Madhusudhan models (smoothing
    radius 16: longer than the column at 5 and 16 layers) with the golden draws, statuses of the rejected ones
    included, the adiabat, and Piette where the grid keeps its eight nodes apart (refused where it does not)."""
    from bart_amd import engine, transit_module as trm
    c = _case(tmp_path, nlayers=L)
    S = len(c.species)
    filt = (np.array([0], np.int32), np.array([4], np.int32), np.ones(4), np.ones(4), RPRS)
    args = list(ptg["line_args"])
    engine.init(c.tcfg)
    try:
        assert engine.nlayers() == L
        rng = np.random.default_rng(L)
        line = np.column_stack([ptg["line_params"], rng.uniform(-2, 1, len(ptg["line_params"]))])
        for thorngren in (False, True):
            engine.step_setup(ptg["line_args"], 0.0, 1e9, c.abund0, [c.species.index("CH4")], *filt,
                              tint_thorngren=thorngren)
            prof, st = _profiles_dev(line, S)
            nok = _compare(line, prof, st, c, ["CH4"], args, t_int_type="thorngren" if thorngren else "const")
            assert nok == len(line)
        for pttype, code, key in MODELS:
            params = np.ascontiguousarray(ptg[key + "_params"])
            if key == "adiab":
                params = np.vstack([params, ADIABATS])
            if key == "piette" and not _piette_nodes_distinct(c.press_bar):
                with pytest.raises(trm.TransitError, match="coincide"):
                    engine.step_setup(None, 0.0, 1e9, c.abund0, [], *filt, pttype=code)
                continue
            engine.step_setup(None, 0.0, 1e9, c.abund0, [], *filt, pttype=code)
            prof, st = _profiles_dev(params, S)
            nok = _compare(params, prof, st, c, [], None, pttype=pttype)
            print("L %d %s: %d of %d draws accepted" % (L, pttype, nok, len(params)))
            assert nok > 0
            if key == "noinv":
                assert nok < len(params)
    finally:
        trm.free_memory()


SPECIES16 = ("H2O", "CO", "CO2", "CH4", "N2", "NH3", "H-", "e-", "H", "C2H2", "C2H4", "HCN", "TiO", "VO", "He", "H2")
ABUND16 = (3e-4, 2e-4, 1e-5, 1e-4, 5e-5, 2e-6, 1e-9, 2e-9, 1e-6, 3e-7, 2e-7, 4e-6, 1e-8, 2e-8, 0.15, 0.849)


@pytest.mark.parametrize("L", [65, 129])
def test_sixteen_species_and_sixteen_fitted_molecules(tmp_path, ptg, L):
    """All 16 species of synth.MOLECULES, H- and e- in the middle of the list (not metals), He and H2 last: the metal
    mask is not "everything after the first two".  First the 12 metals fitted, then 16 factors (kMaxMolfit), four
    molecules named twice -- the later factor wins, in the kernel as in the restatement; 17 are refused."""
    from bart_amd import engine, transit_module as trm
    c = _case(tmp_path, nlayers=L, species=SPECIES16, abund=ABUND16)
    metals = [s for s in SPECIES16 if s not in ("H-", "e-", "He", "H2")]
    filt = (np.array([0], np.int32), np.array([4], np.int32), np.ones(4), np.ones(4), RPRS)
    engine.init(c.tcfg)
    try:
        assert engine.species() == list(SPECIES16)
        rng = np.random.default_rng(16 + L)
        for molfit in (metals, metals + ["CO", "H2O", "TiO", "CO"]):
            assert len(molfit) in (12, 16)
            params = np.column_stack([ptg["line_params"][:8], rng.uniform(-1.5, 1.5, (8, len(molfit)))])
            params[7, 5:] = 3.5             # metals above 1 in sum: rejected (2) by both
            engine.step_setup(ptg["line_args"], 0.0, 1e9, c.abund0, [SPECIES16.index(m) for m in molfit], *filt)
            prof, st = _profiles_dev(params, 16)
            assert _compare(params, prof, st, c, molfit, list(ptg["line_args"])) == 7 and st[7] == 2
        with pytest.raises(trm.TransitError, match="16 fitted molecules"):
            engine.step_setup(ptg["line_args"], 0.0, 1e9, c.abund0, [0] * 17, *filt)
    finally:
        trm.free_memory()


def test_temperature_bounds_and_documented_rejections(tmp_path, ptg):
    """The bounds are closed (BARTfunc.py:327 rejects T < tmin, T > tmax): T == tmin and T == tmax are accepted, the
    next double outside either is status 1.  Non-finite parameters (step.hip, step_body): a NaN T(p) parameter is
    status 1; an abundance parameter of 400 (factor inf) or NaN is status 2."""
    from bart_amd import engine, transit_module as trm
    c = _case(tmp_path, nlayers=17)
    S = len(c.species)
    filt = (np.array([0], np.int32), np.array([4], np.int32), np.ones(4), np.ones(4), RPRS)
    tmin, tmax = 400.0, 3000.0
    engine.init(c.tcfg)
    try:
        engine.step_setup(None, tmin, tmax, c.abund0, [], *filt, pttype=1)
        iso = np.array([[tmin], [tmax], [np.nextafter(tmin, 0.0)], [np.nextafter(tmax, np.inf)], [1700.0], [np.nan]])
        prof, st = _profiles_dev(iso, S)
        assert list(st) == [0, 0, 1, 1, 0, 1], list(st)
        assert _compare(iso[:5], prof, st, c, [], None, tmin, tmax, pttype="iso") == 3
        assert np.all(prof[0, 0] == tmin) and np.all(prof[1, 0] == tmax)
        engine.step_setup(ptg["line_args"], tmin, tmax, c.abund0, [c.species.index("CH4")], *filt)
        good = np.array([-2.0, 0.0, 1.0, 0.0, 0.98, -0.5])
        par = np.tile(good, (9, 1))
        for k in range(5):
            par[1 + k, k] = np.nan              # each T(p) parameter in turn
        par[6, 5], par[7, 5] = 400.0, np.nan
        par[8, 5] = -400.0                      # factor 0: nothing wrong with it
        prof, st = _profiles_dev(par, S)
        assert list(st) == [0, 1, 1, 1, 1, 1, 2, 2, 0], list(st)
        assert _compare(par[[0, 8]], prof[[0, 8]], st[[0, 8]], c, ["CH4"], list(ptg["line_args"]), tmin, tmax) == 2
    finally:
        trm.free_memory()


@pytest.mark.parametrize("L", [128, 129, 257])
def test_fused_launch_equals_converter_then_engine(tmp_path, ptg, L):
    """step_batch_dev builds its profiles in step_prep_profiles (LDS to LDS); step_profiles_dev + run_batch_dev builds
    them in step_profiles and prepares them in prep_profiles.  One body each: the statuses are equal, and so are the
    spectra, bit for bit -- which they are only if every profile value is.  (Five walkers: no launch of four or fewer,
    whose RT kernel prepares its own walkers.)"""
    import torch
    from bart_amd import engine, transit_module as trm
    c = _case(tmp_path, nlayers=L, nwave=70)
    idx0, npts = np.array([0, 30], np.int32), np.array([30, 40], np.int32)
    rng = np.random.default_rng(L)
    engine.init(c.tcfg)
    try:
        engine.step_setup(ptg["line_args"], 400.0, 3000.0, c.abund0, [c.species.index("CH4")], idx0, npts,
                          rng.uniform(0.2, 1.0, 70), rng.uniform(1e5, 3e5, 70), RPRS)
        good = np.array([-2.0, 0.0, 1.0, 0.0, 0.98, -0.5])
        par = good + rng.normal(0, [0.3, 0.2, 0.2, 0.0, 0.03, 0.4], (5, 6))
        par[3] = [-1.0, -2.0, -2.0, 0.0, 1.2, -0.5]          # T > tmax deep down: status 1
        d_par = torch.from_numpy(par).cuda()
        prof, st_u = engine.step_profiles_dev(d_par)
        spec_u = engine.run_batch_dev(prof).clone()
        band, st_f, spec_f = engine.step_batch_dev(d_par, 2, want_spec=True)
        torch.cuda.synchronize()
        assert st_u.cpu().tolist() == [0, 0, 0, 1, 0] and torch.equal(st_f, st_u)
        keep = [0, 1, 2, 4]
        assert torch.isfinite(spec_f[keep]).all() and bool((spec_f[keep] > 0).all())
        assert torch.equal(spec_f[keep], spec_u[keep]), (spec_f[keep] - spec_u[keep]).abs().max()
    finally:
        trm.free_memory()


# ---- 3e: columns whose fused launch needs more than 64 kB of LDS ----------------------------------------------------------
def _fused_lds_bytes(L, S, Nt, ncia_temps, npars, nmolfit):
    """8 (prep_lds_doubles + step_lds_doubles), csrc/prep.hpp and csrc/step.hip."""
    prep = 4 * L + (S + 1) * L + 2 * L + S + 2 * Nt + 2 * ncia_temps + 1
    step = L * (3 + S) + npars + 3 + nmolfit + 3
    return 8 * (prep + step)


DEEP = {
    "300 layers, 10 species, eight molecules, two CIA pairs, transit": dict(
        kw=dict(nlayers=300, nwave=40, species=("He", "H2", "CO", "CO2", "CH4", "H2O", "NH3", "HCN", "C2H2", "N2"),
                abund=(0.15, 0.85) + (1e-4,) * 8, opmol=("CO", "CO2", "CH4", "H2O", "NH3", "HCN", "C2H2", "N2"), cia=2,
                tempdelt=100.0, extra_keys={"solution": "transit", "starrad": 1.145}),
        solution=1, lds=(27, 14)),
    "200 layers, 16 species, eclipse": dict(
        kw=dict(nlayers=200, nwave=40, species=SPECIES16, abund=ABUND16), solution=0, lds=(5, 0)),
}


@pytest.mark.parametrize("name", list(DEEP))
def test_fused_launch_above_64_kb_of_lds(tmp_path, ptg, name):
    """Three walkers through engine.step_batch (one fused launch: T(p), abundances and preparation of a column that
    needs 72.9 kB resp. 67.5 kB of LDS) against the oracle chain pyhalf.step_profiles -> OracleEngine.run ->
    pyhalf.bandflux at rtol 1e-9 (test_full_step_against_oracle_chain's); then one walker through run_transit.  An RT
    kernel folds the preparation into its prologue only while both jobs fit the 64 kB default (lp_geom; the transit
    geometry never folds), so on these columns run_transit reaches the stand-alone prep_profiles launch.  The three
    converters are opted into more than 64 kB (csrc/lds.hpp), as HIP documents; a build without the opt-in passed this
    test on an MI355X too (MEASUREMENTS.md): the runtime did not refuse these launches."""
    from bart_amd import engine, transit_module as trm
    from oracle import pyhalf, rt_oracle as orc
    d = DEEP[name]
    c = _case(tmp_path, **d["kw"])
    L, S = len(c.press_bar), len(c.species)
    need = _fused_lds_bytes(L, S, d["lds"][0], d["lds"][1], 6, 1)
    print("%s: the fused launch asks for %d bytes of LDS" % (name, need))
    assert 64 * 1024 < need <= 160 * 1024
    idx0, npts = np.array([0, 11, 25], np.int32), np.array([12, 14, 15], np.int32)
    rng = np.random.default_rng(L)
    nif, star = rng.uniform(0.2, 1.0, 41), rng.uniform(1e5, 3e5, 41)
    params = np.array([[-2.0, 0.0, 1.0, 0.0, 0.98, -0.5],
                       [-2.3, -0.4, 0.6, 0.3, 0.9, 0.4],
                       [-1.8, 0.2, 0.1, 0.7, 1.0, -1.7]])
    engine.init(c.tcfg)
    try:
        engine.step_setup(ptg["line_args"], 400.0, 3000.0, c.abund0, [c.species.index("CH4")], idx0, npts, nif, star,
                          RPRS, solution=d["solution"])
        band, status = engine.step_batch(params, 3)
        assert list(status) == [0, 0, 0]
        o = orc.OracleEngine(c.tcfg)
        for w in range(3):
            prof, st = pyhalf.step_profiles(params[w], c.press_bar, c.abund0, c.species, ["CH4"],
                                            list(ptg["line_args"]), 400.0, 3000.0)
            assert st == 0
            spec = o.run(prof)
            ref = pyhalf.bandflux(spec, o.wn, idx0, npts, nif, star, RPRS,
                                  solution="eclipse" if d["solution"] == 0 else "transit")
            np.testing.assert_allclose(band[w], ref, rtol=1e-9)
            if w == 0:
                np.testing.assert_allclose(trm.run_transit(prof.ravel(), len(spec)), spec, rtol=1e-9)
    finally:
        trm.free_memory()


def test_prefetch_on_a_column_whose_preparation_passes_64_kb(tmp_path):
    """360 layers x 16 species on an eclipse engine: the preparation alone needs 66 456 bytes of LDS.  An RT launch
    that carried the next batch's preparation would ask for at least that much, and the RT kernels are not opted in
    above 64 kB: the engine drops the prefetch on such a column (Engine::plan_prefetch) and the named batch is prepared
    by its own call.  The spectra are the bits of the calls without a prefetch, and within 1e-9 of the oracle's."""
    import torch
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    c = _case(tmp_path, nlayers=360, nwave=40, species=SPECIES16, abund=ABUND16)
    L, S, Nt = 360, 16, 5
    assert len(c.tgrid) == Nt
    need = 8 * (4 * L + (S + 1) * L + 2 * L + S + 2 * Nt + 1)      # csrc/prep.hpp, prep_lds_doubles; no CIA
    print("the preparation asks for %d bytes of LDS" % need)
    assert 64 * 1024 < need <= 160 * 1024
    rng = np.random.default_rng(360)
    temps = np.clip(c.temp0 + rng.uniform(-300, 600, (10, 1)), 410.0, 2990.0)
    prof = torch.from_numpy(np.stack([c.profiles(t).ravel() for t in temps]).reshape(2, 5, -1)).cuda()
    engine.init(c.tcfg)
    try:
        ref = [engine.run_batch_dev(prof[k]).clone() for k in range(2)]
        for i in range(3):              # every call names the next batch
            out = engine.run_batch_dev(prof[i % 2], next_prof=prof[(i + 1) % 2])
            assert torch.equal(out, ref[i % 2]), i
        assert torch.equal(engine.run_batch_dev(prof[1]), ref[1])
        np.testing.assert_allclose(ref[1][0].cpu().numpy(), orc.OracleEngine(c.tcfg).run(c.profiles(temps[5])), rtol=1e-9)
    finally:
        trm.free_memory()


# ---- 3f: Piette on a grid where two nodes coincide --------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(nlayers=100, pbottom=10.0), dict(nlayers=12)], ids=["bottom_at_10_bar", "12_layers"])
def test_piette_refused_when_nodes_coincide(tmp_path, kw):
    """A bottom pressure below 32 bar, or a coarse grid, puts two of the model's eight pressure nodes on one layer.  The
    reference's spline fit then yields NaN for the layers above the doubled node -- every layer when that node is the
    bottom (oracle/pyhalf.py says the same) -- and its bounds check lets the NaN through; step_setup refuses the model
    on such a grid and names the nodes."""
    from bart_amd import engine, transit_module as trm
    from oracle import pyhalf
    c = _case(tmp_path, **kw)
    assert not _piette_nodes_distinct(c.press_bar)
    par = np.load(os.path.join(G, "pt_golden.npz"))["piette_params"][0]
    with np.errstate(all="ignore"):
        ref = pyhalf.pt_piette(c.press_bar[::-1], *par)
    assert np.isnan(ref).sum() >= len(ref) - 2
    filt = (np.array([0], np.int32), np.array([4], np.int32), np.ones(4), np.ones(4), RPRS)
    engine.init(c.tcfg)
    try:
        with pytest.raises(trm.TransitError, match="nodes coincide.*layer"):
            engine.step_setup(None, 0.0, 1e9, c.abund0, [], *filt, pttype=5)
        engine.step_setup(None, 0.0, 1e9, c.abund0, [], *filt, pttype=4)     # the other models take the grid
    finally:
        trm.free_memory()
