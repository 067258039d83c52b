"""GPU: the layer preparation (csrc/prep.hpp, prep_body) at its edges, against tests/prep_restate.py (mpmath, 50
digits; held to the C oracle on these same cases by tests/test_prep_restate_cpu.py) -- radii through
bartrt_get_radius, the layer records through bartrt_get_prep_records, spectra against the oracle at RTOL.

The one body is driven down four paths, named in every printed line:
  (a) folded ....... one walker, eclipse: the layer-parallel RT kernel prepares its own walker (PrepFold)
  (b) stand-alone .. six walkers: the prep_profiles launch
  (c) fused step ... step_setup / step_batch with the isothermal model: step_prep_profiles
  (d) transit ...... solution transit, three walkers: prep_profiles + the chord table

Bounds (EPS = 2^-52; every rounding is at most EPS / 2 relative, the count is doubled for the compounding and the
reference's own rounding to double) -- roundings counted in prep_body:
  radii, paths .... four times the deviation of the C oracle's plain-double radii (radius differences) from the
                    restatement on the same case, with a floor of 8 ulp of the value (the device's r +- H r^2
                    recurrence with FMA is algebraically the oracle's, rounded differently)
  c2 / T .......... 4: the constant (2), 1 / T, the product
  table weights ... 12: nd = p (1 / T) (1 / kB) (4), rho = q m amu nd (3), f = (T - g_j) (1 / dg) (3), 1 - f, the
                    product.  RELATIVE on rho f; on rho (1 - f), which cancels next to the upper node, 3 EPS rho |f|
                    ABSOLUTE besides (_pair_bounds); planes outside the bracket are zero exactly
  CIA weights ..... 20: n1, n2 (7 each), their product, fc (3), 1 - fc, the product; split the same way.
                    Curvature terms: 40 against n1 n2 h^2 / 6 with h the layer's own bracket (s6: 20; a^3 - a: 19
                    absolute, |a^3 - a| < 0.385)
  Rayleigh ........ 16: flag 1 pow (2), sigma0, q, nd (5), lambda0^4 (4); flag 2 a few less
  grey ............ 4 relative, plus the ramp's slope times the radius bound
Figures are printed before they are asserted (run with -s); the worst measured ones are in MEASUREMENTS.md."""
import numpy as np
import pytest

import prep_cases as pc
import prep_restate as pr

pytestmark = pytest.mark.gpu
RTOL = 1e-10
EPS = 2.0 ** -52
RPRS = 0.11
T_ISO = 1234.5
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_figures():
    """After the module: the largest figure of each quantity over its tests (what MEASUREMENTS.md records)."""
    yield
    for k, v in sorted(WORST.items()):
        print("worst %s: %.3g" % (k, v))


def _note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


def _oracle(case):
    from oracle import rt_oracle as orc
    return orc.OracleEngine(case.tcfg)


def _rad_bounds(o, r, prof):
    """(radius bound [L], path bound [L], the oracle's own worst deviation of either) of one profile: 4 x the oracle's
    deviation from the restatement on this case, floor 8 ulp of the value."""
    rad_o = o.extinction(prof)[1]
    path_o = np.append(np.diff(rad_o), 0.0)
    d_r, d_p = pr.absdev(rad_o, r["radius"]).max(), pr.absdev(path_o, r["path"]).max()
    return (np.maximum(4.0 * d_r, 8.0 * pr.ulp(pr.mag(r["radius"]))), np.maximum(4.0 * d_p, 8.0 * pr.ulp(pr.mag(r["path"]))),
            d_r, d_p)


def check_radii(label, rad, o, r, prof):
    rb, _, d_r, _ = _rad_bounds(o, r, prof)
    dev = pr.absdev(rad, r["radius"])
    print("%s: radii off the restatement by %.3g cm (%.2f ulp) at the most; the oracle by %.3g cm; bound %.3g cm"
          % (label, dev.max(), (dev / pr.ulp(rad)).max(), d_r, rb.min()))
    _note("radius [ulp]", (dev / pr.ulp(rad)).max())
    assert np.all(dev <= rb), (label, dev, rb)


def _pair_bounds(ref, grid, t, scale, n):
    """Bounds [L][planes] of a layer's dense pair of linear weights s (1 - f) on plane j and s f on plane j + 1
    (s = `scale` [L]: rho, or n1 n2; t [L] the temperature the bracket is taken at; n: the roundings of either weight):
      plane j + 1 .. RELATIVE, n EPS of the weight: f = (t - g_j) (1 / dg) carries three relative roundings whatever
                     its size (next to the node the subtraction is exact);
      plane j ...... n EPS of the weight, plus 3 EPS s |f|: 1 - f inherits f's ABSOLUTE error, which is all that is
                     left of it where 1 - f cancels;
      t on node j .. may sit as f = 1 on plane j - 1 as well (the dense form makes the two the same): plane j - 1 is
                     then allowed the cancelled 3 EPS s;
      elsewhere .... zero, exactly.
    A single-temperature table has the one weight s: n EPS, relative."""
    ref = pr.mag(ref)
    B = np.zeros(ref.shape)
    grid = np.asarray(grid, float)
    for l in range(ref.shape[0]):
        if len(grid) == 1:
            B[l, 0] = n * EPS * ref[l, 0]
            continue
        j = pr.bracket(list(grid), t[l])
        f = (t[l] - grid[j]) / (grid[j + 1] - grid[j])
        B[l, j] = n * EPS * ref[l, j] + 3 * EPS * scale[l] * abs(f)
        B[l, j + 1] = n * EPS * ref[l, j + 1]
        if f == 0.0 and j > 0:
            B[l, j - 1] = 3 * EPS * scale[l]
    return B


def check_records(label, su, o, r, prof, rec, W):
    """One walker's records (coef, idx, kstop, ok) in the dense form against the restatement r: every figure is
    worked out and printed first, then asserted."""
    coef, idx, kstop, ok = rec
    L = len(su.press)
    assert ok == 1 and kstop == r["kstop"], (label, ok, kstop, r["kstop"])
    assert coef[0, 0] == 0.0                       # the top layer's path length, exactly
    d = pr.expand_records(su, coef, idx, W)
    rb, pb, d_r, d_p = _rad_bounds(o, r, prof)
    T = np.asarray(prof, float).reshape(len(su.mass) + 1, L)[0]
    fig, held = {}, []                             # held: (name, deviation, bound), asserted after the print

    def hold(name, unit, dev, bound, per):
        """per: what the printed figure is a multiple of (0 where the bound is 0: the deviation must be 0 too)."""
        nz = per > 0
        fig["%s [%s]" % (name, unit)] = max(fig.get("%s [%s]" % (name, unit), 0.0), float((dev[nz] / per[nz]).max()) if nz.any() else 0.0)
        held.append((name, dev, bound))

    dev = pr.absdev(d["path"], r["path"])
    hold("path", "cm", dev, pb, np.ones(L))
    hold("c2/T", "EPS", pr.absdev(d["c2T"], r["c2T"]), 4 * EPS * pr.mag(r["c2T"]), EPS * pr.mag(r["c2T"]))
    if su.opmol:
        for m in range(len(su.opmol)):
            B = _pair_bounds(r["table_weight"][:, :, m], su.tgrid, T, pr.mag(r["rho"][:, m]), 12)
            hold("table weight", "of its bound", pr.absdev(d["table_weight"][:, :, m], r["table_weight"][:, :, m]), B, B)
    for cc, (s1, s2, temps, kind) in enumerate(su.cia):
        temps = np.asarray(temps, float)
        nn = pr.mag(r["cia_scale"][:, cc])
        Tc = np.clip(T, temps[0], temps[-1])
        dev = pr.absdev(d["cia_weight"][cc], r["cia_weight"][cc])
        if kind == 0:
            B = _pair_bounds(r["cia_weight"][cc], temps, Tc, nn, 20)
            hold("CIA weight", "of its bound", dev, B, B)
            continue
        if len(temps) == 1:
            assert np.all(d["cia_weight"][cc] == 0.0)
            continue
        # curvature terms: against the layer's OWN bracket's n1 n2 h^2 / 6, on the bracket's two planes (either
        # factor, a^3 - a and f^3 - f, cancels next to a node); zero elsewhere
        jc = np.array([pr.bracket(list(temps), t) for t in Tc])
        s6 = nn * (temps[jc + 1] - temps[jc]) ** 2 / 6.0
        B = np.zeros(dev.shape)
        B[np.arange(L), jc] = B[np.arange(L), jc + 1] = 40 * EPS * s6
        hold("CIA curvature weight", "EPS n1 n2 h^2/6, h the layer's own bracket", dev, B, B / 40)
    ray = pr.mag(r["rayleigh"])
    hold("Rayleigh", "EPS", pr.absdev(d["rayleigh"], r["rayleigh"]), 16 * EPS * ray, EPS * ray)
    slope = su.cloud_ext / (su.cloud_rup - su.cloud_rdown) if su.cloud_ext > 0 else 0.0
    hold("grey", "of cloudext", pr.absdev(d["grey"], r["grey"]), 4 * EPS * pr.mag(r["grey"]) + slope * rb,
         np.full(L, su.cloud_ext))
    print("%s: records off the restatement by " % label + ", ".join("%s %.3g" % kv for kv in fig.items())
          + "; the oracle's own radius differences by %.3g cm, path bound %.3g cm" % (d_p, pb.min()))
    for k, v in fig.items():
        _note(k, v)
    for name, dev, bound in held:
        assert np.all(dev <= bound), (label, name, dev, bound)
    return d


def check_spectra(label, got, o, profs):
    ref = np.array([o.run(p) for p in profs])
    err = np.max(np.abs(got / ref - 1.0))
    print("%s: spectra off the oracle by %.3g" % (label, err))
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0.0)


def _step_setup(engine, c, W, solution=0):
    engine.step_setup(None, 0.0, 1e9, c.abund0, [], np.array([0], np.int32), np.array([4], np.int32), np.ones(4),
                      np.ones(4), RPRS, solution=solution, pttype=1)


# ---- the reference layer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,L,k,variant", pc.REF_CASES, ids=[c[0] for c in pc.REF_CASES])
def test_reference_layer_down_four_paths(tmp_path, label, L, k, variant):
    """refpress on, next to, below and above the layers (prep_cases.REF_CASES): both walks of the hydrostatic chain at
    every length between empty and two blocks plus remainder.  The engine accepts a reference pressure outside the
    grid (the closest layer's own T and mu stand in for the interpolated ones)."""
    import torch
    from bart_amd import engine, transit_module as trm
    c = pc.ref_case(tmp_path / "e", L, k, variant)
    o = _oracle(c)
    su = pr.setup_from_oracle(o)
    W = len(c.wn)
    profs = pc.profiles(c, 6, seed=L + (k or 0))
    engine.init(c.tcfg)
    try:
        # walker 0 of every path is the isothermal model's own profile, as the per-step kernels build it (the T(p)
        # models are held by test_gpu_step_edges.py; here their output is an input): T_ISO on every layer, the
        # atmosphere file's abundances with He and H2 filling the rest
        _step_setup(engine, c, W)
        par = torch.tensor([[T_ISO], [T_ISO + 300.0]], dtype=torch.float64, device="cuda")
        prof_c, st = engine.step_profiles_dev(par)
        profs[0] = prof_c[0].cpu().numpy()
        assert st.cpu().tolist() == [0, 0] and np.all(profs[0][:L] == T_ISO)
        np.testing.assert_allclose(profs[0], pc.iso_profile(c, T_ISO), rtol=1e-3)
        rs = [pr.restate(su, p) for p in profs]
        assert rs[0]["ref_exact"] == (variant == "on")
        # (a) folded
        engine.walked_begin()
        spec_a = engine.run_batch(profs[:1])
        name = engine.walked_end()[2]
        print("%s path (a): %s" % (label, name))
        assert "prepares its own walkers" in name, name
        with pytest.raises(trm.TransitError, match="inside the RT kernel"):
            engine.prep_records(0)
        rad_a = engine.get_radius()
        check_radii(label + " (a) folded", rad_a, o, rs[0], profs[0])
        check_spectra(label + " (a) folded", spec_a, o, profs[:1])
        assert (rad_a[rs[0]["ref_idx"]] == su.refradius) == (variant == "on")      # the exact branch, or not
        # (b) stand-alone
        engine.walked_begin()
        spec_b = engine.run_batch(profs)
        name = engine.walked_end()[2]
        print("%s path (b): prep_profiles + %s" % (label, name))
        assert "prepares its own walkers" not in name
        rad_b = engine.get_radius()
        check_radii(label + " (b) stand-alone", rad_b, o, rs[0], profs[0])
        recs_b = [engine.prep_records(w) for w in range(6)]
        for w in range(6):
            check_records("%s (b) stand-alone walker %d" % (label, w), su, o, rs[w], profs[w], recs_b[w], W)
        check_spectra(label + " (b) stand-alone", spec_b, o, profs)
        with pytest.raises(trm.TransitError, match="outside the latest batch"):
            engine.prep_records(6)
        with pytest.raises(trm.TransitError, match="outside the latest batch"):
            engine.prep_records(-1)
        # (c) the fused step launch, isothermal: the profile is profs[0] exactly
        engine.walked_begin()
        band, st, spec_c = engine.step_batch_dev(par, 1, want_spec=True)
        torch.cuda.synchronize()
        name = engine.walked_end()[2]
        # (the fused launch -- step_prep_profiles as run_chunk's preparation hook -- is taken where the column's T(p) and
        # preparation halves fit a workgroup's LDS together, as they do at these shapes; the fallback, two launches,
        # would let a two-walker RT kernel prepare its own walkers: its name would say so, and the assertion below and
        # prep_records(0) would fail rather than pass on another path)
        print("%s path (c): the step launch's preparation + %s, two walkers" % (label, name))
        assert "prepares its own walkers" not in name, name
        rad_c = engine.get_radius()
        rec_c = engine.prep_records(0)
        check_records(label + " (c) fused step", su, o, rs[0], profs[0], rec_c, W)
        check_spectra(label + " (c) fused step", spec_c.cpu().numpy()[:1], o, profs[:1])
        # one body: one set of bits
        assert np.array_equal(rad_a, rad_b) and np.array_equal(rad_b, rad_c)
        assert np.array_equal(rec_c[0], recs_b[0][0]) and np.array_equal(rec_c[1], recs_b[0][1])
        assert np.array_equal(spec_a[0], spec_b[0])
    finally:
        trm.free_memory()
    # (d) transit geometry
    ct = pc.ref_case(tmp_path / "t", L, k, variant, extra_keys={"solution": "transit", "starrad": 1.0})
    ot = _oracle(ct)
    engine.init(ct.tcfg)
    try:
        engine.walked_begin()
        spec_d = engine.run_batch(profs[:3])
        print("%s path (d): prep_profiles + chord table + %s" % (label, engine.walked_end()[2]))
        rad_d = engine.get_radius()
        check_radii(label + " (d) transit", rad_d, ot, rs[0], profs[0])
        for w in range(3):
            check_records("%s (d) transit walker %d" % (label, w), su, ot, rs[w], profs[w], engine.prep_records(w), W)
        check_spectra(label + " (d) transit", spec_d, ot, profs[:3])
        assert np.array_equal(rad_d, rad_b)
    finally:
        trm.free_memory()


# ---- temperature edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["linear", "spline"])
def test_temperature_edges(tmp_path, interp):
    """Four molecules on the 100 K grid, two cross-section files on uneven grids: every layer on a node, on the first
    and the last node, one ulp either side of three nodes, a ramp beyond both ends (f < 0, f > 1; the cross sections
    clamp), and the cross sections' own nodes.  Path (b), six walkers."""
    from bart_amd import engine, transit_module as trm
    c = pc.temp_edge_case(tmp_path, extra_keys={"cia_interp": interp})
    o = _oracle(c)
    su = pr.setup_from_oracle(o)
    over = pc.ramp_overshoot(c, o)
    named = pc.temp_edge_profiles(c, over)
    profs = np.array(list(named.values()))
    engine.init(c.tcfg)
    try:
        spec = engine.run_batch(profs)
        for w, name in enumerate(named):
            r = pr.restate(su, profs[w])
            check_records("temperature edges %s (b) %s" % (interp, name), su, o, r, profs[w], engine.prep_records(w), len(c.wn))
        check_spectra("temperature edges %s (b), overshoot %g K" % (interp, over), spec, o, profs)
    finally:
        trm.free_memory()


# ---- single-temperature cross sections -----------------------------------------------------------------------------
@pytest.mark.parametrize("which,interp,solution", pc.SINGLE_CASES, ids=["-".join(c) for c in pc.SINGLE_CASES])
def test_single_temperature_cross_sections(tmp_path, which, interp, solution):
    """nt == 1: jc = 0, fc = 0, one pair plane holding the file's values twice.  The engine accepts such a file under
    `cia_interp spline` too (its curvature table is all zeros).  Six walkers, path (b) / (d)."""
    from bart_amd import engine, transit_module as trm
    c = pc.single_temp_case(tmp_path / "a", which, interp, solution)
    o = _oracle(c)
    su = pr.setup_from_oracle(o)
    profs = pc.profiles(c, 6, seed=5)
    engine.init(c.tcfg)
    try:
        spec = engine.run_batch(profs)
        for w in range(6):
            r = pr.restate(su, profs[w])
            d = check_records("single temperature %s %s %s walker %d" % (which, interp, solution, w), su, o, r, profs[w],
                              engine.prep_records(w), len(c.wn))
            assert np.all(d["cia_weight"][0] > 0.0)
        check_spectra("single temperature %s %s %s" % (which, interp, solution), spec, o, profs)
    finally:
        trm.free_memory()
    bare = pc.single_temp_case(tmp_path / "b", which, interp, solution, with_file=False)
    engine.init(bare.tcfg)
    try:
        moved = np.max(np.abs(spec / engine.run_batch(profs) - 1.0), axis=1)
        print("the single-temperature file moves the spectra by", moved)
        assert np.all(moved > 1e-4)
    finally:
        trm.free_memory()


# ---- small terms ---------------------------------------------------------------------------------------------------------
SPECIES = {"He-H2": (("He", "H2", "CO", "CO2", "CH4", "H2O"), (0.15, 0.85, 1e-4, 1e-4, 1e-4, 1e-4)),
           "no-He": (("H2", "CO", "CH4", "H2O"), (0.9997, 1e-4, 1e-4, 1e-4)),
           "no-H2": (("He", "CO", "CH4", "H2O"), (0.9997, 1e-4, 1e-4, 1e-4))}


@pytest.mark.parametrize("which", list(SPECIES))
def test_rayleigh_records(tmp_path, which):
    """Both flags, H2 or He absent, and a per-walker scattering value (the fused step launch's override)."""
    import torch
    from bart_amd import engine, transit_module as trm
    species, abund = SPECIES[which]
    c = pc.ref_case(tmp_path, 24, 9, "off", species=species, abund=abund)
    o = _oracle(c)
    profs = pc.profiles(c, 6, seed=7)
    engine.init(c.tcfg)
    try:
        for flag in (1, 2):
            trm.set_scattering(flag, -1.5)
            o.set_scattering(flag, -1.5)
            su = pr.setup_from_oracle(o)
            spec = engine.run_batch(profs)
            for w in (0, 5):
                r = pr.restate(su, profs[w])
                d = check_records("Rayleigh %s flag %d (b) walker %d" % (which, flag, w), su, o, r, profs[w],
                                  engine.prep_records(w), len(c.wn))
                assert np.all(d["rayleigh"] > 0.0) == ((flag == 1 and "H2" in species) or flag == 2)
            check_spectra("Rayleigh %s flag %d (b)" % (which, flag), spec, o, profs)
        if which != "He-H2":
            return          # (the per-step converters keep the He / H2 ratio: they need both)
        # per-walker values: parameters (T, scattering) of the isothermal model
        trm.set_scattering(1, -1.5)
        o.set_scattering(1, -1.5)
        su = pr.setup_from_oracle(o)
        _step_setup(engine, c, len(c.wn))
        engine.step_set_extras(0, 0, 1)
        vals = pc.OWN_SCATTERING
        par = torch.tensor([[T_ISO, v] for v in vals], dtype=torch.float64, device="cuda")
        iso = engine.step_profiles_dev(par)[0][0].cpu().numpy()     # (the same for the three: T_ISO, the file's abundances)
        assert np.all(iso[:24] == T_ISO)
        engine.step_batch_dev(par, 1)
        torch.cuda.synchronize()
        for w, v in enumerate(vals):
            r = pr.restate(su, iso, scat_value=v)
            check_records("Rayleigh %s (c) fused step, walker's own value %g" % (which, v), su, o, r, iso,
                          engine.prep_records(w), len(c.wn))
    finally:
        trm.free_memory()


def test_grey_ramp_on_its_ends(tmp_path):
    """cloudrad's two radii are the restated radii of layers 15 and 6 of one walker, written with 17 digits: that
    walker's layer 15 sits on the ramp's upper end (grey 0 at and above it), layer 6 on its lower end (cloudext at and
    below it) -- to within the radius bound, which the grey bound carries as slope x bound."""
    from bart_amd import engine, transit_module as trm
    c0 = pc.ref_case(tmp_path / "bare", 24, 9, "off")
    o0 = _oracle(c0)
    profs = pc.profiles(c0, 6, seed=8)
    rad = [float(x) for x in pr.restate(pr.setup_from_oracle(o0), profs[1])["radius"]]
    c = pc.ref_case(tmp_path / "cloud", 24, 9, "off",
                    extra_keys={"cloudrad": "%.17g %.17g" % (rad[15], rad[6]), "cloudfct": "1.0", "cloudext": "3e-9"})
    o = _oracle(c)
    su = pr.setup_from_oracle(o)
    assert su.cloud_rup == rad[15] and su.cloud_rdown == rad[6] and su.cloud_ext == 3e-9
    engine.init(c.tcfg)
    try:
        spec = engine.run_batch(profs)
        for w in range(6):
            r = pr.restate(su, profs[w])
            d = check_records("grey ramp (b) walker %d" % w, su, o, r, profs[w], engine.prep_records(w), len(c.wn))
            if w == 1:
                g = d["grey"]
                assert np.all(g[:6] == 3e-9) and np.all(g[16:] == 0.0) and np.all((g[7:15] > 0) & (g[7:15] < 3e-9))
                assert g[15] <= 3e-9 * 1e-12 and g[6] >= 3e-9 * (1 - 1e-12)
        check_spectra("grey ramp (b)", spec, o, profs)
    finally:
        trm.free_memory()


def test_stop_layer(tmp_path):
    """cloudtop on a layer's pressure exactly (the deck is that layer: the test is >=), the next value below it that a
    logarithm in the cfg reaches (still that layer), above the top layer (the deck is the top layer) and below the
    bottom (no deck: the column ends on its last layer)."""
    from bart_amd import engine, transit_module as trm
    c0 = pc.ref_case(tmp_path / "bare", 24, 9, "off")
    press = _oracle(c0).press
    l, v_below, cases = pc.stop_layer_cases(press)
    profs = pc.profiles(c0, 6, seed=9)
    for name, x, want in cases:
        c = pc.ref_case(tmp_path / name.replace(" ", "-"), 24, 9, "off", extra_keys={"cloudtop": repr(x)})
        o = _oracle(c)
        su = pr.setup_from_oracle(o)
        if name == "on the layer":
            assert su.cloudtop == press[l]
        if name == "just below it":
            assert su.cloudtop == v_below < press[l] and su.cloudtop > press[l + 1]
        engine.init(c.tcfg)
        try:
            spec = engine.run_batch(profs)
            for w in (0, 3):
                r = pr.restate(su, profs[w])
                assert r["kstop"] == want
                check_records("cloud top %s (b) walker %d" % (name, w), su, o, r, profs[w], engine.prep_records(w), len(c.wn))
            check_spectra("cloud top %s (b)" % name, spec, o, profs)
        finally:
            trm.free_memory()


# ---- the bad flag --------------------------------------------------------------------------------------------------------
def test_bad_flag(tmp_path):
    """A batch of eight: walker 0 plain, then one layer's T = 0, -1, inf, 1e30 (rejected: the test is < 1e30), 9.9e29
    (accepted by the flag), a NaN abundance in the last layer only, a mean mass of exactly 0 in one layer.  Every such
    value is inside what prep_body tests for."""
    from bart_amd import engine, transit_module as trm
    c = pc.ref_case(tmp_path, 24, 9, "off")
    o = _oracle(c)
    su = pr.setup_from_oracle(o)
    L, S, W = 24, len(c.species), len(c.wn)
    good = pc.profiles(c, 8, seed=10)
    batch = good.copy().reshape(8, S + 1, L)
    for w, T in zip((1, 2, 3, 4, 5), (0.0, -1.0, np.inf, 1e30, 9.9e29)):
        batch[w, 0, 5 + w] = T
    batch[6, S, L - 1] = np.nan
    batch[7, 1:, 11] = 0.0
    batch = batch.reshape(8, -1)
    want = [int(pr.is_ok(su, p)) for p in batch]
    assert want == [1, 0, 0, 0, 0, 1, 0, 0]
    engine.init(c.tcfg)
    try:
        spec, ok = engine.run_batch(batch, want_ok=True)
        assert ok.tolist() == want
        recs = [engine.prep_records(w) for w in range(8)]
        for w in range(8):
            coef, idx, kstop, okw = recs[w]
            assert okw == want[w] and kstop == L - 1      # (no cloud: the stop layer does not depend on the flag)
            if not want[w]:
                # the documented zeros, c2 / T = 1
                z = np.zeros_like(coef)
                z[:, 1] = 1.0
                assert np.array_equal(coef, z) and not idx.any()
        check_records("bad flag (b) walker 0", su, o, pr.restate(su, batch[0]), batch[0], recs[0], W)
        # the accepted walker and the plain one, in a batch without the bad ones
        clean = np.array([batch[0], batch[5], good[1], good[2], good[3], good[4]])
        spec2, ok2 = engine.run_batch(clean, want_ok=True)
        assert ok2.tolist() == [1] * 6
        for a, b in ((0, 0), (5, 1)):
            rec2 = engine.prep_records(b)
            assert np.array_equal(recs[a][0], rec2[0], equal_nan=True) and np.array_equal(recs[a][1], rec2[1])
            assert recs[a][2:] == rec2[2:]
            assert np.array_equal(spec[a], spec2[b], equal_nan=True)
        check_spectra("bad flag (b) walker 0", spec[:1], o, batch[:1])
        # a bad walker's radii read 0 (bartrt_get_radius: the batch's first walker)
        spec3, ok3 = engine.run_batch(np.array([batch[1], batch[0], good[1], good[2], good[3], good[4]]), want_ok=True)
        assert ok3.tolist() == [0, 1, 1, 1, 1, 1] and not engine.get_radius().any()
        assert np.array_equal(spec3[1], spec[0])
    finally:
        trm.free_memory()
