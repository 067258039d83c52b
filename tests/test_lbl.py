"""Line-by-line (Voigt) path: TLI round trip and oracle sanity on CPU; device
extinction, spectra and the generated opacity grid against the oracle on GPU.

Tolerance: the device evaluates the Faddeeva function with a rational
approximation (|z| < 8: absolute error <= 1e-14 of the line-centre value, 1e-9
relative wherever the function is above 1e-6) / an asymptotic series (|z| >= 8: 3e-12; three terms from |z| = 100: 1.4e-11);
the oracle uses scipy's wofz.  1e-7 relative on sums of positive terms;
test_voigt_function_against_wofz holds the function itself."""
import numpy as np
import pytest

RTOL = 1e-7


def test_tli_round_trip(tmp_path):
    from bart_amd import synth_lbl
    from oracle import lbl_oracle
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=300, nwave=50, nlayers=5)
    dbs = lbl_oracle.read_tli(c.tli)
    assert [d["molecule"] for d in dbs] == ["H2O", "CO"]
    for got, src in zip(dbs, c.linedbs):
        o = np.argsort(src["wn"], kind="stable")
        assert np.array_equal(got["wn"], np.asarray(src["wn"])[o])
        assert np.array_equal(got["gf"], np.asarray(src["gf"])[o])
        assert np.array_equal(got["iso"], np.asarray(src["iso"])[o])
        assert len(got["isotopes"]) == 2 and got["isotopes"][0]["ratio"] == 0.98
        assert np.all(np.diff(got["wn"]) >= 0)


def test_isolated_line_integrates_to_its_strength(tmp_path):
    """One line, wide window: the profile integrates to S (Voigt is normalised),
    up to the wings beyond nwidth half-widths."""
    from bart_amd import synth, synth_lbl
    from oracle import lbl_oracle
    c = synth_lbl.make_lbl_case(str(tmp_path), molecules=("CO",), nlines=1, nwave=4001,
                                wnlow=2099.0, wndelt=0.0005, nlayers=3, nwidth=400)
    db = c.linedbs[0]
    db["wn"][:] = 2100.0; db["iso"][:] = 0; db["elow"][:] = 100.0; db["gf"][:] = 1e-5
    synth.write_tli(c.tli, c.linedbs, 2000.0, 2200.0)
    o = lbl_oracle.LblOracle(c.tcfg)
    prof = c.profiles()
    l = 2                                   # top layer: narrow, Doppler-dominated line
    ext = o.extinction(prof)[l]
    T, p, q = prof[0, l], o.press[l], prof[1:, l]
    info = db["isotopes"][0]
    Z = np.interp(T, db["temps"], info["Z"])
    n = info["ratio"] * q[c.species.index("CO")] * p / (lbl_oracle.KB * T)
    S = lbl_oracle.SIGCTE * 1e-5 * n / Z * np.exp(-lbl_oracle.EXPCTE * 100.0 / T) * \
        (1 - np.exp(-lbl_oracle.EXPCTE * 2100.0 / T))
    integ = np.sum(0.5 * (ext[1:] + ext[:-1]) * np.diff(o.wn))
    assert abs(integ / S - 1) < 2e-3
    assert ext.argmax() == 2000


@pytest.mark.gpu
def test_voigt_function_against_wofz():
    """The kernels' K(x, y) over the (x, y) plane the line-by-line path visits -- Doppler
    cores to pressure-broadened wings -- against scipy's Faddeeva function: every branch
    boundary (|z| = 8, 17, 100; y = 0.13 and the order steps below it), both sides."""
    from scipy.special import wofz
    from bart_amd import engine
    rng = np.random.default_rng(7)
    n = 400000
    x = np.concatenate([rng.uniform(0, 9, n), rng.uniform(7.9, 18, n), 10 ** rng.uniform(0.9, 4, n), np.zeros(1000),
                        np.nextafter(8.0, [0.0, 9.0]), np.nextafter(17.0, [0.0, 20.0]), np.nextafter(100.0, [0.0, 200.0])])
    y = 10 ** rng.uniform(-9, 3.5, x.size)
    y[::3] = 10 ** rng.uniform(-7, -0.5, y[::3].size)          # the small-y expansions' range, densely
    steps = np.array([6.0e-6, 5.0e-4, 3.0e-3, 9.5e-3, 2.2e-2, 4.0e-2, 6.5e-2, 9.5e-2, 0.13])
    y[1::7] = np.nextafter(rng.choice(steps, y[1::7].size), rng.choice([0.0, 1.0], y[1::7].size))
    y[-6:] = 1e-6
    k = engine.voigt(x, y)
    ref = wofz(x + 1j * y).real
    r2 = x * x + y * y
    assert np.all(np.isfinite(k)) and np.all(k > 0)
    rel = np.abs(k / ref - 1)
    # |z| >= 100: three terms of the asymptotic series (1.4e-11 at |z| = 100)
    assert rel[r2 >= 1e4].max() < 2e-11
    # 8 <= |z| < 100: the series (eleven terms from 8: 3e-12, six from 17: 3.8e-12 near the real axis), or for y <= 0.13 and
    # |z| < 17 the expansion about the real axis (cancellation: 5e-12); the omitted exp(-z^2) is < 2e-28
    assert rel[(r2 >= 64) & (r2 < 1e4)].max() < 1e-11
    # |z| < 8: the expansion about the real axis (truncation 3e-12) or, y > 0.13, Weideman N = 36 (3e-13) --
    # RELATIVE everywhere (the N = 40 approximation that covered all of |z| < 8 before was held to
    # 1e-14 of the line-centre value and 1e-9 relative above 1e-6)
    assert rel[r2 < 64].max() < 5e-12
    # broadcasting / empty input
    assert engine.voigt(np.zeros(0), np.zeros(0)).size == 0
    assert engine.voigt(1.0, np.array([0.5, 2.0])).shape == (2,)


@pytest.mark.gpu
def test_lbl_extinction_and_spectrum_match_oracle(tmp_path):
    from bart_amd import engine, synth_lbl, transit_module as trm
    from oracle import lbl_oracle, rt_oracle as orc
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=1500, nwave=300, nlayers=16, cia=True)
    engine.init(c.tcfg)
    try:
        prof = c.profiles()
        ext = engine.lbl_extinction(prof)
        ref = lbl_oracle.LblOracle(c.tcfg).extinction(prof)
        assert ref.max() > 0
        np.testing.assert_allclose(ext, ref, rtol=RTOL, atol=1e-30)
        o = orc.OracleEngine(c.tcfg)
        o.set_extra_extinction(ref)
        spec = trm.run_transit(prof.ravel(), trm.get_no_samples())
        np.testing.assert_allclose(spec, o.run(prof), rtol=RTOL)
        # a second, different profile in a batch of two
        p2 = c.profiles(temp=c.temp0 * 1.2)
        both = engine.run_batch(np.array([prof.ravel(), p2.ravel()]))
        o.set_extra_extinction(lbl_oracle.LblOracle(c.tcfg).extinction(p2))
        np.testing.assert_allclose(both[1], o.run(p2), rtol=RTOL)
        assert np.array_equal(both[0], spec)
    finally:
        trm.free_memory()


def test_downsample_rule():
    """The reduction of the oversampled line sums (oracle statement of DESIGN.md C15):
    odd factor = mean of the centred points, even factor = end points at half weight,
    grid ends = the half window that exists; a linear function is reproduced inside."""
    from oracle import lbl_oracle
    x = np.arange(0.0, 25.0)                     # W = 7 at dv = 4; W = 9 at dv = 3
    np.testing.assert_allclose(lbl_oracle.downsample(x, 4)[1:-1], x[4:-4:4], rtol=1e-15)
    np.testing.assert_allclose(lbl_oracle.downsample(x, 3)[1:-1], x[3:-3:3], rtol=1e-15)
    assert lbl_oracle.downsample(x, 4)[0] == (0 + 1 + 0.5 * 2) / 2.5
    assert lbl_oracle.downsample(x, 3)[-1] == (23 + 24) / 2
    y = np.zeros(25); y[10] = 1.0                # a spike two fine points left of output point 3
    assert lbl_oracle.downsample(y, 4)[2] == 0.5 / 4 and lbl_oracle.downsample(y, 4)[3] == 0.5 / 4
    assert lbl_oracle.divisors(12) == [1, 2, 3, 4, 6, 12]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [
    dict(wnosamp=4),                                            # a small factor: dv in {1, 2, 4}
    dict(wnosamp=2160),                                         # the reference cfgs' value: dv up to a few dozen
    dict(wnosamp=2160, wndelt=1.0, nwave=40, nlines=150),       # 1 cm-1 sampling (demo): dv in the hundreds
    dict(wnosamp=5, rule="full"),                               # odd factor on every layer
    dict(wnosamp=2160, rule="full", nwave=9, nlines=60, nlayers=4),   # one output point per sub-tile
])
def test_wnosamp_oversampling_matches_oracle(tmp_path, kw):
    """`wnosamp` (code/makecfg.py:38, examples/demo/transit_demo.cfg:27-29; VERDICT r1
    item 2; convention C15): the line sums are evaluated dv times finer than the output
    grid -- dv per layer the smallest divisor of wnosamp that puts two points on the
    narrowest half-width -- and reduced to it; against the scipy-Faddeeva oracle's
    statement of the same rule, incl. the blocks of a sharded engine."""
    import os
    import subprocess
    import sys
    from bart_amd import synth_lbl
    from oracle import lbl_oracle
    kw = dict(kw)
    rule = kw.pop("rule", "divisor")
    kw.setdefault("nlines", 900)
    kw.setdefault("nwave", 150)
    kw.setdefault("nlayers", 10)
    c = synth_lbl.make_lbl_case(str(tmp_path), **kw)
    prof = c.profiles()
    np.save(os.path.join(c.dir, "p.npy"), prof)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import numpy as np, sys; sys.path.insert(0, %r)\n"
            "from bart_amd import engine, transit_module as trm\n"
            "p = np.load(%r); out = []\n"
            "for sh in (None, (0, 3), (1, 3), (2, 3)):\n"
            "    engine.init(%r, shard=sh); out.append(engine.lbl_extinction(p)); trm.free_memory()\n"
            "np.save(%r, out[0]); np.save(%r, np.concatenate(out[1:], axis=1))\n"
            % (root, os.path.join(c.dir, "p.npy"), c.tcfg, os.path.join(c.dir, "e.npy"), os.path.join(c.dir, "s.npy")))
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, BARTRT_OSAMP_RULE=rule), timeout=600)
    ext = np.load(os.path.join(c.dir, "e.npy"))
    o = lbl_oracle.LblOracle(c.tcfg, osamp_rule=rule)
    dvs = [o.layer_dv(prof[0, l], o.press[l], prof[1:, l]) for l in range(prof.shape[1])]
    assert max(dvs) > 1 and all(o.osamp % d == 0 for d in dvs)
    ref = o.extinction(prof)
    assert ref.max() > 0
    np.testing.assert_allclose(ext, ref, rtol=RTOL, atol=1e-30 + 1e-13 * ref.max())
    assert np.array_equal(np.load(os.path.join(c.dir, "s.npy")), ext)      # sharded blocks: bit for bit
    o1 = lbl_oracle.LblOracle(c.tcfg)
    o1.osamp = 1                                          # the output-point evaluation is something else
    assert np.abs(o1.extinction(prof) - ref).max() > 1e-3 * ref.max()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [
    dict(wnosamp=1),                                            # profiles on the output points
    dict(wnosamp=4),
    dict(wnosamp=2160),                                         # the reference cfgs' value
    dict(wnosamp=2160, wndelt=1.0, nwave=40, nlines=150),       # 1 cm-1 sampling (demo): dv in the hundreds
    dict(wnosamp=6, extra_keys=dict(ndop=7, nlor=5)),           # a coarse width grid
    dict(wnosamp=6, extra_keys=dict(ndop=1, nlor=1)),           # one width each
    dict(wnosamp=12, cia=True, ptop=1e-4, pbottom=30.0, nwidth=5, ethresh=1e-3),
])
def test_voigt_width_grid_matches_oracle(tmp_path, kw):
    """`voigt grid` (SURVEY.md App. A-5 as recalled): profiles tabulated on a grid
    of Doppler x Lorentz half-widths, a line takes the nearest widths' profile centred on the
    sampling point nearest to its centre.  The table-lookup kernels against the oracle's
    statement of the same rule (scipy Faddeeva values at the grid widths) -- extinction of the
    whole engine and of its wavenumber blocks (bit for bit), the spectrum on top of it, and the
    switch's other value: the exact evaluation differs, and is what `voigt exact` returns."""
    import os
    import subprocess
    import sys
    from bart_amd import synth_lbl
    from oracle import lbl_oracle, rt_oracle as orc
    kw = dict(kw)
    extra = dict(kw.pop("extra_keys", {}), voigt="grid")
    kw.setdefault("nlines", 900)
    kw.setdefault("nwave", 150)
    kw.setdefault("nlayers", 10)
    c = synth_lbl.make_lbl_case(str(tmp_path), extra_keys=extra, **kw)
    assert "voigt grid" in open(c.tcfg).read()
    prof = c.profiles()
    np.save(os.path.join(c.dir, "p.npy"), prof)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    f = lambda n: os.path.join(c.dir, n)
    code = ("import numpy as np, sys, os; sys.path.insert(0, %r)\n"
            "from bart_amd import engine, transit_module as trm\n"
            "p = np.load(%r); out = []\n"
            "for sh in (None, (0, 3), (1, 3), (2, 3)):\n"
            "    engine.init(%r, shard=sh); out.append(engine.lbl_extinction(p))\n"
            "    if sh is None: np.save(%r, engine.run_batch(np.array([p.ravel(), p.ravel()])))\n"
            "    trm.free_memory()\n"
            "np.save(%r, out[0]); np.save(%r, np.concatenate(out[1:], axis=1))\n"
            "os.environ['BARTRT_VOIGT'] = 'exact'\n"
            "engine.init(%r); np.save(%r, engine.lbl_extinction(p)); trm.free_memory()\n"
            % (root, f("p.npy"), c.tcfg, f("spec.npy"), f("e.npy"), f("s.npy"), c.tcfg, f("x.npy")))
    subprocess.check_call([sys.executable, "-c", code], timeout=600)
    ext = np.load(f("e.npy"))
    o = lbl_oracle.LblOracle(c.tcfg)
    assert o.voigt == "grid"
    ref = o.extinction(prof)
    assert ref.max() > 0
    np.testing.assert_allclose(ext, ref, rtol=RTOL, atol=1e-30 + 1e-13 * ref.max())
    assert np.array_equal(np.load(f("s.npy")), ext)                     # sharded blocks: bit for bit
    exact = lbl_oracle.LblOracle(c.tcfg, voigt="exact").extinction(prof)
    np.testing.assert_allclose(np.load(f("x.npy")), exact, rtol=RTOL, atol=1e-30 + 1e-13 * exact.max())
    assert np.abs(exact - ref).max() > 1e-4 * ref.max()                  # the two values of the switch differ
    # the spectrum over the width-grid extinction (the oracle's RT on the oracle's extinction)
    spec = np.load(f("spec.npy"))
    assert np.array_equal(spec[0], spec[1]) and np.all(np.isfinite(spec))
    oe = orc.OracleEngine(c.tcfg)
    oe.set_extra_extinction(ref)
    want = oe.run(prof)
    np.testing.assert_allclose(spec[0], want, rtol=1e-6, atol=1e-9 * np.abs(want).max())


@pytest.mark.gpu
def test_voigt_width_grid_in_the_generated_opacity_grid(tmp_path):
    """The `--justOpacity` step under `voigt grid`: the table mode of the same kernels."""
    from bart_amd import engine, synth_lbl, transit_module as trm
    from oracle import lbl_oracle, rt_oracle as orc
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=300, nwave=90, nlayers=5, with_table=True, wnosamp=12,
                                tlow=700.0, thigh=1900.0, tempdelt=600.0, ptop=1e-4, pbottom=1.0,
                                extra_keys=dict(voigt="grid", ndop=12, nlor=9))
    engine.init(c.tcfg)
    try:
        op = orc.read_opacity(c.keys["opacityfile"])
        ref = lbl_oracle.LblOracle(c.tcfg).opacity_table(op["temps"])
        np.testing.assert_allclose(op["kappa"], ref, rtol=RTOL, atol=1e-300 + 1e-13 * ref.max())
        with pytest.raises(trm.TransitError, match="voigt"):
            cfg2 = c.tcfg + ".bad"
            open(cfg2, "w").write(open(c.tcfg).read().replace("voigt grid", "voigt lookup"))
            trm.free_memory()
            trm.transit_init(3, ["transit", "-c", cfg2])
    finally:
        trm.free_memory()


@pytest.mark.gpu
def test_wnosamp_in_the_generated_opacity_grid(tmp_path):
    """The `--justOpacity` step honours wnosamp too: grid mode of the same kernels."""
    from bart_amd import engine, synth_lbl, transit_module as trm
    from oracle import lbl_oracle, rt_oracle as orc
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=300, nwave=90, nlayers=5, with_table=True, wnosamp=12,
                                tlow=700.0, thigh=1900.0, tempdelt=600.0, ptop=1e-4, pbottom=1.0)
    engine.init(c.tcfg)
    try:
        op = orc.read_opacity(c.keys["opacityfile"])
        ref = lbl_oracle.LblOracle(c.tcfg).opacity_table(op["temps"])
        np.testing.assert_allclose(op["kappa"], ref, rtol=RTOL, atol=1e-300 + 1e-13 * ref.max())
    finally:
        trm.free_memory()


@pytest.mark.gpu
def test_extinction_chunks_keep_per_walker_overrides(tmp_path, monkeypatch):
    """The eager line-by-line path works through the walkers in chunks bounded by the
    size of ext[walkers][L][W]; the walkers' own cloud-top / scattering parameters
    (BARTfunc.py:350-360) must follow them into every chunk (chunks after
    the first fell back to the engine-wide values).  Two walkers per chunk and one
    chunk for all give the same band fluxes, and so does walker by walker."""
    from bart_amd import engine, synth_lbl, transit_module as trm
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=600, nwave=150, nlayers=10, cia=True)
    L, W = 10, 150
    engine.init(c.tcfg)
    try:
        ptargs = [1.145 * 6.95508e10, 6075.0, 100.0, 0.047 * 1.4959787066e13, 897.70]
        engine.step_setup(ptargs, 0.0, 1e9, c.abund0, [c.species.index("CO")], [0], [W],
                          np.full(W, 1.0 / W), np.ones(W), 0.1)
        engine.step_set_extras(0, 1, 1)      # cloud top and scattering travel with each walker
        rng = np.random.default_rng(11)
        base = np.array([-2.0, 0.0, 1.0, 0.0, 0.98, -1.0, 1.0, 0.0])   # PT(5), log10 cloudtop, scattering, CO
        pars = base + rng.normal(0, [0.1, 0.1, 0.1, 0.0, 0.01, 1.0, 0.8, 0.3], (5, 8))
        whole, st = engine.step_batch(pars, 1)
        assert (st == 0).all() and np.ptp(whole) > 0
        monkeypatch.setenv("BARTRT_LBL_CHUNK_BYTES", str(2 * L * W * 8))
        chunked, _ = engine.step_batch(pars, 1)
        assert np.array_equal(chunked, whole)
        monkeypatch.setenv("BARTRT_LBL_CHUNK_BYTES", "1")
        single = np.array([engine.step_batch(q[None, :], 1)[0][0] for q in pars])
        assert np.array_equal(single, whole)
    finally:
        trm.free_memory()


@pytest.mark.gpu
def test_several_linedb_files_are_merged(tmp_path):
    """makecfg writes one `linedb <file>` line per TLI (code/makecfg.py:93-104):
    two files, one molecule each, on two lines give the extinction of the single
    file that holds both databases -- bit for bit (the second line used
    to replace the first)."""
    from bart_amd import engine, synth, synth_lbl, transit_module as trm
    from oracle import lbl_oracle
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=700, nwave=180, nlayers=8)
    prof = c.profiles()
    engine.init(c.tcfg)
    try:
        one = engine.lbl_extinction(prof)
    finally:
        trm.free_memory()
    parts = []
    for i, db in enumerate(c.linedbs):
        parts.append(str(tmp_path / ("part%d.tli" % i)))
        synth.write_tli(parts[-1], [db], 1900.0, 2100.0)
    two = str(tmp_path / "two.cfg")
    lines = [l for l in open(c.tcfg) if not l.startswith("linedb")]
    open(two, "w").write("".join(lines) + "".join("linedb %s\n" % p for p in parts))
    assert lbl_oracle.LblOracle(two).dbs[1]["molecule"] == "CO"
    engine.init(two)
    try:
        assert np.array_equal(engine.lbl_extinction(prof), one)
    finally:
        trm.free_memory()
    # a repeated key that is not a file list keeps its last value
    open(two, "a").write("nwidth 3\n")
    engine.init(two)
    try:
        narrow = engine.lbl_extinction(prof)
        assert (narrow <= one).all() and (narrow < one).any()
    finally:
        trm.free_memory()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [
    dict(ptop=1e-6, pbottom=1e-3, nwave=333),              # Doppler cores only: the pair kernel, ragged last wave
    dict(ptop=1.0, pbottom=100.0, nwave=300),              # pressure-broadened only: the tile kernel
    dict(ptop=1e-5, pbottom=100.0, nwave=70, wndelt=0.4),  # coarse grid: narrow = less than one point
    dict(ptop=1e-4, pbottom=1.0, nwave=260, nlines=40),    # sparse list: empty windows
])
def test_narrow_and_broad_states(tmp_path, kw):
    """Each layer state is summed by one of two kernels (lines a few points wide /
    lines many points wide): atmospheres that are all one kind, grids that end
    inside a wave, windows without lines."""
    from bart_amd import engine, synth_lbl, transit_module as trm
    from oracle import lbl_oracle
    kw = dict(kw)
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=kw.pop("nlines", 1200), nlayers=12, **kw)
    engine.init(c.tcfg)
    try:
        prof = c.profiles()
        ext = engine.lbl_extinction(prof)
        ref = lbl_oracle.LblOracle(c.tcfg).extinction(prof)
        assert ref.max() > 0
        np.testing.assert_allclose(ext, ref, rtol=RTOL, atol=1e-30 + 1e-12 * ref.max())
    finally:
        trm.free_memory()


@pytest.mark.gpu
def test_corrupt_transition_count_is_refused(tmp_path):
    """A transition count the TLI file cannot hold is an input error at once, not an
    allocation of that many records."""
    import struct
    import time
    from bart_amd import synth_lbl, transit_module as trm
    lc = synth_lbl.make_lbl_case(str(tmp_path), nlines=50, nwave=20, nlayers=4)
    data = bytearray(open(lc.tli, "rb").read())
    first = struct.pack("=q", len(lc.linedbs[0]["wn"]))
    at = data.index(first, 32)                           # the first database's transition count
    data[at:at + 8] = struct.pack("=q", 1 << 33)
    open(lc.tli, "wb").write(bytes(data))
    t0 = time.time()
    with pytest.raises(trm.TransitError, match="truncated|transition count"):
        trm.transit_init(3, ["transit", "-c", lc.tcfg])
    assert time.time() - t0 < 20


@pytest.mark.gpu
def test_ethresh_and_nwidth_are_applied(tmp_path):
    from bart_amd import engine, synth_lbl, transit_module as trm
    from oracle import lbl_oracle
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=800, nwave=200, nlayers=8, nwidth=5,
                                ethresh=1e-2)
    engine.init(c.tcfg)
    try:
        prof = c.profiles()
        ext = engine.lbl_extinction(prof)
        ref = lbl_oracle.LblOracle(c.tcfg).extinction(prof)
        np.testing.assert_allclose(ext, ref, rtol=RTOL, atol=1e-30)
        assert (ref == 0).any()          # the narrow cut leaves gaps between lines
    finally:
        trm.free_memory()


@pytest.mark.gpu
def test_opacity_grid_generated_from_lines(tmp_path):
    """opacityfile named but absent + linedb present: the engine builds the grid
    (the reference's `transit --justOpacity` step, BART.py:561-565), then runs
    on it."""
    import os
    from bart_amd import engine, synth_lbl, transit_module as trm
    from oracle import lbl_oracle, rt_oracle as orc
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=400, nwave=120, nlayers=6, with_table=True,
                                tlow=600.0, thigh=1800.0, tempdelt=600.0)
    path = c.keys["opacityfile"]
    assert not os.path.exists(path)
    engine.init(c.tcfg)
    try:
        assert os.path.exists(path)
        op = orc.read_opacity(path)
        assert list(op["temps"]) == [600.0, 1200.0, 1800.0] and op["kappa"].shape == (6, 3, 2, 120)
        ref = lbl_oracle.LblOracle(c.tcfg).opacity_table(op["temps"])
        np.testing.assert_allclose(op["kappa"], ref, rtol=RTOL, atol=1e-300)
        prof = c.profiles(temp=np.linspace(1500.0, 700.0, 6))
        spec = trm.run_transit(prof.ravel(), trm.get_no_samples())
        np.testing.assert_allclose(spec, orc.OracleEngine(c.tcfg).run(prof), rtol=1e-10)
    finally:
        trm.free_memory()


@pytest.mark.gpu
def test_lazy_fused_kernel_matches_eager(tmp_path):
    """BARTRT_LBL=lazy (layers' line sums evaluated only as deep as tau requires)
    gives the same spectra as the default eager two-pass form."""
    import os, subprocess, sys
    from bart_amd import synth_lbl
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=1200, nwave=600, nlayers=24, cia=True)
    prof = np.array([c.profiles().ravel(), c.profiles(temp=c.temp0 * 0.9).ravel()])
    np.save(os.path.join(c.dir, "p.npy"), prof)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("eager", "lazy"):
        out = os.path.join(c.dir, "s_%s.npy" % mode)
        code = ("import numpy as np, sys; sys.path.insert(0, %r)\n"
                "from bart_amd import engine, transit_module as trm\n"
                "engine.init(%r); np.save(%r, engine.run_batch(np.load(%r))); trm.free_memory()\n"
                % (root, c.tcfg, out, os.path.join(c.dir, "p.npy")))
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, BARTRT_LBL=mode),
                              timeout=300)
        outs[mode] = np.load(out)
    np.testing.assert_allclose(outs["lazy"], outs["eager"], rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("wnosamp,nslice,layers", [(1, 2000, range(0, 100, 4)), (2160, 400, (3, 40, 71, 99))])
def test_config5_slice_against_the_oracle(tmp_path, wnosamp, nslice, layers):
    """BASELINE config 5 at full size (1e6 lines, 1e5 points, 100 layers) where the
    oracle CAN follow: a block of consecutive samples from the middle of
    the grid, every line of the 1e6-line list that reaches it (the strength threshold
    is taken over the whole list, as in the full run), against scipy's Faddeeva
    function at 1e-7 -- the engine holds that block as one wavenumber shard of the
    full case.  Also with the reference cfgs' wnosamp 2160."""
    from bart_amd import engine, synth_lbl, transit_module as trm
    from oracle import lbl_oracle
    mols = ("H2O", "CO", "CO2", "CH4")
    c = synth_lbl.make_lbl_case(str(tmp_path), molecules=mols, nlines=250000, nwave=100000,
                                wnlow=1000.0, wndelt=0.1, nlayers=100, cia=False, wnosamp=wnosamp)
    nshard = 100000 // nslice
    r = nshard // 2 + 1
    engine.init(c.tcfg, shard=(r, nshard))
    try:
        lo, hi = engine.local_range()
        assert hi - lo == nslice
        prof = c.profiles()
        ext = engine.lbl_extinction(prof)
    finally:
        trm.free_memory()
    o = lbl_oracle.LblOracle(c.tcfg, wn_slice=(lo, hi))
    assert len(o.wn) == nslice and sum(len(db["wn"]) for db in o.dbs) == 1000000
    layers = list(layers)
    ref = o.extinction(prof, layers=layers)
    assert ref[layers].max() > 0 and (ref[layers] > 0).mean() > 0.5
    np.testing.assert_allclose(ext[layers], ref[layers], rtol=RTOL, atol=1e-30 + 1e-13 * ref.max())


@pytest.mark.gpu
def test_config5_size_properties(tmp_path):
    """BASELINE config 5's size (1e6 lines, 1e5 points, 100 layers), where the
    oracle cannot follow: extinction is non-negative and exactly linear in a
    molecule's abundance (a factor 2 is a bit-exact doubling: strengths and the
    ethresh reference scale together, widths depend on H2 / He only), and the
    wavenumber blocks of a sharded engine concatenate to the unsharded result bit
    for bit (which of the two accumulation kernels owns a layer state depends on
    the tiling of the grid: they must agree to the last bit)."""
    from bart_amd import engine, synth_lbl, transit_module as trm
    mols = ("H2O", "CO", "CO2", "CH4")
    c = synth_lbl.make_lbl_case(str(tmp_path), molecules=mols, nlines=250000, nwave=100000,
                                wnlow=1000.0, wndelt=0.1, nlayers=100, cia=False)
    engine.init(c.tcfg)
    try:
        prof = c.profiles()
        ext = engine.lbl_extinction(prof)
        assert ext.shape == (100, 100000) and np.all(np.isfinite(ext)) and ext.min() >= 0 and ext.max() > 0
        sp = engine.species()
        twice = prof.copy()
        for m in mols:
            twice[1 + sp.index(m)] *= 2.0
        assert np.array_equal(engine.lbl_extinction(twice), 2.0 * ext)
        spec = trm.run_transit(prof.ravel(), 100000)     # default rule (1): line cores put tau steps >> 1
        assert np.all(np.isfinite(spec))                  # on single layers, where its panels may go negative
        trm.set_integ(0)
        spec0 = trm.run_transit(prof.ravel(), 100000)
        assert np.all(np.isfinite(spec0)) and spec0.min() > 0
        assert np.median(np.abs(spec / spec0 - 1)) < 0.05
    finally:
        trm.free_memory()
    parts = []
    for r in range(4):
        engine.init(c.tcfg, shard=(r, 4))
        parts.append(engine.lbl_extinction(prof))
        trm.free_memory()
    assert np.array_equal(np.concatenate(parts, axis=1), ext)


@pytest.mark.gpu
@pytest.mark.parametrize("nlayers,transparent", [(16, 0), (40, 1), (150, 0)])
def test_line_by_line_in_transit_geometry(tmp_path, nlayers, transparent):
    """On-the-fly line-by-line extinction through the transit geometry: the extinction array feeds the
    matrix-tile kernel (rt_transit_mfma with the array as one more load; 150 layers: its deep form) --
    modulation spectra of a batch against the oracle's chord integration over the oracle's extinction,
    with and without an opaque core."""
    from bart_amd import engine, synth_lbl, transit_module as trm
    from oracle import lbl_oracle, rt_oracle as orc
    extra = {"solution": "transit", "starrad": 1.145}
    if transparent:
        extra["transparent"] = 1
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=900, nwave=200, nlayers=nlayers, cia=True, extra_keys=extra)
    engine.init(c.tcfg)
    try:
        profs = [c.profiles(), c.profiles(temp=c.temp0 * 1.15), c.profiles(temp=c.temp0 * 0.9)]
        got = engine.run_batch(np.array([p.ravel() for p in profs]))
        lo = lbl_oracle.LblOracle(c.tcfg)
        o = orc.OracleEngine(c.tcfg)
        assert o.c.solution == 1 and o.c.transparent == transparent
        for w, p in enumerate(profs):
            o.set_extra_extinction(lo.extinction(p))
            ref = o.run(p)
            assert 0 < ref.min() and ref.max() < 1
            np.testing.assert_allclose(got[w], ref, rtol=1e-9)
    finally:
        trm.free_memory()


@pytest.mark.gpu
@pytest.mark.parametrize("wnosamp,ptop,pbottom", [(1, 1e-6, 1e-2), (90, 1e-6, 1e-2), (1, 1e-3, 30.0)])
def test_voigt_expansion_switch(tmp_path, wnosamp, ptop, pbottom):
    """`BARTRT_VOIGT_TAYLOR=0` (A/B runs) evaluates every |z| < 8 sample with Weideman's rational approximation, the
    default takes the expansion about the real axis where y <= 0.13 -- Doppler-dominated layers, on the output
    grid and oversampled, and pressure-broadened ones where the switch must change nothing but rounding.  The two
    agree to the rational approximation's own accuracy, and each with the oracle (scipy's wofz)."""
    import os
    from bart_amd import engine, synth_lbl, transit_module as trm
    from oracle import lbl_oracle
    c = synth_lbl.make_lbl_case(str(tmp_path), nlines=1200, nwave=250, nlayers=10, wndelt=0.05, ptop=ptop,
                                pbottom=pbottom, wnosamp=wnosamp)
    prof = c.profiles()
    ref = lbl_oracle.LblOracle(c.tcfg).extinction(prof)
    out = {}
    for flag in ("1", "0"):
        os.environ["BARTRT_VOIGT_TAYLOR"] = flag
        try:
            engine.init(c.tcfg)
            out[flag] = engine.lbl_extinction(prof)
        finally:
            del os.environ["BARTRT_VOIGT_TAYLOR"]
            trm.free_memory()
        np.testing.assert_allclose(out[flag], ref, rtol=RTOL, atol=1e-30)
    # (N = 36 is good to 8e-10 where K > 1e-6 of the line centre and loses from there down: samples that a single
    # line's far core dominates differ by up to 1e-8 -- the rational approximation's error, the expansion's is 3e-12)
    np.testing.assert_allclose(out["1"], out["0"], rtol=5e-8, atol=1e-30)
    if pbottom < 1.0:
        assert not np.array_equal(out["1"], out["0"])      # the branch is taken
