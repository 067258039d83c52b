"""GPU: the elementary functions every RT kernel calls (csrc/kernels.hpp exp_rt_n / exp_rt, exp_core, rcp_core, rcp_n1;
csrc/lbl.hip exp_rt_fma3; the Planck term as its call sites spell it), evaluated by the device through
bartrt_rt_math (engine.rt_math) and held to references that share nothing with them:

  exp_rt, exp_core .. the exact restatement of the same formula (tests/rtmath_restate.py, mpmath at 50 digits) on
                      rt_points(): what is left is fp64 rounding, <= 4e-16 relative
  bit identity ...... exp_rt_fma3 and every slot of exp_rt_n<4> give exp_rt's bits
  reciprocals ....... |y d - 1| in mpmath: the header's figures, and what one Newton step implies from the estimate
  planck_inv ........ the restated exp_rt composed with an exact reciprocal
  two eclipse cases . against the oracle at the suite's 1e-10, where the synthetic grid never goes: optically thin
                      layers (arguments near 0 in every kernel form) and Planck exponents below ln2 / 2

The restatement's own distance from mpmath.exp is held on the CPU (tests/test_rt_math_cpu.py).  Figures are printed
before they are asserted (run with -s); MEASUREMENTS.md keeps them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rtmath_restate as rs

pytestmark = pytest.mark.gpu

RTOL = 1e-10                      # tests/test_gpu_parity.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_NORMAL = 2.0 ** -1022

_device = {}


def device(name, x):
    """engine.rt_math(name, x) on one of the shared point sets, evaluated once per process."""
    from bart_amd import engine
    key = (name, id(x))
    if key not in _device:
        _device[key] = (x, engine.rt_math(name, x))       # (x kept alive: its id is the key)
    return _device[key][1]


def exp_rt_points():
    return rs.restated_on_points("exp_rt")[0]


# ---- exp_rt, exp_core ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exp_rt", "exp_core"])
def test_exponentials_against_their_exact_restatement(name):
    """Bound 4e-16: every Horner step rounds by half an ulp of its result; the error of the step of coefficient
    c_j reaches the value multiplied by |r|^j <= (ln2/2)^j, so the sum is at most 2^-53 / (1 - ln2/2) = 1.7e-16
    relative to a value q >= 0.707 (2.4e-16 of it), plus r's own half ulp times |r| (0.4e-16): < 2.7e-16.  2^n is
    exact.  Measured on an MI355X (printed below; MEASUREMENTS.md): exp_rt 1.11e-16 (at 2^-53), exp_core 1.28e-16."""
    mp = rs.mp50()
    x, ref = rs.restated_on_points(name)
    got = device(name, x)
    assert got.shape == x.shape
    assert np.all(np.isfinite(got)) and np.all(got >= TINY_NORMAL), x[~(got >= TINY_NORMAL)][:5]
    worst = (0.0, None, 0)
    for v, g, (r, n) in zip(x, got, ref):
        err = float(abs(mp.mpf(float(g)) / r - 1))
        if err > worst[0]:
            worst = (err, float(v), n)
    print("%s: %d points, worst device / restatement - 1 = %.4g at x = %r (n = %d)" % ((name, x.size) + worst))
    assert worst[0] <= 4e-16, worst
    from bart_amd import engine
    assert engine.rt_math(name, 0.0) == 1.0
    assert engine.rt_math(name, np.zeros(0)).size == 0
    # the range ends, by their bits' meaning: n = -1021 and 1010 (1023) leave a normal number
    lo, hi = engine.rt_math(name, np.array([rs.X_MIN, rs.X_MAX_RT if name == "exp_rt" else rs.X_MAX_CORE]))
    assert 3.3e-308 * 0.999 < lo < 3.31e-308 * 1.001 and hi > (1.0142e304 if name == "exp_rt" else 8.2184e307) * 0.999


def test_copies_of_exp_rt_give_the_same_bits():
    """exp_rt_fma3 ("same operations, same bits", csrc/lbl.hip) and each of the four slots of the interleaved
    exp_rt_n<4>: equal to exp_rt as uint64 on every point; the inputs are rotated so every slot sees every point, and
    a length that is no multiple of four leaves a ragged last lane."""
    from bart_amd import engine
    x = exp_rt_points()
    ref = device("exp_rt", x).view(np.uint64)
    got = engine.rt_math("exp_rt_fma3", x).view(np.uint64)
    print("exp_rt_fma3: %d of %d points differ from exp_rt" % (int((got != ref).sum()), x.size))
    assert np.array_equal(got, ref), x[got != ref][:5]
    for rot in range(4):
        xs = np.ascontiguousarray(np.roll(x, rot))
        got = engine.rt_math("exp_rt_n4", xs).view(np.uint64)
        bad = got != np.roll(ref, rot)
        print("exp_rt_n4, inputs rotated by %d: %d of %d points differ from exp_rt" % (rot, int(bad.sum()), x.size))
        assert not bad.any(), (rot, xs[bad][:5])
    for cut in (1, 2, 3):
        got = engine.rt_math("exp_rt_n4", x[:-cut].copy()).view(np.uint64)
        assert np.array_equal(got, ref[:-cut]), cut
    assert engine.rt_math("exp_rt_n4", x[:1].copy()).view(np.uint64)[0] == ref[0]


# ---- the reciprocals -------------------------------------------------------------------------------------------------
def planck_points():
    rng = np.random.default_rng(20261021)
    x = list(np.exp(rng.uniform(np.log(1e-8), np.log(700.0), 8192)))
    h = rs.LN2 / 2
    x += [np.nextafter(h, 0.0), np.nextafter(h, 1.0), np.nextafter(700.0, 0.0), np.nextafter(700.0, np.inf), 701.0, 1e4]
    return np.array(x, np.float64)


_rcp = None


def rcp_points():
    global _rcp
    if _rcp is None:
        mp = rs.mp50()
        rng = np.random.default_rng(20261022)
        d = list(np.exp(rng.uniform(np.log(1e-300), np.log(1e300), 65536)))
        for k in range(-996, 997, 12):
            d += [np.nextafter(2.0 ** k, 0.0), 2.0 ** k, np.nextafter(2.0 ** k, np.inf)]
        d += [float(mp.expm1(mp.mpf(float(v)))) for v in planck_points() if v <= 700.0]
        _rcp = np.array(d, np.float64)
        _rcp.setflags(write=False)
    return _rcp


def rcp_errors(d, y):
    """|y d - 1| per point, the product and the difference formed in mpmath (exact at 50 digits: 106 bits)."""
    mp = rs.mp50()
    one = mp.mpf(1)
    return np.array([float(abs(mp.mpf(a) * mp.mpf(b) - one)) for a, b in zip(d.tolist(), y.tolist())])


def test_reciprocals_hold_their_stated_errors():
    """rcp_core <= 1.2e-16 and rcp_n1 <= 2.3e-15: the header's figures, last digit rounded up.  The hardware estimate
    is recorded, not bounded by a number of its own; what one Newton step makes of it is: with e = 1 - d y the step
    returns y (1 + e) up to the roundings of e (2^-53 e) and of the result (2^-53), so 1 - d y' = e^2 and
    |y' d - 1| <= e^2 + 1.01 * 2^-53 point by point."""
    d = rcp_points()
    assert np.all(d >= TINY_NORMAL) and np.all(np.isfinite(d))
    err = {}
    for name in ("rcp_raw", "rcp_n1", "rcp_core"):
        y = device(name, d)
        assert np.all(np.isfinite(y)) and np.all(y > 0)
        err[name] = rcp_errors(d, y)
        i = int(np.argmax(err[name]))
        print("%s: %d points, worst |y d - 1| = %.4g at d = %r" % (name, d.size, err[name][i], float(d[i])))
    step = err["rcp_n1"] - (err["rcp_raw"] ** 2 + 1.01 * 2.0 ** -53)
    i = int(np.argmax(step))
    print("rcp_n1 against one Newton step from the estimate: largest excess %.4g at d = %r (n1 %.4g, raw %.4g)"
          % (step[i], float(d[i]), err["rcp_n1"][i], err["rcp_raw"][i]))
    assert step[i] <= 0.0
    assert err["rcp_core"].max() <= 1.2e-16
    assert err["rcp_n1"].max() <= 2.3e-15


# ---- the Planck term -------------------------------------------------------------------------------------------------
def test_planck_term_as_the_call_sites_spell_it():
    """rcp_n1(exp_rt(fmin(x, 700)) - 1) against 1 / (restated exp_rt - 1): exp_rt's rounding (4e-16 of e^x) stands
    under the difference, e^x / (e^x - 1) times as large in it, and the one-step reciprocal adds its 2.3e-15.  Beyond
    the clamp the result is the one at 700, bit for bit."""
    from bart_amd import engine
    mp, k = rs.mp50(), rs.read_kernels_hpp()
    x = planck_points()
    got = engine.rt_math("planck_inv", x)
    assert np.all(np.isfinite(got)) and np.all(got >= TINY_NORMAL)
    worst, worst_excess = (0.0, None), (-1.0, None)
    for v, g in zip(x, got):
        v, g = float(v), float(g)
        if v > 700.0:
            continue
        e = rs.exp_rt_restated(mp, v, k)[0]
        err = float(abs(mp.mpf(g) * (e - 1) - 1))
        bound = 4e-16 * float(e / (e - 1)) + 2.3e-15
        if err > worst[0]:
            worst = (err, v)
        if err / bound > worst_excess[0]:
            worst_excess = (err / bound, v)
    print("planck_inv: %d points, worst relative error %.4g at x = %r; largest error / bound %.3f at x = %r"
          % ((x.size,) + worst + worst_excess))
    assert worst_excess[0] <= 1.0, worst_excess
    at700 = engine.rt_math("planck_inv", 700.0).view(np.uint64)
    beyond = x[x > 700.0]
    assert beyond.size == 3
    assert np.all(got[x > 700.0].view(np.uint64) == at700), beyond
    assert float(at700.view(np.float64)) >= TINY_NORMAL


def test_selector_and_arguments_are_checked():
    import ctypes as C
    from bart_amd import engine, transit_module as trm
    x, out = np.ones(4), np.zeros(4)
    L = trm.lib()
    for which in (-1, len(engine.RT_MATH), 99):
        assert L.bartrt_rt_math(which, trm._ptr(x), trm._ptr(out), 4) == -1         # BARTRT_EINVAL
        assert b"rt_math" in L.bartrt_last_error()
    assert L.bartrt_rt_math(0, None, trm._ptr(out), 4) == -1 and L.bartrt_rt_math(0, trm._ptr(x), None, 4) == -1
    assert L.bartrt_rt_math(0, trm._ptr(x), trm._ptr(out), -1) == -1
    assert L.bartrt_rt_math(0, None, None, 0) == 0 and np.all(out == 0.0)
    assert sorted(engine.RT_MATH.values()) == list(range(len(engine.RT_MATH)))
    with pytest.raises(ValueError):
        engine.rt_math("exp", x)
    assert C.sizeof(C.c_double) == x.itemsize


# ---- end to end, where the synthetic grid never goes -----------------------------------------------------------------
# The window of the per-layer optical-depth steps at the vertical ray.  Thin means at most 1e-3; the lower end is where
# the ORACLE's own noise in a difference of neighbouring transmittances, 2.2e-16 / step, reaches 1e-12, two orders
# under the tolerance: 2.2e-4 (which lies inside a window opened at 1e-5, so that is the one lower limit there is).
THIN_LO, THIN_HI = 2.2e-16 / 1e-12, 1e-3
FORMS = ["", "generic", "mono_ilp", "split", "quad"]       # BARTRT_KERNEL, as in tests/test_gpu_parity.py


def _temperatures(case, rng, lo, hi):
    L = len(case.press_bar)
    t = rng.uniform(lo + 200.0, hi - 200.0) + 150.0 * np.sin(np.linspace(0, rng.uniform(1, 6), L) + rng.uniform(0, 6))
    return np.clip(t, lo, hi)


def _layer_dtau(o, prof):
    """The oracle's own tau output of one profile as per-layer steps [W][L - 1] (vertical ray, from the top)."""
    _, tau, last = o.run(prof, want_tau=True)
    assert np.all(last == o.L - 1)          # toomuch is never reached: every layer is walked
    return np.diff(tau, axis=1)


def thin_case(path):
    """(case, profiles[2]): sixteen layers whose optical-depth steps all lie in [THIN_LO, THIN_HI] = [2.2e-4,
    1e-3], which the caller asserts.  synth's line forest spans e^+-6 from one wavenumber to the next, more
    than the window is wide whatever the abundances are, so the case carries a table of its own (smooth in wavenumber,
    temperature and pressure, a factor of two from end to end); the absorbers' abundances are then scaled layer by
    layer, by the same factor for the four of them, until the oracle's steps sit mid-window."""
    from bart_amd import synth
    from oracle import rt_oracle as orc
    c = synth.make_case(str(path), nlayers=16, nwave=70, cia=False, toomuch=10.0)
    M = len(c.opmol)

    def plane(l):
        tt = (c.tgrid[:, None, None] - 1500.0) / 1000.0
        m = np.arange(M)[None, :, None]
        w = c.wn[None, None, :]
        return np.exp(0.25 * np.sin(w / 7.0 + m) + (0.15 + 0.05 * np.cos(w / 5.0 + 2 * m)) * tt
                      + 0.03 * np.log10(c.press_bar[l]) * np.sin(w / 11.0) - 0.2 * m)
    synth.write_opacity(c.opacity, [synth.MOLECULES[m][0] for m in c.opmol], c.tgrid, c.press_bar * 1e6, c.wn,
                        plane_fn=plane)
    o = orc.OracleEngine(c.tcfg)
    target = float(np.sqrt(THIN_LO * THIN_HI))
    rng = np.random.default_rng(41)
    profs = []
    for _ in range(2):
        t = _temperatures(c, rng, 410.0, 2990.0)
        scale = np.full(len(t), 1e-6)               # atm layer order: bottom first; the oracle's tau runs from the top
        for _ in range(12):
            ab = c.abund0.copy()
            ab[:, 2:] *= scale[:, None]
            q = 1 - ab[:, 2:].sum(1)
            ab[:, 1], ab[:, 0] = 0.85 * q, 0.15 * q
            prof = c.profiles(t, ab).ravel()
            g = np.exp(np.log(_layer_dtau(o, prof)).mean(axis=0))       # [L - 1], step k joins layers k and k + 1 from the top
            f = np.ones(len(t))
            f[1:] *= np.sqrt(target / g)
            f[:-1] *= np.sqrt(target / g)
            scale *= f[::-1] ** 0.7
        profs.append(prof)
    return c, np.array(profs)


def far_infrared_case(path):
    """(case, profiles[2]): 20 .. 89 cm-1 at 2000 K and above: every Planck exponent is below 0.0641 < ln2 / 2, the
    piece of exp_rt the grid at 1000 cm-1 and up never evaluates (n = 0; e^x - 1 on the interpolant's exact 1 + r)."""
    from bart_amd import synth
    c = synth.make_case(str(path), nlayers=16, nwave=70, wnlow=20.0, wndelt=1.0, tlow=2000.0, thigh=3000.0)
    rng = np.random.default_rng(42)
    profs = []
    for _ in range(2):
        t = _temperatures(c, rng, 2000.0, 2990.0)
        ab = c.abund0.copy()
        for s in range(2, ab.shape[1]):
            ab[:, s] *= 10 ** rng.uniform(-2, 1)
        q = 1 - ab[:, 2:].sum(1)
        ab[:, 1], ab[:, 0] = 0.85 * q, 0.15 * q
        profs.append(c.profiles(t, ab).ravel())
    profs = np.array(profs)
    assert profs[:, :16].min() >= 2000.0
    assert 1.4387769 * c.wn.max() / profs[:, :16].min() < rs.LN2 / 2
    return c, profs


CHILD = ("import json, numpy as np, sys; sys.path.insert(0, %r)\n"
         "from bart_amd import engine, transit_module as trm\n"
         "tcfg, pfile, out = sys.argv[1:4]\n"
         "engine.init(tcfg); p = np.load(pfile); res, names = [], []\n"
         "for integ, cut in ((1, 'slant'), (0, 'slant'), (0, 'vertical'), (2, 'vertical')):\n"
         "    trm.set_integ(integ); trm.set_cut(cut)\n"
         "    engine.walked_begin(); res.append(engine.run_batch(p)); names.append(engine.walked_end()[2])\n"
         "np.save(out, np.array(res)); trm.free_memory()\n"
         "print('KERNELS' + json.dumps(names))\n" % ROOT)
RULES = ((1, "slant"), (0, "slant"), (0, "vertical"), (2, "vertical"))


@pytest.fixture(scope="module")
def thin(tmp_path_factory):
    """The thin column, its profiles and the oracle's spectra under each (rule, cut) the children run; computed once."""
    from oracle import rt_oracle as orc
    c, profs = thin_case(tmp_path_factory.mktemp("rtmath_thin"))
    o = orc.OracleEngine(c.tcfg)
    dt = np.concatenate([_layer_dtau(o, p).ravel() for p in profs])
    print("thin column: per-layer optical-depth steps %.3g .. %.3g" % (dt.min(), dt.max()))
    assert THIN_LO < dt.min() and dt.max() <= THIN_HI, (dt.min(), dt.max())
    assert 2.2e-16 / dt.min() < 1e-12           # (THIN_LO, said the way it is meant)
    refs = [orc.OracleEngine(c.tcfg, integ=integ, cut=cut).run_batch(profs) for integ, cut in RULES]
    pfile = os.path.join(c.dir, "p.npy")
    np.save(pfile, profs)
    return c, pfile, refs


@pytest.mark.parametrize("mode", FORMS)
def test_thin_column_under_every_kernel_form(thin, mode):
    """Every transmittance argument is within 0.1 of zero (sixteen layers of at most 1e-3, slant factor below 6) and
    neighbouring layers' transmittances differ by 2e-4 .. 6e-3 of themselves: the rule-0 sums are made of exactly the
    differences the interpolant's exact 1 + r is there for.  Default rule and cut, and the other rules, in one child
    per forced form (BARTRT_KERNEL is read once per process)."""
    import json
    c, pfile, refs = thin
    out = os.path.join(c.dir, "s_%s.npy" % (mode or "default"))
    env = dict(os.environ)
    env.pop("BARTRT_KERNEL", None)
    if mode:
        env["BARTRT_KERNEL"] = mode
    r = subprocess.run([sys.executable, "-c", CHILD, c.tcfg, pfile, out], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    names = json.loads([l for l in r.stdout.splitlines() if l.startswith("KERNELS")][0][7:])
    # the forced form is the one that ran (the name without its notes, as in tests/test_gpu_parity.py).  The
    # producer / consumer split exists for rules 0 and 2 under `cut vertical` only: under `cut slant` a forced split
    # runs the single-wave slant kernel (csrc/rt_launch.hpp, launch_rt_spec ends in launch_form_slant there)
    from test_gpu_parity import forced_kernel
    assert len(names) == len(RULES)
    for (integ, cut), name in zip(RULES, names):
        if mode:
            form = "mono_ilp" if (mode == "split" and cut == "slant") else mode
            assert name.split(" [")[0] == forced_kernel(form, integ, cut), (mode, integ, cut, name)
        else:
            assert name.startswith("rt_eclipse") and "generic" not in name, (integ, cut, name)
    if mode:
        assert any(forced_kernel(mode, i, c) == n.split(" [")[0] for (i, c), n in zip(RULES, names))
    got = np.load(out)
    worst = [float(np.abs(g / ref - 1).max()) for g, ref in zip(got, refs)]
    print("thin column, BARTRT_KERNEL=%r: worst relative difference per (rule, cut) %s; kernels %s"
          % (mode, ["%.3g" % w for w in worst], names))
    for g, ref in zip(got, refs):
        assert np.all(np.isfinite(g)) and g.min() > 0
        np.testing.assert_allclose(g, ref, rtol=RTOL)


def test_far_infrared_hot_column(tmp_path):
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    c, profs = far_infrared_case(tmp_path)
    engine.init(c.tcfg)
    try:
        for integ, cut in RULES:
            trm.set_integ(integ); trm.set_cut(cut)
            ref = orc.OracleEngine(c.tcfg, integ=integ, cut=cut).run_batch(profs)
            got = engine.run_batch(profs)
            print("far infrared, rule %d, cut %s: worst relative difference %.3g" % (integ, cut, np.abs(got / ref - 1).max()))
            np.testing.assert_allclose(got, ref, rtol=RTOL)
    finally:
        trm.free_memory()
