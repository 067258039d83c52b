"""A call's result does not depend on what was called before it.

Two hand-overs between calls are documented and are the only exceptions: the per-walker radius / cloud-top /
scattering values that bartrt_step_profiles_dev leaves for the NEXT run, and the batch that
bartrt_prefetch_profiles_dev names for the run after the next.  Everything else a launch is asked to do (the fused
step's preparation, its overrides, the optical-depth and intensity outputs) belongs to that launch alone.

Every reference below is the first call after a fresh engine.init (a getter: after the one host-buffer run it
re-runs); the sequence then makes the same calls on ONE engine, in an order chosen so that each follows a call that
could leak into it, and compares bit for bit -- both sides are the same library's own results, so there is no
tolerance.  Eclipse geometry under the default conventions, three walkers on the 777-sample case (13 single-wave
columns): the layer-parallel forms and the preparation folded into the RT launch are on the path.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NW = 3                               # walkers
IDX0, NPTS = [100, 400], [40, 60]    # two filters of a few dozen samples
RPRS = 0.1


def _init(case):
    from bart_amd import engine
    engine.init(case.tcfg)
    rng = np.random.default_rng(5)
    tot = sum(NPTS)
    # the isothermal model; radius, cloud top and scattering value travel with every walker
    engine.step_setup(None, 0.0, 1e9, case.abund0, [], IDX0, NPTS, rng.uniform(0.5, 1.5, tot) / tot,
                      rng.uniform(1e5, 2e5, tot), RPRS, pttype=1)
    engine.step_set_extras(1, 1, 1)


def _fresh(case, call):
    """call() as the first thing a new engine does."""
    from bart_amd import transit_module as trm
    _init(case)
    try:
        return call()
    finally:
        trm.free_memory()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.double)).cuda()


def _intensity(walker):
    from bart_amd import engine, transit_module as trm
    lo, hi = engine.local_range()
    nang = trm.check(trm.lib().bartrt_get_nangles())
    out = np.zeros((nang, hi - lo))
    trm.check(trm.lib().bartrt_get_intensity_of(int(walker), trm._ptr(out), nang, hi - lo))
    return out


def _step_dev(params):
    from bart_amd import engine
    band, status, spec = engine.step_batch_dev(_dev(params), len(NPTS), want_spec=True)
    return band.cpu().numpy(), status.cpu().numpy(), spec.cpu().numpy()


def _run_dev(prof, **kw):
    from bart_amd import engine
    return engine.run_batch_dev(prof if hasattr(prof, "is_cuda") else _dev(prof), **kw).cpu().numpy()


def _profiles_then_run(params):
    """-> (profiles as the converter wrote them, the spectra of the run that takes the walkers' extras)."""
    from bart_amd import engine
    prof, _ = engine.step_profiles_dev(_dev(params))
    spec = engine.run_batch_dev(prof).cpu().numpy()
    return prof.cpu().numpy(), spec


@pytest.fixture(scope="module")
def inputs(small_case):
    c = small_case
    base = c.profiles().ravel()
    L = len(c.press_bar)

    def scaled(f):
        p = np.tile(base, (NW, 1))
        p[:, :L] *= np.asarray(f)[:, None]      # the temperatures, every walker its own
        return p
    r0 = float(c.keys["refradius"])
    # [T, radius km, log10 cloud top bar, scattering value]: radii 5 % off the cfg's, a cloud deck in the column
    params = np.array([[1300.0, 1.05 * r0, -1.0, 1.0],
                       [1500.0, 0.95 * r0, -2.0, 1.0],
                       [1700.0, 1.05 * r0, -0.5, 1.0]])
    return {"P": scaled([1.0, 0.9, 1.1]), "A": scaled([0.95, 1.05, 1.0]), "B": scaled([1.02, 0.98, 0.93]),
            "params": params}


@pytest.fixture(scope="module")
def refs(small_case, inputs):
    from bart_amd import engine
    c, P, A, B, params = small_case, inputs["P"], inputs["A"], inputs["B"], inputs["params"]
    r = {}
    r["run_P"] = _fresh(c, lambda: engine.run_batch(P, want_ok=True))
    r["step_dev"] = _fresh(c, lambda: _step_dev(params))
    r["dev_P"] = _fresh(c, lambda: _run_dev(P))
    r["tau_1"] = _fresh(c, lambda: (engine.run_batch(P), engine.get_tau(walker=1))[1])
    r["intens_1"] = _fresh(c, lambda: (engine.run_batch(P), _intensity(1))[1])
    r["prof_Q"], r["dev_Q_over"] = _fresh(c, lambda: _profiles_then_run(params))
    r["dev_Q"] = _fresh(c, lambda: _run_dev(r["prof_Q"]))
    r["dev_A"] = _fresh(c, lambda: _run_dev(A))
    r["dev_B"] = _fresh(c, lambda: _run_dev(B))
    r["step_host"] = _fresh(c, lambda: engine.step_batch(params, len(NPTS)))
    return r


def test_the_references_tell_the_cases_apart(refs):
    """What the sequence compares must be able to differ, or equality proves nothing."""
    assert np.all(refs["run_P"][1] == 1) and np.all(np.isfinite(refs["run_P"][0]))
    assert np.all(refs["step_dev"][1] == 0)
    # the walkers' own radius and cloud top against the cfg's, on the same profiles
    assert not np.array_equal(refs["dev_Q_over"], refs["dev_Q"])
    assert not np.array_equal(refs["dev_A"], refs["dev_B"])
    assert not np.array_equal(refs["step_dev"][2], refs["dev_Q"])
    assert np.any(refs["tau_1"][0] > 0) and np.any(refs["intens_1"] > 0)


def _eq(got, want):
    if isinstance(want, tuple):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            _eq(g, w)
    else:
        assert np.array_equal(got, want)


def test_calls_in_sequence_on_one_engine(small_case, inputs, refs):
    from bart_amd import engine, transit_module as trm
    P, A, B, params = inputs["P"], inputs["A"], inputs["B"], inputs["params"]
    _init(small_case)
    try:
        dP, dA, dB = _dev(P), _dev(A), _dev(B)
        # 1. host buffers, zero-copy size
        _eq(engine.run_batch(P, want_ok=True), refs["run_P"])
        # 2. the fused step: its preparation launch and the walkers' extras
        _eq(_step_dev(params), refs["step_dev"])
        # 3. ... are gone
        _eq(_run_dev(dP), refs["dev_P"])
        # 4. the optical-depth output of one walker, and nothing of it in the run that follows
        engine.run_batch(P)
        _eq(engine.get_tau(walker=1), refs["tau_1"])
        _eq(engine.run_batch(P, want_ok=True), refs["run_P"])
        # 5. the intensity output of one walker, likewise
        _eq(_intensity(1), refs["intens_1"])
        _eq(_run_dev(dP), refs["dev_P"])
        # 6. first hand-over: the run after step_profiles_dev takes the walkers' extras, the one after that does not
        prof, spec = _profiles_then_run(params)
        _eq(prof, refs["prof_Q"])
        _eq(spec, refs["dev_Q_over"])
        _eq(_run_dev(prof), refs["dev_Q"])
        # ... and any run takes them, a getter's included: the run after it finds none
        engine.run_batch(P)
        dQ, _ = engine.step_profiles_dev(_dev(params))
        engine.get_tau(walker=1)
        _eq(_run_dev(dQ), refs["dev_Q"])
        # 7. second hand-over: the batch named for the run after the next
        _eq(_run_dev(dA, next_prof=dB), refs["dev_A"])
        _eq(_run_dev(dB), refs["dev_B"])
        # ... with a call in between that takes no part in it.  A device-buffer call keeps no profile: the getter
        # refuses before it launches anything
        _eq(_run_dev(dA, next_prof=dB), refs["dev_A"])
        with pytest.raises(trm.TransitError, match="no host-buffer spectrum"):
            engine.get_tau()
        _eq(_run_dev(dB), refs["dev_B"])
        # ... and a getter that does launch: it cannot carry the request, which is dropped, not kept for later
        engine.run_batch(P)
        trm.check(trm.lib().bartrt_prefetch_profiles_dev(C.c_void_p(dB.data_ptr()), NW))
        _eq(engine.get_tau(walker=1), refs["tau_1"])
        _eq(_run_dev(dA), refs["dev_A"])
        _eq(_run_dev(dB), refs["dev_B"])
        # 8. the pinned buffer holds parameters after a host step: the getters must not re-run it as a profile
        engine.run_batch(P)
        _eq(engine.step_batch(params, len(NPTS)), refs["step_host"])
        with pytest.raises(trm.TransitError, match="no host-buffer spectrum"):
            engine.get_tau()
        _eq(engine.run_batch(P, want_ok=True), refs["run_P"])
    finally:
        trm.free_memory()
