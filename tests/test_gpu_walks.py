"""GPU: MC3's other two walks.  `mrw` in the resident loop (bartrt_mcmc_opts.walk = 2) by the single-step replay of
tests/test_gpu_mcmc_resident.py -- its replay function, given the restatement of the mrw move -- and the model grids
of `walk = unif` (bartrt_grid_run, csrc/grid.hip): samples against the restatement, every model row against the step
on the same rows in one call of the same batch size, rejected rows, chunks, `first`, refusals and the command line.
The engine is the small synthetic one of test_gpu_mcmc_resident.py (its fixture and helpers are imported)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_mcmc_resident as T  # noqa: E402
import walks_restate as wr  # noqa: E402
from test_gpu_mcmc_resident import W  # noqa: E402,F401  (the module-scoped worker fixture)

pytestmark = pytest.mark.gpu

STEP = np.array([0.005, 0.0, 0.0, 0.0, 0.0005, 0.02, -6.0])     # fixed ones, and the last shared with the sixth
N = 40


def mrw_cfg(data, nch, nsteps=N, **over):
    return T.scfg(data, nch, "mrw", stepsize=STEP, numit=nsteps * nch, **over)


def mrw_problem(cfg):
    return wr.MrwProblem(cfg.params, cfg.pmin, cfg.pmax, cfg.stepsize, cfg.data, cfg.uncert, cfg.nchains, cfg.seed,
                         cfg.prior, cfg.priorlow, cfg.priorup)


@pytest.mark.parametrize("nch", [1, 3, 65])
def test_mrw_replay_and_thinning(W, nch, monkeypatch):
    """40 iterations: every decision of the unthinned run replayed from the device's own previous state (T.replay,
    with the mrw move restated), then the run with thin 3 holds rows 2, 5, ... and the last of it, bit for bit."""
    monkeypatch.setattr(T, "NSTEPS", N)
    monkeypatch.setattr(T, "problem", mrw_problem)
    cfg = mrw_cfg(W.data, nch)
    res = T.run(W, cfg)
    n = T.replay(W, cfg, res)
    assert n["accepted"] > 0
    assert np.all(res["chain"][:, :, [1, 2, 3]] == np.array(T.P0)[[1, 2, 3]])
    assert np.array_equal(res["chain"][:, :, 6], res["chain"][:, :, 5]) and np.ptp(res["chain"][:, :, 5]) > 0
    assert np.array_equal(res["models"], T.models_of(W, res["chain"]))
    thin = T.run(W, mrw_cfg(W.data, nch, thinning=3))
    rows = list(range(2, N, 3)) + [N - 1]
    assert thin["chain"].shape == (nch, 14, 7) and rows[-2:] == [38, 39]
    for key in ("chain", "chisq", "models"):
        assert np.array_equal(thin[key], res[key][:, rows]), key
    # not the demc chain under another name
    assert not np.array_equal(res["chain"], T.run(W, T.scfg(W.data, nch, "demc", stepsize=STEP, numit=N * nch))["chain"])


def test_mrw_resume_same_bytes(W):
    whole = T.run(W, mrw_cfg(W.data, 5, 24, thinning=3))
    head = T.run(W, mrw_cfg(W.data, 5, 12, thinning=3))
    tail = T.run(W, mrw_cfg(W.data, 5, 24, thinning=3), first=12, start=head["chain"][:, -1])
    assert whole["chain"].shape == (5, 8, 7) and tail["done"] == 12
    for key in ("chain", "chisq", "models"):
        both = np.concatenate([head[key], tail[key]], axis=1)
        assert both.tobytes() == whole[key].tobytes(), key
    assert head["accepted"] + tail["accepted"] == whole["accepted"] > 0


def test_mrw_refusals(W):
    from bart_amd import sampler, transit_module as trm
    lib = trm.lib()
    cfg = T.scfg(W.data, 4, "demc")
    args = [np.ascontiguousarray(v, float) for v in (cfg.params, cfg.pmin, cfg.pmax, cfg.stepsize, cfg.data, cfg.uncert)]
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    chain, chis = np.zeros((4, 3, 7)), np.zeros((4, 3))

    def call(walk):
        opts = sampler.McmcOpts(size=C.sizeof(sampler.McmcOpts), seed=1, walk=walk)
        return lib.bartrt_mcmc_run_resident(4, 7, C.c_long(3), *[p(v) for v in args[:4]], 3, p(args[4]), p(args[5]),
                                            C.cast(C.byref(opts), C.c_void_p), p(chain), p(chis), None, None, None)
    assert call(0) == 0 and call(2) == 0
    assert call(3) == -1 and b"bartrt_grid_run" in lib.bartrt_last_error()            # BARTRT_EINVAL
    assert call(7) == -1 and b"walk = 7" in lib.bartrt_last_error()
    with pytest.raises(ValueError, match="run_grid"):
        sampler.run_resident(W.worker, T.scfg(W.data, 4, "unif"))


# ---- model grids ------------------------------------------------------------------------------------------------------
PMIN = np.array([-5.0, -2.0, -2.0, 0.0, 0.55, -3.0, -9.0])
PMAX = np.array([-1.0, 1.0, 1.0, 1.0, 1.2, 0.0, 1.5])
GSTEP = np.array([0.01, 0.0, 0.0, 0.0, 0.001, 0.05, -6.0])
NIT, SEED = 7, 17


def gcfg(nrows, niter=NIT, seed=SEED, **over):
    from bart_amd import sampler
    kw = dict(params=np.array(T.P0), pmin=PMIN, pmax=PMAX, stepsize=GSTEP, data=np.zeros(0), uncert=np.zeros(0),
              nchains=nrows, numit=niter * nrows, walk="unif", seed=seed)
    kw.update(over)
    return sampler.SamplerConfig(**kw)


def restated(cfg, t0=0, niter=NIT):
    """[nrows, niter, npars] from tests/walks_restate.py"""
    rows = [wr.grid_samples(cfg.seed, t, cfg.nchains, cfg.params, cfg.pmin, cfg.pmax, cfg.stepsize)
            for t in range(t0, t0 + niter)]
    return np.array(rows).swapaxes(0, 1)


_REF = {}


def reference(W, cfg, key):
    """The step on every iteration's rows in one call of the same batch size, computed once per case and shared:
    band [nrows, niter, nf] and status from bartrt_step_batch, spectra [nrows, niter, nwave] from the batched
    spectrum call."""
    import torch
    from bart_amd import engine
    if key not in _REF:
        par = restated(cfg, 0, int(np.ceil(cfg.numit / cfg.nchains)))
        band, status, spec = [], [], []
        for t in range(par.shape[1]):
            rows = np.ascontiguousarray(par[:, t])
            b, s = engine.step_batch(rows, W.worker.nfilters)
            _, s2, sp = engine.step_batch_dev(torch.tensor(rows, dtype=torch.float64, device="cuda"),
                                              W.worker.nfilters, want_spec=True)
            torch.cuda.synchronize()
            assert np.array_equal(s, s2.cpu().numpy())
            band.append(b), status.append(s), spec.append(sp.cpu().numpy())
        ref = dict(params=par, band=np.stack(band, 1), status=np.stack(status, 1), spec=np.stack(spec, 1))
        for v in ref.values():
            v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def check_rows(got, ref, spectra, f32):
    want = ref["spec" if spectra else "band"].copy()
    want[ref["status"] != 0] = -1.0
    if f32:
        assert got["models"].dtype == np.float32
        want = want.astype(np.float32)
    assert got["models"].shape == want.shape
    assert got["models"].tobytes() == want.tobytes()
    assert np.array_equal(got["status"], ref["status"])
    assert got["params"].tobytes() == ref["params"].tobytes()
    assert got["nbad"] == [int((ref["status"] == k).sum()) for k in (1, 2, 3)]


@pytest.mark.parametrize("nrows", [1, 3, 65])
def test_grid_values(W, nrows):
    """7 iterations in chunks of 3: params are the restated samples and bartrt_grid_draws', every f64 row is the
    step's on that iteration's rows bit for bit, f32 rows are np.float32 of them, statuses are the step's."""
    from bart_amd import sampler
    cfg = gcfg(nrows, modelper=3)
    ref = reference(W, cfg, ("plain", nrows))
    assert (ref["status"] == 0).any()
    for t in range(NIT):
        dev = sampler.grid_draws(cfg.seed, t, nrows, cfg.params, cfg.pmin, cfg.pmax, cfg.stepsize)
        assert dev.tobytes() == np.ascontiguousarray(ref["params"][:, t]).tobytes(), t
    for spectra in (False, True):
        for f32 in (False, True):
            got = sampler.run_grid(W.worker, cfg, spectra=spectra, f32=f32)
            assert got["models"].shape == (nrows, NIT, W.worker.nwave if spectra else W.worker.nfilters)
            check_rows(got, ref, spectra, f32)
    # whole spectra are not band fluxes, and a valid row is not the sentinel
    ok = ref["status"] == 0
    assert np.all(ref["spec"][ok] != -1.0) and np.all(ref["band"][ok] != -1.0)


# chosen on the CPU with oracle/pyhalf.py's step_profiles on the restated samples of this synthetic case: with beta in
# [1, 3] and seed 4, 205 of the 65 x 7 rows (45 %) leave the temperature bounds [400, 3000] K
HOT = dict(seed=4, pmin=np.array([-5.0, -2.0, -2.0, 0.0, 1.0, -3.0, -9.0]),
           pmax=np.array([-1.0, 1.0, 1.0, 1.0, 3.0, 0.0, 1.5]))


def test_grid_rejected_rows(W):
    from bart_amd import sampler
    cfg = gcfg(65, modelper=3, **HOT)
    ref = reference(W, cfg, "hot")
    bad = ref["status"] != 0
    assert 0.25 * bad.size <= bad.sum() <= 0.75 * bad.size, (int(bad.sum()), bad.size)     # both kinds occur
    assert (ref["status"][bad] == 1).all()
    for spectra in (False, True):
        for f32 in (False, True):
            got = sampler.run_grid(W.worker, cfg, spectra=spectra, f32=f32)
            check_rows(got, ref, spectra, f32)
            assert np.all(got["models"][bad] == -1.0) and np.all(got["models"][~bad] != -1.0)
            assert got["nbad"] == [int(bad.sum()), 0, 0]


def test_grid_chunks_and_sink(W):
    from bart_amd import sampler
    cfg = gcfg(3, modelper=3)
    ref = reference(W, cfg, ("plain", 3))
    seen, parts = [], []

    def sink(k, t0, params, status, models):
        seen.append((k, t0, len(params)))
        assert params.shape == (len(params), 3, 7) and status.shape == (len(params), 3)
        parts.append((params.copy(), status.copy(), models.copy()))
    out = sampler.run_grid(W.worker, cfg, sink=sink)
    assert seen == [(0, 0, 3), (1, 3, 3), (2, 6, 1)]
    assert out["models"] == 21 and not out["stopped"]
    cat = lambda j: np.concatenate([p[j] for p in parts], axis=0).swapaxes(0, 1)
    assert cat(0).tobytes() == ref["params"].tobytes() and np.array_equal(cat(1), ref["status"])
    whole = np.ascontiguousarray(cat(2))
    # chunk = 0: one call with all 7 iterations and the same bytes
    seen0, parts0 = [], []
    sampler.run_grid(W.worker, gcfg(3, modelper=0), sink=lambda k, t0, p, s, m: (seen0.append((k, t0, len(p))),
                                                                                 parts0.append(m.copy()))[0])
    assert seen0 == [(0, 0, 7)]
    assert np.ascontiguousarray(parts0[0].swapaxes(0, 1)).tobytes() == whole.tobytes()
    # a sink that stops at k = 0: the call ends with its value, and no call for k = 2 follows
    calls = []
    out = sampler.run_grid(W.worker, cfg, sink=lambda k, *a: (calls.append(k), True)[1])
    assert out["stopped"] and calls == [0]
    from bart_amd import transit_module as trm
    lib = trm.lib()
    ks = []
    cb = sampler.SINK(lambda k, t0, n, a, b, c, u: (ks.append(k), 5)[1])
    opts = sampler.GridOpts(size=C.sizeof(sampler.GridOpts), seed=SEED, chunk=3, spectra=1, sink=C.cast(cb, C.c_void_p))
    p = lambda v: np.ascontiguousarray(v, float).ctypes.data_as(C.c_void_p)
    rc = lib.bartrt_grid_run(3, 7, C.c_long(7), p(cfg.params), p(PMIN), p(PMAX), p(GSTEP),
                             C.cast(C.byref(opts), C.c_void_p), None)
    assert rc == 5 and ks == [0] and b"sink" in lib.bartrt_last_error()
    # an exception in the sink ends the run and comes out of run_grid
    def boom(*a):
        raise KeyError("boom")
    with pytest.raises(KeyError, match="boom"):
        sampler.run_grid(W.worker, cfg, sink=boom)


def test_grid_first(W):
    """first = 3, four iterations: iterations 3 .. 6 of the whole run, bit for bit."""
    from bart_amd import sampler
    for nrows in (3, 65):
        cfg = gcfg(nrows, modelper=3)
        ref = reference(W, cfg, ("plain", nrows))
        got = sampler.run_grid(W.worker, cfg, first=3)
        assert got["models"].shape == (nrows, 4, W.worker.nwave)
        assert got["params"].tobytes() == np.ascontiguousarray(ref["params"][:, 3:]).tobytes()
        want = ref["spec"][:, 3:].copy()
        want[ref["status"][:, 3:] != 0] = -1.0
        assert got["models"].tobytes() == want.tobytes()
        assert np.array_equal(got["status"], ref["status"][:, 3:])


def test_grid_refusals(W):
    from bart_amd import sampler, transit_module as trm
    lib = trm.lib()
    p = lambda v: np.ascontiguousarray(v, float).ctypes.data_as(C.c_void_p)
    cb = sampler.SINK(lambda *a: 0)

    def call(nrows=3, pmin=PMIN, sink=cb, nsteps=2):
        opts = sampler.GridOpts(size=C.sizeof(sampler.GridOpts), seed=1, chunk=1,
                                sink=C.cast(sink, C.c_void_p) if sink is not None else None)
        return lib.bartrt_grid_run(nrows, 7, C.c_long(nsteps), p(T.P0), p(pmin), p(PMAX), p(GSTEP),
                                   C.cast(C.byref(opts), C.c_void_p), None)
    assert call() == 0
    assert call(sink=None) == -1 and b"sink" in lib.bartrt_last_error()                 # BARTRT_EINVAL
    over = PMIN.copy()
    over[4] = PMAX[4] + 0.1
    assert call(pmin=over) == -1 and b"pmin[4]" in lib.bartrt_last_error()
    fixed = PMIN.copy()
    fixed[1] = PMAX[1] + 1.0                                                          # a fixed parameter's box is not read
    assert call(pmin=fixed) == 0
    assert call(nrows=0) == -1 and b"nrows" in lib.bartrt_last_error()
    assert call(nsteps=0) == -1
    with pytest.raises(trm.TransitError, match="pmin"):
        sampler.grid_draws(1, 0, 3, T.P0, over, PMAX, GSTEP)


def test_retrieve_writes_the_grid(W, tmp_path):
    """`retrieve` on a walk = unif configuration without data.  LAST in this module: retrieve.main makes workers of
    its own, after which the module's worker is rebuilt."""
    from bart_amd import BARTfunc, retrieve, sampler, synthcfg
    line = lambda v: " ".join(repr(float(x)) for x in v)
    want = sampler.run_grid(W.worker, gcfg(5, modelper=3))
    bands = sampler.run_grid(W.worker, gcfg(5, modelper=3), spectra=False)
    nwave, nf = W.worker.nwave, W.worker.nfilters

    def write(name, **over):
        case, cfg = synthcfg.make_worker_case(str(tmp_path / name), **T.CASE)
        head, tail = open(cfg).read().split("[MCMC]", 1)
        kw = dict(params=line(T.P0), pmin=line(PMIN), pmax=line(PMAX), stepsize=line(GSTEP), nchains="5", numit="35",
                  walk="unif", seed=str(SEED), modelper="3", savemodel="grid.npy")
        kw.update(over)
        keep = [l for l in tail.split("\n") if l.split("=")[0].strip() not in kw]
        with open(cfg, "w") as f:
            f.write(head + "[MCMC]\n" + "\n".join("%s = %s" % kv for kv in kw.items()) + "\n" + "\n".join(keep))
        assert "data" not in kw and not any(l.startswith("data") for l in keep)
        return cfg

    W.worker.close()
    W.worker = None
    try:
        out = str(tmp_path / "o3")
        retrieve.main(["-c", write("m3"), "--out", out])
        assert np.load(os.path.join(out, "output.npy")).tobytes() == want["params"].tobytes()
        assert np.load(os.path.join(out, "output.npy")).shape == (5, 7, 7)
        assert np.array_equal(np.load(os.path.join(out, "status.npy")), want["status"])
        files = sorted(os.listdir(os.path.join(out, "grid")))
        assert files == ["grid_00000.npy", "grid_00001.npy", "grid_00002.npy"]
        parts = [np.load(os.path.join(out, "grid", f)) for f in files]
        assert [v.shape for v in parts] == [(5, nwave, 3), (5, nwave, 3), (5, nwave, 1)]
        assert np.concatenate(parts, axis=2).tobytes() == np.ascontiguousarray(want["models"].transpose(0, 2, 1)).tobytes()
        log = open(os.path.join(out, "MCMC.log")).read()
        assert "35 models in" in log and "Bad iterations due to temperature" in log
        out = str(tmp_path / "o0")
        retrieve.main(["-c", write("m0", modelper="0"), "--out", out])
        one = np.load(os.path.join(out, "grid.npy"))
        assert one.shape == (5, nwave, 7) and one.tobytes() == np.concatenate(parts, axis=2).tobytes()
        out = str(tmp_path / "ob")
        retrieve.main(["-c", write("mb", modelper="0"), "--out", out, "--grid-bands", "--grid-f32"])
        one = np.load(os.path.join(out, "grid.npy"))
        assert one.shape == (5, nf, 7) and one.dtype == np.float32
        assert np.array_equal(one, bands["models"].transpose(0, 2, 1).astype(np.float32))
        for extra in (["--resume", "--resident"], ["--leastsq"], ["--python-loop"]):
            with pytest.raises(SystemExit):
                retrieve.main(["-c", write("bad"), "--out", out, *extra])
        with pytest.raises(SystemExit):
            retrieve.main(["-c", write("gx", grexit="True"), "--out", out])
    finally:
        W.worker = BARTfunc.Worker(W.wcfg)
