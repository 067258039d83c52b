"""GPU: the batched multi-start fit through the engine (bartrt_fit, csrc/fit.hip) on the worker case of
tests/test_gpu_mcmc_resident.py with eight filters.

The strong test is a SINGLE-ITERATION REPLAY: every record of the device's trace is rebuilt by tests/fit_restate.py
from the device's own previous record, its models from engine.step_batch -- Jacobian rows, frozen set, damped solves
(numpy.linalg.solve), trial rows, the pick and its counters.  The replay solves from its own A and g; the device's
trial point (the trace's next x) must lie within the restatement's bound of the replay's for the rung the device took,
and rung, status, iteration count and nbad must be equal, at every row."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_restate as fr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOLS = ("H2O", "CH4")
P0 = (-2.0, 0.0, 1.0, 0.0, 0.98, -0.5, -0.5)
CASE = dict(nwave=300, wnlow=1200.0, opmol=MOLS, molfit=MOLS, params=P0, nfilters=8)
PMIN = np.array([-5.0, -2.0, -2.0, 0.0, 0.55, -9.0, -9.0])
PMAX = np.array([-1.0, 1.0, 1.0, 1.0, 1.2, 1.5, 1.5])
STEP = np.array([0.01, 0.0, 0.0, 0.0, 0.001, 0.05, 0.05])          # four free parameters
MAXITER = 30


class Shared:
    worker = None
    wcfg = None
    data = None


@pytest.fixture(scope="module")
def W(tmp_path_factory):
    from bart_amd import BARTfunc, synthcfg
    case, cfg = synthcfg.make_worker_case(str(tmp_path_factory.mktemp("fit")), **CASE)
    Shared.wcfg = BARTfunc.WorkerConfig.from_cfg(cfg)
    Shared.worker = BARTfunc.Worker(Shared.wcfg)
    Shared.data = Shared.worker.step(np.array(P0))[0].copy()
    yield Shared
    if Shared.worker is not None:
        Shared.worker.close()


def scfg(data, **over):
    from bart_amd import sampler
    kw = dict(params=np.array(P0), pmin=PMIN.copy(), pmax=PMAX.copy(), stepsize=STEP.copy(), data=data,
              uncert=0.01 * np.abs(data), nchains=4, numit=40, burnin=2, walk="snooker", seed=9, grtest=False)
    kw.update(over)
    return sampler.SamplerConfig(**kw)


def problem(cfg, **opts):
    return fr.Problem(cfg.pmin, cfg.pmax, cfg.stepsize, cfg.data, cfg.uncert, cfg.prior, cfg.priorlow, cfg.priorup,
                      maxiter=opts.get("maxiter", MAXITER), **{k: v for k, v in opts.items() if k != "maxiter"})


def run(W, cfg, starts, **opts):
    from bart_amd import fit
    opts.setdefault("maxiter", MAXITER)
    return fit.fit(W.worker, cfg, starts=np.array(starts, float), **opts)


def model_of(nf):
    from bart_amd import engine
    return lambda rows: engine.step_batch(np.ascontiguousarray(np.atleast_2d(rows), float), nf)


def replay(cfg, res, starts, **opts):
    """-> dict(iterations, nbad [4], frozen: per start the frozen sets met)."""
    P, call = problem(cfg, **opts), model_of(len(cfg.data))
    np_, tr = P.npars, res["trace"]
    total, out = [0, 0, 0, 0], dict(iterations=0, frozen=[])
    worst = 0.0
    for s, start in enumerate(np.atleast_2d(starts)):
        band, status = call(P.shared(start))
        st = P.pick0(start, band[0], status[0])
        if 1 <= int(status[0]) <= 3:
            total[int(status[0])] += 1
        assert np.array_equal(tr[s, 0, :np_], st["x"]) and tr[s, 0, np_ + 3] == st["status"], (s, tr[s, 0], st)
        assert st["status"] == fr.NO_START or abs(tr[s, 0, np_] - st["chisq"]) <= 1e-13 * st["chisq"]
        D, it, frozen = np.zeros(np_), 0, []
        while st["status"] == fr.RUNNING:
            it += 1
            # the device's previous record is the state
            st["x"], st["chisq"], st["lam"] = tr[s, it - 1, :np_].copy(), tr[s, it - 1, np_], tr[s, it - 1, np_ + 1]
            st["cur"] = call(st["x"])[0][0]
            pband, pstatus = call(P.jacobian_rows(st["x"]))
            sol = P.solve(st["x"], st["lam"], D, st["cur"], pband, pstatus)
            D = sol["D"]
            frozen.append(list(sol["frozen"]))
            tband, tstatus = call(sol["trial"])
            new, nb, margin = P.pick(st, it, sol["trial"], sol["valid"], tband, tstatus)
            total = [a + b + c for a, b, c in zip(total, sol["nbad"], nb)]
            rec = tr[s, it]
            out["iterations"] += 1
            assert rec[np_ + 2] == new["rung"] and rec[np_ + 3] == new["status"], (s, it, rec[np_:], new, margin)
            if new["rung"] >= 0:
                k = new["rung"]
                assert sol["cond"][k] <= 1e8, (s, it, k, sol["cond"][k])
                err = np.abs(rec[:np_] - sol["trial"][k])
                assert np.all(err <= sol["tol"][k]), (s, it, k, err, sol["tol"][k])
                worst = max(worst, float(np.max(err / np.maximum(sol["tol"][k], 1e-300))))
                assert abs(rec[np_] - new["chisq"]) <= 1e-9 * abs(new["chisq"]) + 1e-20, (s, it, rec[np_], new["chisq"])
            else:
                assert np.array_equal(rec[:np_], st["x"]) and rec[np_] == st["chisq"]
            assert abs(rec[np_ + 1] - new["lam"]) <= 1e-14 * new["lam"], (s, it, rec[np_ + 1], new["lam"])
            st = new
        assert it == res["niter"][s] and st["status"] == res["status"][s], (s, it, res["niter"][s], res["status"][s])
        out["frozen"].append(frozen)
    assert total == res["nbad"], (total, res["nbad"])
    out["nbad"] = total
    print("replay: %d iterations, largest trial-point error / bound %.3g, nbad %r" % (out["iterations"], worst, total))
    return out


def jittered(n, seed=5):
    from bart_amd import fit
    return fit.default_starts(scfg(np.ones(8)), n, seed)


def test_single_iteration_replay(W):
    cfg = scfg(W.data * (1.0 + 0.01 * np.array([1, -1, 2, 0, -2, 1, -1, 0.5])))
    starts = jittered(3)
    res = run(W, cfg, starts)
    n = replay(cfg, res, starts)
    assert n["iterations"] >= 3 and (res["status"] != fr.RUNNING).all()
    assert np.all(res["trace"][:, :, [1, 2, 3]] == np.array(P0)[[1, 2, 3]])
    # three free parameters, a shared one, a prior, eight rungs
    z = np.zeros(7)
    prior, lo, up = z.copy(), z.copy(), z.copy()
    prior[5], lo[5], up[5] = -0.45, 0.02, 0.0
    step = STEP.copy()
    step[6] = -6.0
    cfg2 = scfg(cfg.data, stepsize=step, prior=prior, priorlow=lo, priorup=up)
    res2 = run(W, cfg2, starts[:2], nrungs=8)
    replay(cfg2, res2, starts[:2], nrungs=8)
    assert np.array_equal(res2["trace"][:, :, 6], res2["trace"][:, :, 5]) and np.ptp(res2["trace"][:, :, 5]) > 0


def test_recovery(W):
    """Noise-free data of the engine at P0: every start that ends converged has chisq <= 1e-8 of its starting value;
    the start at the true point does, and so does at least one start away from it."""
    from bart_amd import fit
    # The start at the true point and three jittered by thirty stepsizes: their starting chisq is 27 to 750, so 1e-8
    # of it lies above the 1e-10 to 1e-7 at which the forward differences let a start call itself converged.
    cfg = scfg(W.data)
    starts = fit.default_starts(scfg(W.data, stepsize=30.0 * STEP), 4, seed=5)
    assert np.array_equal(starts[0], P0) and np.all(np.abs(starts[1:] - np.array(P0))[:, STEP > 0].max(axis=1) > 0)
    P, call = problem(cfg), model_of(8)

    def holds(status, chisq, c0, who):
        conv = np.array(status) == fr.CONVERGED
        print("%s: status %r chisq %r from %r" % (who, list(status), list(chisq), list(c0)))
        assert conv[0] and conv[1:].any(), (who, status)
        assert np.all(np.array(chisq)[conv] <= 1e-8 * np.array(c0)[conv]), (who, chisq, c0)
    runs = [P.run(call, s) for s in starts]                       # the restatement first
    holds([r["status"] for r in runs], [r["chisq"] for r in runs], [r["trace"][0]["chisq"] for r in runs], "restatement")
    res = run(W, cfg, starts)
    holds(res["status"].tolist(), res["chisq"].tolist(), res["trace"][:, 0, 7].tolist(), "device")
    assert (res["niter"][1:] > 0).all() and res["niter"][0] == 0
    assert np.array_equal(res["bestp"], res["best"][np.argmin(res["chisq"])])


def test_rejections_and_a_box_that_cuts_the_path(W):
    from bart_amd import engine
    # a start the T(p) model rejects (temperature out of [tmin, tmax]): the first beta of a ladder that it refuses
    bad = None
    for beta in (1.2, 0.55, 1.6, 0.3, 2.5, 4.0, 0.1):
        p = np.array(P0)
        p[4] = beta
        if int(engine.step_batch(np.array([p]), 8)[1][0]) == 1:
            bad = p
            break
    assert bad is not None, "no beta of the ladder is rejected for its temperature"
    cfg = scfg(W.data * (1.0 + 0.01 * np.array([1, -1, 2, 0, -2, 1, -1, 0.5])))
    starts = np.array([np.array(P0), bad])
    res = run(W, cfg, starts)
    n = replay(cfg, res, starts)
    assert res["status"][1] == fr.NO_START and np.isinf(res["chisq"][1]) and res["status"][0] != fr.NO_START
    assert sum(n["nbad"]) >= 1
    # the box stops log CH4 above the data's value: the optimum lies on that bound
    pmin = PMIN.copy()
    pmin[6] = -0.4
    cfgb = scfg(W.data, pmin=pmin)
    startb = np.array(P0)
    startb[6] = -0.2
    resb = run(W, cfgb, [startb])
    replay(cfgb, resb, [startb])
    assert resb["best"][0][6] == -0.4 and resb["chisq"][0] > 0 and resb["status"][0] in (fr.CONVERGED, fr.STALLED)


def test_batching_and_repeat(W):
    cfg = scfg(W.data * (1.0 + 0.01 * np.array([1, -1, 2, 0, -2, 1, -1, 0.5])))
    starts = jittered(5, seed=8)
    together = run(W, cfg, starts)
    again = run(W, cfg, starts)
    for key in ("best", "chisq", "status", "niter", "trace"):
        assert together[key].tobytes() == again[key].tobytes(), key
    for s in (0, 3):
        alone = run(W, cfg, starts[s:s + 1])
        n = int(alone["niter"][0])
        assert alone["best"].tobytes() == together["best"][s:s + 1].tobytes()
        assert alone["chisq"][0] == together["chisq"][s] and alone["status"][0] == together["status"][s]
        assert np.array_equal(alone["trace"][0, :n + 1], together["trace"][s, :n + 1])
    other = run(W, cfg, starts, check=1)                        # the host's look changes nothing
    assert other["trace"].tobytes() == together["trace"].tobytes()


def test_refusals(W):
    from bart_amd import fit, transit_module as trm
    cfg = scfg(W.data)
    with pytest.raises(trm.TransitError, match="nrungs"):
        run(W, cfg, [P0], nrungs=9)
    with pytest.raises(trm.TransitError, match="no free parameter"):
        run(W, scfg(W.data, stepsize=np.zeros(7)), [P0])
    with pytest.raises(trm.TransitError, match="stepsize\\[6\\]"):
        run(W, scfg(W.data, stepsize=np.array([0.01, 0.0, 0.0, 0.0, 0.001, 0.05, -9.0])), [P0])
    with pytest.raises(TypeError, match="unknown option"):
        run(W, cfg, [P0], tolerance=1)
    cov = fit.covariance(W.worker, cfg, np.array(P0))
    assert cov.shape == (4, 4) and np.all(np.diag(cov) > 0) and np.allclose(cov, cov.T, rtol=1e-6)


CHILD_COMM = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
os.environ["BARTRT_KERNEL_BY"] = "whole"
import numpy as np
import torch
import torch.distributed as dist
import test_gpu_fit as T
from bart_amd import BARTfunc, engine, synthcfg
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%(port)d", rank=0, world_size=1, device_id=dev)
t = torch.ones(8, device=dev)
dist.all_reduce(t)
torch.cuda.synchronize()
case, cfg = synthcfg.make_worker_case(%(tmp)r, **T.CASE)
T.Shared.worker = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
data = T.Shared.worker.step(np.array(T.P0))[0].copy()
sc = T.scfg(data * (1.0 + 0.01 * np.array([1, -1, 2, 0, -2, 1, -1, 0.5])))
starts = T.jittered(3)
plain = T.run(T.Shared, sc, starts, check=1)
assert engine.comm_info()["ncollectives"] == 0
engine.comm_init()
k = engine.comm_info()["ncollectives"]
comm = T.run(T.Shared, sc, starts, check=1)
# model launches: the starts' own, then two per iteration made (check = 1: the loop stops at the first idle pick)
launches = 1 + 2 * int(plain["niter"].max())
assert engine.comm_info()["ncollectives"] - k == launches, (engine.comm_info(), k, launches)
for key in ("best", "chisq", "status", "niter", "trace"):
    assert plain[key].tobytes() == comm[key].tobytes(), key
assert plain["nbad"] == comm["nbad"]
engine.comm_free()
T.Shared.worker.close()
dist.destroy_process_group()
print("ok")
"""


def test_one_rank_communicator_same_bytes(tmp_path):
    """With a one-rank RCCL communicator the fit's bytes are the plain engine's, one collective per model launch.  (A
    fresh process with a time limit of its own, as every process that talks to RCCL in this suite.)"""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    code = CHILD_COMM % {"root": ROOT, "port": port, "tmp": str(tmp_path / "case")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout.splitlines(), "exit %d\n%s\n%s" % (r.returncode, r.stdout[-1500:],
                                                                                      r.stderr[-3000:])


def test_retrieve_reads_leastsq_and_chisqscale(W, tmp_path, monkeypatch):
    """retrieve.main on a synthetic cfg: with leastsq and chisqscale bestFit.txt holds the optimum and the sampler gets
    the scaled uncertainties; with both false output.npy is the bytes of a run that never enters the new code."""
    from bart_amd import BARTfunc, fit, retrieve, sampler, synthcfg
    W.worker.close()                       # retrieve.main makes its own worker (LAST test of this module)
    W.worker = None
    data = W.data * (1.0 + 0.01 * np.array([1, -1, 2, 0, -2, 1, -1, 0.5]))
    f = lambda v: " ".join(repr(float(x)) for x in v)

    def write(name, extra):
        case, cfg = synthcfg.make_worker_case(str(tmp_path / name), **CASE)
        txt = open(cfg).read()
        assert "[MCMC]" in txt
        head, tail = txt.split("[MCMC]", 1)
        keep = [l for l in tail.split("\n") if l.split("=")[0].strip() not in (
            "params", "pmin", "pmax", "stepsize", "data", "uncert", "nchains", "numit", "burnin", "walk", "grtest", "seed")]
        mc = ["params = " + f(P0), "pmin = " + f(PMIN), "pmax = " + f(PMAX), "stepsize = " + f(STEP), "data = " + f(data),
              "uncert = " + f(0.01 * np.abs(data)), "nchains = 4", "numit = 80", "burnin = 2", "walk = snooker",
              "grtest = False", "seed = 3"] + extra
        open(cfg, "w").write(head + "[MCMC]\n" + "\n".join(mc) + "\n" + "\n".join(keep))
        return cfg
    seen = {}
    real = sampler.run_native

    def spy(worker, cfg, log=None):
        seen["uncert"], seen["params"] = np.array(cfg.uncert, float), np.array(cfg.params, float)
        return real(worker, cfg, log=log)
    monkeypatch.setattr(sampler, "run_native", spy)
    cfg_on = write("on", ["leastsq = True", "chisqscale = True"])
    res = retrieve.main(["-c", cfg_on, "--out", str(tmp_path / "out_on"), "--fit-starts", "3"])
    best = res["fit"]
    assert (best["status"] != fit.RUNNING).all() and best["best_chisq"] < best["trace"][0, 0, 7]
    line = open(tmp_path / "out_on" / "bestFit.txt").read().split("\n")
    assert np.allclose([float(v) for v in line[1].split()], best["bestp"], rtol=1e-7, atol=0)
    assert "chisq = %.6f" % best["best_chisq"] in line[0]
    factor = np.sqrt(best["best_chisq"] / (8 - 4))
    assert np.array_equal(seen["uncert"], 0.01 * np.abs(data) * factor) and np.array_equal(seen["params"], best["bestp"])
    log = open(tmp_path / "out_on" / "MCMC.log").read()
    assert "fit start 2:" in log and "chisqscale" in log and "best-fit uncertainties" in log
    # both keys false: the fit is never called and the chain is the bytes of the run without the keys in the file
    monkeypatch.setattr(fit, "fit", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fit.fit was called")))
    retrieve.main(["-c", write("off", ["leastsq = False", "chisqscale = False"]), "--out", str(tmp_path / "out_off")])
    assert np.array_equal(seen["uncert"], 0.01 * np.abs(data))
    retrieve.main(["-c", write("none", []), "--out", str(tmp_path / "out_none")])
    a, b = (open(tmp_path / d / "output.npy", "rb").read() for d in ("out_off", "out_none"))
    assert a == b and len(a) > 128
    # chisqscale comes with leastsq, and needs a chi-square to scale by
    monkeypatch.undo()
    with pytest.raises(SystemExit):
        retrieve.main(["-c", write("alone", ["chisqscale = True"]), "--out", str(tmp_path / "out_alone")])
    zero = sampler.SamplerConfig.from_cfg(cfg_on)
    zero.data, zero.uncert = W.data, 0.01 * np.abs(W.data)
    w = BARTfunc.Worker(W.wcfg)
    try:
        with pytest.raises(ValueError, match="chi-square of zero"):
            retrieve.least_squares(w, zero, 1, lambda m: None)
    finally:
        w.close()
    # chisqscale without enough data
    with pytest.raises(ValueError, match="chisqscale"):
        few = sampler.SamplerConfig.from_cfg(cfg_on)
        few.stepsize = np.full(7, 0.01)
        few.data, few.uncert = few.data[:7], few.uncert[:7]
        retrieve.least_squares(None, few, 2, lambda m: None)
