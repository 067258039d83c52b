"""GPU: the resident sampler (bartrt_mcmc_run_resident, csrc/mcmc.hip: mcmc_advance).

The strong test is a SINGLE-STEP REPLAY: from the chain the device wrote, every iteration t is rebuilt on the host from
the device's own previous state chain[:, t - 1] -- draws from tests/mcmc_restate.py (its own Philox), the model
through engine.step_batch on all nchains rows, out-of-box rows replaced by the current point as the loop does -- and
the proposal, the stored chisq and the decision must be the replay's.  Rounding cannot accumulate; a wrong partner,
slot, guard or counter shows at the step where it happens.  A decision is left out only where |log u - log a| < 1e-9,
at most 0.5 % of a case's decisions (expected: none)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcmc_restate as mr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOLS = ("H2O", "CH4")
P0 = (-2.0, 0.0, 1.0, 0.0, 0.98, -0.5, -0.5)
NSTEPS = 41
CASE = dict(nwave=300, wnlow=1200.0, opmol=MOLS, molfit=MOLS, params=P0, nfilters=3)


class Shared:
    worker = None
    wcfg = None
    data = None


@pytest.fixture(scope="module")
def W(tmp_path_factory):
    from bart_amd import BARTfunc, synthcfg
    case, cfg = synthcfg.make_worker_case(str(tmp_path_factory.mktemp("resident")), **CASE)
    Shared.wcfg = BARTfunc.WorkerConfig.from_cfg(cfg)
    Shared.worker = BARTfunc.Worker(Shared.wcfg)
    Shared.data = Shared.worker.step(np.array(P0))[0].copy()
    yield Shared
    if Shared.worker is not None:
        Shared.worker.close()


def scfg(data, nch, walk, seed=9, **over):
    from bart_amd import sampler
    kw = dict(params=np.array(P0), pmin=np.array([-5.0, -2.0, -2.0, 0.0, 0.55, -9.0, -9.0]),
              pmax=np.array([-1.0, 1.0, 1.0, 1.0, 1.2, 1.5, 1.5]),
              stepsize=np.array([0.01, 0.0, 0.0, 0.0, 0.001, 0.05, 0.05]), data=data, uncert=0.01 * np.abs(data),
              nchains=nch, numit=NSTEPS * nch, burnin=2, walk=walk, seed=seed, grtest=False)
    kw.update(over)
    return sampler.SamplerConfig(**kw)


def run(W, cfg, **kw):
    from bart_amd import sampler
    before = dict(W.worker.nbad)
    res = sampler.run_resident(W.worker, cfg, **kw)
    res["nbad"] = [W.worker.nbad[k] - before[k] for k in (1, 2, 3)]
    return res


def problem(cfg):
    return mr.Problem(cfg.params, cfg.pmin, cfg.pmax, cfg.stepsize, cfg.data, cfg.uncert, cfg.nchains,
                      cfg.walk == "snooker", cfg.seed, cfg.prior, cfg.priorlow, cfg.priorup)


def replay(W, cfg, res):
    """Every iteration of an unthinned run rebuilt from the device's previous state.  Returns counts for the caller's
    own assertions: dict(outside, status1, accepted, skipped, decisions, nbad)."""
    from bart_amd import engine
    P, nch, nf = problem(cfg), cfg.nchains, len(cfg.data)
    chain, chisq = res["chain"], res["chisq"]
    assert chain.shape == (nch, NSTEPS, len(cfg.params)) and chisq.shape == (nch, NSTEPS)
    model = lambda rows: engine.step_batch(np.array(rows, float), nf)
    span = np.asarray(cfg.pmax, float) - np.asarray(cfg.pmin, float)
    x, cur, c, seen = P.start(model)
    nbad = [seen.count(k) for k in (1, 2, 3)]
    n = dict(outside=0, status1=0, accepted=0, skipped=0, decisions=0)
    for t in range(NSTEPS):
        if t > 0:
            x, c = chain[:, t - 1].tolist(), chisq[:, t - 1].tolist()
        props, inside, logjac = P.propose(t, x)
        band, status = model([props[i] if inside[i] else x[i] for i in range(nch)])
        for i in range(nch):
            cp = math.inf
            if inside[i]:
                if 1 <= status[i] <= 3:
                    nbad[status[i] - 1] += 1
                    n["status1"] += status[i] == 1
                    assert np.all(band[i] == -1.0)
                if status[i] == 0:
                    cp = P.chisq(band[i], props[i])
            else:
                n["outside"] += 1
            logu = P.log_u(t, i)
            loga = -0.5 * (cp - c[i]) + logjac[i] if math.isfinite(cp) else -math.inf
            want = math.isfinite(cp) and logu < loga
            # the device's decision: it either kept its state, bit for bit, or took the proposal
            # (at t = 0 the previous state is the restatement's own start: the device's agrees to rounding)
            near = lambda v: 1e-12 * np.abs(np.array(v)) + 1e-12 * span
            if t == 0:
                stayed = bool(np.all(np.abs(chain[i, 0] - np.array(x[i])) <= near(x[i])))
            else:
                stayed = np.array_equal(chain[i, t], np.array(x[i])) and chisq[i, t] == c[i]
            n["decisions"] += 1
            if stayed == want:
                if math.isfinite(loga) and abs(logu - loga) < 1e-9:
                    n["skipped"] += 1
                    continue
                raise AssertionError("iteration %d chain %d: the device %s, the replay %s (log u %r, log a %r)" % (
                    t, i, "stayed" if stayed else "moved", "accepts" if want else "refuses", logu, loga))
            if want:
                n["accepted"] += 1
                assert np.all(np.abs(chain[i, t] - np.array(props[i])) <= near(props[i])), (t, i, chain[i, t], props[i])
                assert abs(chisq[i, t] - cp) <= 1e-12 * abs(cp), (t, i, chisq[i, t], cp)
            elif t == 0:
                assert chisq[i, 0] == c[i] or abs(chisq[i, 0] - c[i]) <= 1e-12 * abs(c[i]), (i, chisq[i, 0], c[i])
    assert n["skipped"] <= 0.005 * n["decisions"], n
    assert n["accepted"] == round(res["accept_rate"] * NSTEPS * nch), (n, res["accept_rate"])
    n["nbad"] = nbad
    assert res["nbad"] == nbad, (res["nbad"], nbad)
    print("replay: %r" % n)
    return n


def models_of(W, chain):
    from bart_amd import engine
    return np.stack([engine.step_batch(np.ascontiguousarray(chain[:, k]), len(W.data))[0]
                     for k in range(chain.shape[1])], axis=1)


@pytest.mark.parametrize("walk", ["demc", "snooker"])
@pytest.mark.parametrize("nch", [1, 2, 3, 4, 5, 12, 64, 65, 130])
def test_replay_chain_counts(W, nch, walk):
    cfg = scfg(W.data, nch, walk)
    res = run(W, cfg)
    n = replay(W, cfg, res)
    assert n["accepted"] > 0
    assert np.all(res["chain"][:, :, [1, 2, 3]] == np.array(P0)[[1, 2, 3]])
    # models: the band fluxes of every chain's current state, bit for bit
    assert np.array_equal(res["models"], models_of(W, res["chain"]))


@pytest.mark.parametrize("walk", ["demc", "snooker"])
def test_replay_one_free_parameter(W, walk):
    cfg = scfg(W.data, 6, walk, stepsize=np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.05, 0.0]))
    assert replay(W, cfg, run(W, cfg))["accepted"] > 0


@pytest.mark.parametrize("walk", ["demc", "snooker"])
def test_replay_fixed_parameter_outside_its_box(W, walk):
    cfg = scfg(W.data, 6, walk, pmin=np.array([-5.0, 0.5, -2.0, 0.0, 0.55, -9.0, -9.0]))
    res = run(W, cfg)
    n = replay(W, cfg, res)
    assert n["accepted"] > 0 and np.all(res["chain"][:, :, 1] == 0.0)


@pytest.mark.parametrize("walk", ["demc", "snooker"])
def test_replay_shared_parameter(W, walk):
    cfg = scfg(W.data, 6, walk, stepsize=np.array([0.01, 0.0, 0.0, 0.0, 0.001, 0.05, -6.0]))
    res = run(W, cfg)
    n = replay(W, cfg, res)
    assert n["accepted"] > 0 and np.array_equal(res["chain"][:, :, 6], res["chain"][:, :, 5])
    assert np.ptp(res["chain"][:, :, 6]) > 0


@pytest.mark.parametrize("walk", ["demc", "snooker"])
def test_replay_two_sided_prior(W, walk):
    z = np.zeros(7)
    prior, lo, up = z.copy(), z.copy(), z.copy()
    prior[5], lo[5], up[5] = -0.48, 0.03, 0.06
    cfg = scfg(W.data, 6, walk, prior=prior, priorlow=lo, priorup=up)
    res = run(W, cfg)
    assert replay(W, cfg, res)["accepted"] > 0
    # the stored chisq is the data term plus the prior term: both sides of the prior value occur
    d = res["chain"][:, :, 5] - prior[5]
    assert (d < 0).any() and (d > 0).any()
    plain = run(W, scfg(W.data, 6, walk))
    assert not np.array_equal(plain["chisq"], res["chisq"])


@pytest.mark.parametrize("walk", ["demc", "snooker"])
def test_replay_tight_box(W, walk):
    pmin, pmax = np.array([-5.0, -2.0, -2.0, 0.0, 0.55, -0.52, -0.52]), np.array([-1.0, 1.0, 1.0, 1.0, 1.2, -0.48, -0.48])
    cfg = scfg(W.data, 12, walk, pmin=pmin, pmax=pmax)
    res = run(W, cfg)
    n = replay(W, cfg, res)            # (nbad equal to the replay's count: asserted there)
    assert n["outside"] > NSTEPS * 12 / 3, n
    assert np.all(res["chain"][:, :, 5:] >= -0.52) and np.all(res["chain"][:, :, 5:] <= -0.48)


def test_thinning_models_and_block_handover(W):
    cfg = scfg(W.data, 5, "snooker")
    full = run(W, cfg)
    cfg3 = scfg(W.data, 5, "snooker", thinning=3)
    thin = run(W, cfg3)
    rows = list(range(2, NSTEPS, 3)) + [NSTEPS - 1]
    assert rows[-2:] == [38, 40] and thin["chain"].shape == (5, 14, 7)
    for key in ("chain", "chisq", "models"):
        assert np.array_equal(thin[key], full[key][:, rows]), key
    assert thin["accept_rate"] == full["accept_rate"]
    assert np.array_equal(thin["models"], models_of(W, thin["chain"]))
    # blocks of 7 iterations, two in flight, against one block: the same bits; the progress reports arrive in order
    lines = []
    small = run(W, cfg, block=7, log=lines.append)
    for key in ("chain", "chisq", "models"):
        assert np.array_equal(small[key], full[key]), key
    steps = [int(l.split()[1].split("/")[0]) for l in lines if l.startswith("step ")]
    assert steps == [7, 14, 21, 28, 35, 41], lines
    one = run(W, cfg, block=1)
    assert np.array_equal(one["chain"], full["chain"]) and np.array_equal(one["chisq"], full["chisq"])


def test_same_seed_same_bytes_other_seed_other_chain(W):
    a, b = run(W, scfg(W.data, 5, "demc", seed=21)), run(W, scfg(W.data, 5, "demc", seed=21))
    c = run(W, scfg(W.data, 5, "demc", seed=22))
    for key in ("chain", "chisq", "models"):
        assert a[key].tobytes() == b[key].tobytes()
    assert not np.array_equal(a["chain"], c["chain"])


def test_device_draws_against_the_restatement(W):
    """bartrt_mcmc_draws: uniforms and partner indices exact; normals and log u within 4 ulp (the margin the device
    math library documents for double-precision log and sincos)."""
    from bart_amd import sampler
    worst = 0.0
    for seed, t, nch, npars in ((0, 0, 1, 1), (9, 7, 3, 7), (2 ** 64 - 1, 10, 130, 6), (12345, mr.START_T + 3, 65, 64)):
        got = sampler.draws(seed, t, nch, npars)
        want = np.array([mr.draws_row(seed, t, nch, i, npars) for i in range(nch)])
        exact = [0, 1, 2, 3, 4, 6, 7, 8]
        assert np.array_equal(got[:, exact], want[:, exact])
        rest = [5] + list(range(9, 9 + npars))
        ulp = np.abs(got[:, rest] - want[:, rest]) / np.spacing(np.abs(want[:, rest]))
        worst = max(worst, float(ulp.max()))
    print("device draws: worst difference of a normal or log u against the host restatement: %.2f ulp" % worst)
    assert worst <= 4.0


def test_refusals(W):
    from bart_amd import sampler, transit_module as trm
    with pytest.raises(trm.TransitError, match="1024 chains"):
        run(W, scfg(W.data, 1025, "demc"))
    big = np.zeros(65)
    with pytest.raises(trm.TransitError, match="too many parameters"):
        run(W, scfg(W.data, 4, "demc", params=big, pmin=big - 1, pmax=big + 1, stepsize=big + 0.1))
    for bad in (-9.0, -7.0, -0.5):       # out of range; itself; not a parameter's number
        with pytest.raises(trm.TransitError, match="stepsize\\[6\\]"):
            run(W, scfg(W.data, 4, "demc", stepsize=np.array([0.01, 0.0, 0.0, 0.0, 0.001, 0.05, bad])))
    with pytest.raises(trm.TransitError, match="shared"):     # shared with a shared one
        run(W, scfg(W.data, 4, "demc", stepsize=np.array([0.01, 0.0, 0.0, 0.0, 0.001, -7.0, -6.0])))
    lib = trm.lib()
    cfg = scfg(W.data, 4, "demc")
    args = [np.ascontiguousarray(v, float) for v in (cfg.params, cfg.pmin, cfg.pmax, cfg.stepsize, cfg.data, cfg.uncert)]
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    chain, chis = np.zeros((4, 3, 7)), np.zeros((4, 3))
    call = lambda n, npars: lib.bartrt_mcmc_run_resident(n, npars, C.c_long(3), *[p(v) for v in args[:4]], 3, p(args[4]),
                                                        p(args[5]), None, p(chain), p(chis), None, None, None)
    assert call(4, 7) == 0                                    # (null options, no models, no counters)
    assert call(1025, 7) == -1 and b"1024" in lib.bartrt_last_error()          # BARTRT_EINVAL
    assert call(4, 65) == -1 and lib.bartrt_last_error()
    # the host loop is as it was: runs, and refuses a shared parameter
    res = sampler.run_native(W.worker, scfg(W.data, 4, "demc", numit=40))
    assert res["chain"].shape == (4, 10, 7) and res["accept_rate"] > 0
    args[3][6] = -6.0
    rc = lib.bartrt_mcmc_run(4, 7, C.c_long(3), *[p(v) for v in args[:4]], 3, p(args[4]), p(args[5]), 0,
                             C.c_ulonglong(1), p(chain), p(chis), None, None)
    assert rc < 0 and b"shared" in lib.bartrt_last_error()


CHILD_COMM = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
os.environ["BARTRT_KERNEL_BY"] = "whole"
import numpy as np
import torch
import torch.distributed as dist
import test_gpu_mcmc_resident as T
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
sc = T.scfg(data, 6, "snooker")
plain = T.run(T.Shared, sc)
start = T.problem(sc).start(lambda rows: engine.step_batch(np.array(rows, float), len(data)))
calls = len(start[3]) // 6 + T.NSTEPS            # model calls of a run: the start's rounds and the iterations
assert engine.comm_info()["ncollectives"] == 0
engine.comm_init()
k = engine.comm_info()["ncollectives"]
comm = T.run(T.Shared, sc)
assert engine.comm_info()["ncollectives"] - k == calls, (engine.comm_info(), k, calls)    # one per model call
for key in ("chain", "chisq", "models"):
    assert plain[key].tobytes() == comm[key].tobytes(), key
assert plain["accept_rate"] == comm["accept_rate"] and plain["nbad"] == comm["nbad"]
engine.comm_free()
T.Shared.worker.close()
dist.destroy_process_group()
print("ok")
"""


def test_one_rank_communicator_same_bytes(tmp_path):
    """Under kernel_by whole with a one-rank RCCL communicator: chain, chisq and models are the bytes of the run
    without one, and ncollectives rose by one per model call.  (A fresh process with a time limit of its own, as every
    process that talks to RCCL in this suite.)"""
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


def test_replay_model_rejections_with_tmax_just_above_the_start_profile(W):
    """LAST in this module: it replaces the module's worker by one whose Tmax lies just above the hottest layer of the
    start profile, so the T(p) model rejects some in-box proposals (status 1, -1 rows): they are counted in nbad[1]
    and the chain does not move on them."""
    import torch
    from bart_amd import BARTfunc, engine
    prof, st = engine.step_profiles_dev(torch.tensor([P0], dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    hottest = float(prof[0, :engine.nlayers()].max().cpu())
    assert int(st[0]) == 0 and 400.0 < hottest < 3000.0
    W.worker.close()
    W.worker = None
    W.wcfg.Tmax = hottest + 1.0
    W.worker = BARTfunc.Worker(W.wcfg)
    for walk in ("demc", "snooker"):
        cfg = scfg(W.data, 12, walk, stepsize=np.array([0.01, 0.0, 0.0, 0.0, 0.002, 0.05, 0.05]))
        res = run(W, cfg)
        n = replay(W, cfg, res)
        assert n["status1"] > 0 and res["nbad"][0] > 0 and res["nbad"][1:] == [0, 0], (n, res["nbad"])
        assert n["accepted"] > 0
