"""GPU: convergence tests, exit and resume of the resident sampler (bartrt_mcmc_run_resident with burnin / grcheck /
grexit / first / start; csrc/mcmc.hip: mcmc_gr_leaf, mcmc_gr_merge, mcmc_gr_finish; bartrt_mcmc_gr).

The statistic is held to the host build of csrc/gr_core.hpp bit for bit (tests/gr_core_host.cpp) and to exact
rationals within the bound tests/gr_restate.py measures (8 x the larger deviation of the host build and of numpy:
8.55e-08 as measured, see tests/test_gr_core_cpu.py).  The loop is held to itself: a run cut in two, or stopped on
convergence and resumed, writes the bytes of the uninterrupted run.  The case and the configuration helper are those
of tests/test_gpu_mcmc_resident.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gr_restate as gr  # noqa: E402
import test_gpu_mcmc_resident as T  # noqa: E402

pytestmark = pytest.mark.gpu

N = 48            # iterations of every full run here
SENTINEL = -777.0
EXIT_SEED = 9     # test_exit: the seed whose first converged test is not the last one (T.scfg's own default)


@pytest.fixture(scope="module")
def W(tmp_path_factory):
    from bart_amd import BARTfunc, synthcfg
    case, cfg = synthcfg.make_worker_case(str(tmp_path_factory.mktemp("converge")), **T.CASE)
    T.Shared.wcfg = BARTfunc.WorkerConfig.from_cfg(cfg)
    T.Shared.worker = BARTfunc.Worker(T.Shared.wcfg)
    T.Shared.data = T.Shared.worker.step(np.array(T.P0))[0].copy()
    yield T.Shared
    if T.Shared.worker is not None:
        T.Shared.worker.close()
    T.Shared.worker = None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return gr.build_host(tmp_path_factory.mktemp("gr_core"))


def call(data, nsteps, walk="snooker", seed=9, thin=1, block=8, nch=5, **o):
    """bartrt_mcmc_run_resident itself, on arrays filled with SENTINEL.  Returns the full arrays and every output;
    rc < 0: the call's refusal, with its message."""
    from bart_amd import sampler, transit_module as trm
    cfg = T.scfg(data, nch, walk, seed=seed)
    par, pmin, pmax, step, dat, unc, _ = sampler.problem_arrays(cfg, "test")
    nk, ngr = -(-nsteps // thin), 16
    out = dict(chain=np.full((nch, nk, 7), SENTINEL), chisq=np.full((nch, nk), SENTINEL),
               models=np.full((nch, nk, 3), SENTINEL), grstat=np.zeros((ngr, 7)), grwhen=np.zeros(ngr, np.int64))
    made, done, nacc, nbad = C.c_int(-1), C.c_long(-1), C.c_long(-1), (C.c_long * 4)()
    opts = sampler.McmcOpts(size=C.sizeof(sampler.McmcOpts), snooker=int(walk == "snooker"), seed=seed, thin=thin,
                            block=block, ngr=ngr, grstat=out["grstat"].ctypes.data, grwhen=out["grwhen"].ctypes.data,
                            ngr_out=C.addressof(made), done=C.addressof(done))
    start = o.pop("start", None)
    if start is not None:
        start = np.ascontiguousarray(start, float)
        opts.start = start.ctypes.data
    for k, v in o.items():
        setattr(opts, k, v)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    lib = trm.lib()
    rc = lib.bartrt_mcmc_run_resident(nch, 7, C.c_long(nsteps), p(par), p(pmin), p(pmax), p(step), 3, p(dat), p(unc),
                                      C.cast(C.byref(opts), C.c_void_p), p(out["chain"]), p(out["chisq"]),
                                      p(out["models"]), C.cast(C.byref(nacc), C.c_void_p), C.cast(nbad, C.c_void_p))
    out.update(rc=rc, err=lib.bartrt_last_error().decode() if rc < 0 else "", done=done.value, ngr=made.value,
               naccept=nacc.value, nbad=list(nbad)[1:], stepsize=step)
    return out


KEYS = ("chain", "chisq", "models")


@pytest.mark.parametrize("shape", gr.SHAPES, ids=lambda s: "rows%d-ch%d-p%d-r%d" % s)
def test_probe_is_the_host_build(host, shape):
    """bartrt_mcmc_gr on random chains (no engine): triples and R the host program's bits, converged the same."""
    from bart_amd import sampler
    chain, step, r0, r1 = gr.case(shape)
    psrf, triples, conv = sampler.gelman_rubin_dev(chain, step, r0, r1)
    hp, ht, hc = host("stat", chain, step, r0, r1)
    assert triples.tobytes() == ht.tobytes()
    assert np.all(psrf[step <= 0] == 0.0)
    ulp = np.abs(psrf - hp)[step > 0] / np.spacing(hp[step > 0])
    print("probe: R against the host build: %.1f ulp at most" % ulp.max())
    assert ulp.max() <= 1.0 and conv == bool(hc)


def test_probe_accuracy_and_edges(host):
    from bart_amd import sampler, transit_module as trm
    m = gr.measure(host)
    for shape in gr.EXACT_SHAPES:
        chain, step, r0, r1 = gr.case(shape)
        dev = gr.deviation(sampler.gelman_rubin_dev(chain, step, r0, r1)[0], gr.exact(chain, step, r0, r1))
        print("probe %r: deviation from the exact value %.3g (bound %.3g)" % (shape, dev, m["bound"]))
        assert dev <= m["bound"]
    chain, step, r0, r1 = gr.case((gr.TILE + 1, 3, 7, 3))
    flat = chain.copy()
    flat[:, :, 4] = 97000.0                              # a free parameter that never moved
    psrf, _, conv = sampler.gelman_rubin_dev(flat, step, r0, r1, 1e9)
    assert np.isnan(psrf[4]) and not conv
    assert sampler.gelman_rubin_dev(chain, step, r0, r1, 1e9)[2]
    for ch, a, b in ((chain, 3, 6), (chain[:1], 3, 200)):          # fewer than four rows; one chain
        psrf, triples, conv = sampler.gelman_rubin_dev(ch, step, a, b, 1e9)
        assert not psrf.any() and not triples.any() and not conv
    with pytest.raises(trm.TransitError, match="bartrt_mcmc_gr"):
        sampler.gelman_rubin_dev(chain, step, 0, chain.shape[1] + 1)


@pytest.mark.parametrize("walk", ["demc", "snooker"])
def test_split_and_resume(W, walk):
    """48 iterations against 16 + 32 resumed (16 is no multiple of ten: a resumed call that counted from zero would
    take its gamma = 1 moves at the wrong iterations), and at thin 4 against 20 + 28."""
    for thin, cut in ((1, 16), (4, 20)):
        full = call(W.data, N, walk, thin=thin)
        a = call(W.data, cut, walk, thin=thin)
        b = call(W.data, N - cut, walk, thin=thin, first=cut, start=a["chain"][:, -1])
        assert full["rc"] == a["rc"] == b["rc"] == 0 and (full["done"], a["done"], b["done"]) == (N, cut, N - cut)
        for k in KEYS:
            assert np.concatenate([a[k], b[k]], axis=1).tobytes() == full[k].tobytes(), (thin, k)
        assert not (full["chain"] == SENTINEL).any() and full["naccept"] > 0
        assert a["naccept"] + b["naccept"] == full["naccept"]
        assert [x + y for x, y in zip(a["nbad"], b["nbad"])] == full["nbad"]


def test_resume_refusals(W):
    good = call(W.data, 16)
    start = good["chain"][:, -1]
    for kw, word in ((dict(thin=4, first=18, start=start), "first"), (dict(start=start), "start"),
                     (dict(first=16), "start"), (dict(grcheck=12), "grcheck")):
        r = call(W.data, 16, **kw)
        assert r["rc"] == -1 and "mcmc_run_resident" in r["err"] and word in r["err"], r["err"]      # BARTRT_EINVAL
        assert (r["chain"] == SENTINEL).all()
    again = call(W.data, 16)
    assert again["rc"] == 0 and again["chain"].tobytes() == good["chain"].tobytes()


@pytest.fixture(scope="module")
def history(W):
    """The run of test 6: grcheck 8, burnin 8, no exit."""
    return call(W.data, N, seed=EXIT_SEED, burnin=8, grcheck=8)


def test_records(W, host, history):
    from bart_amd import sampler
    h = history
    # after 8 iterations no row lies past the burn-in; after 16 there are eight
    assert h["rc"] == 0 and h["done"] == N and h["ngr"] == 5
    assert h["grwhen"][:5].tolist() == [16, 24, 32, 40, 48] and not h["grwhen"][5:].any()
    plain = call(W.data, N, seed=EXIT_SEED)
    assert plain["ngr"] == 0 and all(plain[k].tobytes() == h[k].tobytes() for k in KEYS)
    bound, step, free = gr.measure(host)["bound"], h["stepsize"], h["stepsize"] > 0
    for k in range(5):
        T_k = int(h["grwhen"][k])
        probe = sampler.gelman_rubin_dev(h["chain"], step, 8, T_k)[0]
        assert h["grstat"][k].tobytes() == probe.tobytes(), k
        want = sampler.gelman_rubin(h["chain"][:, 8:T_k][:, :, free])
        rel = np.abs(h["grstat"][k][free] - want) / want
        print("record %d (after %d): R %r, against numpy %.3g" % (k, T_k, h["grstat"][k][free].tolist(), rel.max()))
        assert np.all(np.isfinite(want)) and rel.max() <= bound
    # a resumed call tests its own rows alone: burnin 8 lies before first = 16, so its tests start 4 rows in
    b = call(W.data, 32, seed=EXIT_SEED, burnin=8, grcheck=8, first=16, start=h["chain"][:, 15])
    assert b["grwhen"][:b["ngr"]].tolist() == [24, 32, 40, 48]
    assert b["grstat"][0].tobytes() == sampler.gelman_rubin_dev(h["chain"], step, 16, 24)[0].tobytes()


def exit_point(h):
    """The threshold of test 7 from the history, and the record at which a run under it stops."""
    free = h["stepsize"] > 0
    tops = h["grstat"][:h["ngr"]][:, free].max(axis=1)
    tops = np.where(np.isfinite(tops), tops, np.inf)              # (a NaN or an inf never counts as converged)
    thr = (1 + 1e-6) * float(tops.min())
    kstar = int(np.argmax(tops < thr))
    assert kstar < h["ngr"] - 1, "seed %d: the first converged test is the last one; take another seed" % EXIT_SEED
    return thr, int(h["grwhen"][kstar])


def check_exit(data, h, thr, stop):
    for block in (8, 4):
        e = call(data, N, seed=EXIT_SEED, block=block, burnin=8, grcheck=8, grexit=1, grthreshold=thr)
        assert e["rc"] == 0 and e["done"] == stop, (block, e["done"], stop)
        plain = call(data, stop, seed=EXIT_SEED)
        for k in KEYS:
            assert e[k][:, :stop].tobytes() == h[k][:, :stop].tobytes(), (block, k)
            assert (e[k][:, stop:] == SENTINEL).all(), (block, k)
        assert (e["naccept"], e["nbad"]) == (plain["naccept"], plain["nbad"])
        assert e["grwhen"][:e["ngr"]].tolist() == list(range(16, stop + 1, 8))
    never = call(data, N, seed=EXIT_SEED, burnin=8, grcheck=8, grexit=1, grthreshold=1.0)
    assert never["done"] == N and never["chain"].tobytes() == h["chain"].tobytes()
    rest = call(data, N - stop, seed=EXIT_SEED, first=stop, start=e["chain"][:, stop - 1])
    for k in KEYS:
        assert rest[k].tobytes() == h[k][:, stop:].tobytes(), k
    return e


def test_exit(W, history):
    thr, stop = exit_point(history)
    print("exit: threshold %.9g stops the run after %d of %d iterations" % (thr, stop, N))
    check_exit(W.data, history, thr, stop)


CHILD_COMM = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
os.environ["BARTRT_KERNEL_BY"] = "whole"
import numpy as np
import torch
import torch.distributed as dist
import test_gpu_mcmc_converge as V
import test_gpu_mcmc_resident as T
from bart_amd import BARTfunc, engine, synthcfg
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%(port)d", rank=0, world_size=1, device_id=dev)
t = torch.ones(8, device=dev)
dist.all_reduce(t)
torch.cuda.synchronize()
case, cfg = synthcfg.make_worker_case(%(tmp)r, **T.CASE)
worker = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
data = worker.step(np.array(T.P0))[0].copy()
h = V.call(data, V.N, seed=V.EXIT_SEED, burnin=8, grcheck=8)
thr, stop = V.exit_point(h)
plain = V.check_exit(data, h, thr, stop)
engine.comm_init()
k = engine.comm_info()["ncollectives"]
hc = V.call(data, V.N, seed=V.EXIT_SEED, burnin=8, grcheck=8)
assert engine.comm_info()["ncollectives"] > k
for key in V.KEYS + ("grstat", "grwhen"):
    assert hc[key].tobytes() == h[key].tobytes(), key
comm = V.check_exit(data, hc, thr, stop)
for key in V.KEYS:
    assert comm[key].tobytes() == plain[key].tobytes(), key
assert (comm["done"], comm["naccept"], comm["nbad"]) == (plain["done"], plain["naccept"], plain["nbad"])
engine.comm_free()
worker.close()
dist.destroy_process_group()
print("ok")
"""


def test_one_rank_communicator_same_stop(tmp_path):
    """test_exit with a one-rank RCCL communicator on an unsharded engine (kernel_by whole): the same bytes and the
    same stop.  A fresh process with a time limit of its own, as every process that talks to RCCL in this suite."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    code = CHILD_COMM % {"root": T.ROOT, "port": port, "tmp": str(tmp_path / "case")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout.splitlines(), "exit %d\n%s\n%s" % (r.returncode, r.stdout[-1500:],
                                                                                      r.stderr[-3000:])


def test_retrieve_grexit_then_resume(W, history, tmp_path, capsys):
    """`retrieve --resident` under grexit, then `--resume` with grexit off: the output of the uninterrupted run.
    LAST in this module: retrieve.main makes workers of its own, after which the module's worker is rebuilt."""
    from bart_amd import BARTfunc, retrieve, synthcfg
    thr, stop = exit_point(history)
    sc = T.scfg(W.data, 5, "snooker", seed=EXIT_SEED)
    line = lambda v: " ".join(repr(float(x)) for x in v)

    def write(name, **over):
        case, cfg = synthcfg.make_worker_case(str(tmp_path / name), **T.CASE)
        head, tail = open(cfg).read().split("[MCMC]", 1)
        kw = dict(params=line(sc.params), pmin=line(sc.pmin), pmax=line(sc.pmax), stepsize=line(sc.stepsize),
                  data=line(sc.data), uncert=line(sc.uncert), nchains="5", numit=str(5 * N), burnin="8", walk="snooker",
                  grtest="True", grexit="False", grcheck="8", grthreshold=repr(thr), seed=str(EXIT_SEED),
                  savemodel="band.npy")
        kw.update(over)
        keep = [l for l in tail.split("\n") if l.split("=")[0].strip() not in kw]
        with open(cfg, "w") as f:
            f.write(head + "[MCMC]\n" + "\n".join("%s = %s" % kv for kv in kw.items()) + "\n" + "\n".join(keep))
        return cfg

    W.worker.close()
    W.worker = None
    try:
        whole = retrieve.main(["-c", write("whole"), "--resident", "--out", str(tmp_path / "o_whole")])
        assert whole["done"] == N and whole["chain"].shape == (5, N, 7)
        assert whole["chain"].tobytes() == history["chain"].tobytes()
        out = str(tmp_path / "o_cut")
        first = retrieve.main(["-c", write("exit", grexit="True"), "--resident", "--out", out])
        assert first["done"] == stop and np.load(os.path.join(out, "output.npy")).shape == (5, stop, 7)
        state = np.load(os.path.join(out, "state.npz"))
        assert (int(state["iterations"]), int(state["seed"]), int(state["nchains"])) == (stop, EXIT_SEED, 5)
        log = open(os.path.join(out, "MCMC.log")).read()
        assert "Gelman-Rubin after %d iterations" % stop in log and "All parameters have converged" in log
        with pytest.raises(SystemExit):
            retrieve.main(["-c", write("seed", seed="10"), "--resident", "--resume", "--out", out])
        assert "`seed`" in capsys.readouterr().err
        retrieve.main(["-c", write("rest"), "--resident", "--resume", "--out", out])
        for name in ("output.npy", "band.npy"):
            got, want = (np.load(os.path.join(d, name)) for d in (out, str(tmp_path / "o_whole")))
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
        after = np.load(os.path.join(out, "state.npz"))
        assert (int(after["iterations"]), int(after["naccept"])) == (N, whole["accepted"])
        assert open(os.path.join(out, "MCMC.log")).read().startswith(log)
    finally:
        W.worker = BARTfunc.Worker(W.wcfg)
