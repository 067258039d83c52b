"""GPU + RCCL: the library's own communicator (include/bartrt.h, bartrt_comm_*) and the per-step path it opens.

One child under a torch `nccl` group of world 1 -- the torch group's RCCL and the library's communicator live in the
same process -- checks that attaching a communicator of one rank changes no bit (host and device step, spectra,
bartrt_mcmc_run), issues exactly one collective per step, detaches cleanly, and that bad use is refused.  With two or
more GPUs visible, N children (one per GPU, `--shard r N` on device r, the id handed over through a file) check the
sharded ranks against an unsharded run, and torch.distributed.run drives bart_amd.retrieve --native-sharded.  Every
process that talks to RCCL is a fresh child of pytest with a time limit of its own; a failing child ends the test."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOLS = ("H2O", "CO", "CO2", "CH4")
P0 = (-2.0, 0.0, 1.0, 0.0, 0.98, -0.5, -0.5, -0.5, -0.5)


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _env(**extra):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    e.setdefault("OMP_NUM_THREADS", "1")
    e.update(extra)
    return e


def _run(args, timeout, **env):
    r = subprocess.run(args, env=_env(**env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


# the inputs every process of a test rebuilds the same way (a seeded case and parameter sets)
COMMON = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from bart_amd import BARTfunc, engine, sampler, synthcfg, transit_module as trm
MOLS, P0 = %(mols)r, %(p0)r
cfg = os.path.join(%(tmp)r, "BART.cfg")
if not os.path.exists(cfg):    # (the ranks of a multi-GPU test read what the unsharded run before them wrote)
    case, cfg = synthcfg.make_worker_case(%(tmp)r, nwave=%(nwave)d, wnlow=1200.0, opmol=MOLS, molfit=MOLS, params=P0,
                                          nfilters=5, ebalance=True)
rng = np.random.default_rng(3)
pars = np.array(P0) + rng.normal(0, [0.3, 0.2, 0.2, 0.05, 0.02, 0.5, 0.5, 0.5, 0.5], (3, 7, 9))
pars[..., 3] = np.clip(pars[..., 3], 0, 1)
pars[1, 2, 4] = 5.0        # T(p) above Tmax: status 1
pars[2, 4, 8] = 4.5        # CH4 above 1: status 2

def scfg(data):
    return sampler.SamplerConfig(params=np.array(P0), pmin=np.array([-5.0, -2.0, -2.0, 0.0, 0.55, -9, -9, -9, -9]),
                                 pmax=np.array([-1.0, 1.0, 1.0, 1.0, 1.2, 1.5, 1.5, 1.5, 1.5]),
                                 stepsize=np.array([0.01, 0.0, 0.0, 0.0, 0.001, 0.05, 0.05, 0.0, 0.05]),
                                 data=data, uncert=0.01 * np.abs(data), nchains=6, numit=60, burnin=2, seed=9,
                                 grtest=False)

def mcmc(w, data):
    nb = dict(w.nbad)
    res = sampler.run_native(w, scfg(data))
    return res, [w.nbad[k] - nb[k] for k in (1, 2, 3)]
"""

CHILD_WORLD1 = COMMON + r"""
import ctypes as C
import torch
import torch.distributed as dist
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%(port)d", rank=0, world_size=1, device_id=dev)
t = torch.ones(8, device=dev)
dist.all_reduce(t)                                 # the torch group's RCCL is up and mapped
torch.cuda.synchronize()
lib = trm.lib()
EINVAL, EIO, ENOTSUP = -1, -2, -4

w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
nf = w.nfilters
d_par = torch.from_numpy(pars).to(dev)
data = engine.step_batch(np.array([P0]), nf)[0][0]

def host(s):
    return engine.step_batch(pars[s], nf)

def bits(x):
    # (bit-identical, NaN included: the spectrum of a walker whose profile the RT cannot evaluate may hold NaN)
    return x.view(torch.int64) if x.dtype == torch.float64 else x

def same(a, b):
    return torch.equal(bits(a), bits(b))

def device(s):
    band, st, spec = engine.step_batch_dev(d_par[s], nf, want_spec=True)
    torch.cuda.synchronize()
    return band.cpu(), st.cpu(), spec.cpu()

plain_h = [host(s) for s in range(3)]
plain_d = [device(s) for s in range(3)]
assert {0, 1, 2} <= set(np.concatenate([h[1] for h in plain_h]).tolist()), [h[1] for h in plain_h]
plain_mc = mcmc(w, data)
assert engine.comm_info() == {"rank": -1, "nranks": 0, "ncollectives": 0}

engine.comm_init()                                 # id over the torch nccl group, then attach
info = engine.comm_info()
assert info["rank"] == 0 and info["nranks"] == 1 and info["ncollectives"] == 0, info
maps = open("/proc/self/maps").read().split("\n")
rccl = {l.split()[-1] for l in maps if "librccl" in l}
assert len(rccl) == 1, rccl                        # the library took the copy torch had mapped
uid = engine.comm_unique_id()
assert lib.bartrt_comm_init(uid, 0, 1) == EINVAL   # a second init
k = engine.comm_info()["ncollectives"]
for s in range(3):
    b, st = host(s)
    assert engine.comm_info()["ncollectives"] == k + 1
    k += 1
    assert np.array_equal(b, plain_h[s][0]) and np.array_equal(st, plain_h[s][1]), s
    bd, sd, spd = device(s)
    assert engine.comm_info()["ncollectives"] == k + 1
    k += 1
    assert same(bd, plain_d[s][0]) and same(sd, plain_d[s][1]) and same(spd, plain_d[s][2]), (
        s, same(bd, plain_d[s][0]), same(sd, plain_d[s][1]), same(spd, plain_d[s][2]), sd.tolist())
    # the torch group keeps working beside the library's communicator
    dist.all_reduce(t)
comm_mc = mcmc(w, data)
assert engine.comm_info()["ncollectives"] > k
for a, b in ((plain_mc[0]["chain"], comm_mc[0]["chain"]), (plain_mc[0]["chisq"], comm_mc[0]["chisq"])):
    assert np.array_equal(a, b)
assert plain_mc[0]["accept_rate"] == comm_mc[0]["accept_rate"] and plain_mc[1] == comm_mc[1], (plain_mc[1], comm_mc[1])

engine.comm_free()
k = engine.comm_info()["ncollectives"]
assert engine.comm_info()["nranks"] == 0
for s in range(3):
    b, st = host(s)
    bd, sd, spd = device(s)
    assert np.array_equal(b, plain_h[s][0]) and same(bd, plain_d[s][0]) and same(spd, plain_d[s][2])
assert engine.comm_info()["ncollectives"] == k
# bad use: ranks that are not the engine's block
assert lib.bartrt_comm_init(uid, 0, 2) == EINVAL and lib.bartrt_comm_init(uid, 1, 1) == EINVAL
assert lib.bartrt_comm_init(uid, 1, 2) == EINVAL
w.close()

# a sharded engine without a communicator: the step fails as before, contribution functions stay unsupported
ws = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg), shard=(0, 2))
band = np.zeros((7, nf)); st = np.zeros(7, np.int32)
p = np.ascontiguousarray(pars[0])
assert lib.bartrt_step_batch(p.ctypes.data, 7, 9, band.ctypes.data, st.ctypes.data) == EIO
prof = np.zeros((1, engine.nprof())); out = np.zeros((1, 5, engine.nlayers()))
assert lib.bartrt_cf_batch(prof.ctypes.data, 1, prof.shape[1], 1, out.ctypes.data, None, None) == ENOTSUP
assert lib.bartrt_comm_init(uid, 0, 1) == EINVAL and lib.bartrt_comm_init(uid, 1, 2) == EINVAL
ws.close()
assert lib.bartrt_comm_init(uid, 0, 1) == EINVAL   # no engine
dist.all_reduce(t)
dist.destroy_process_group()
print("ok")
"""


def test_comm_world1_under_torch_nccl_group(tmp_path):
    code = CHILD_WORLD1 % {"root": ROOT, "port": _free_port(), "tmp": str(tmp_path / "case"), "nwave": 1777,
                           "mols": MOLS, "p0": P0}
    r = _run([sys.executable, "-c", code], 900)
    assert "ok" in r.stdout.splitlines(), r.stdout[-1500:] + r.stderr[-3000:]


# ---- two or more GPUs ---------------------------------------------------------
def _visible_gpus():
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], env=_env(),
                       capture_output=True, text=True, timeout=120)
    return int(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else 0


# one rank of N (or, with N == 0, the unsharded run): band fluxes, statuses and mcmc_run chains to out.npz
CHILD_RANK = COMMON + r"""
import time
rank, N, kernel_by, out, idfile = %(rank)d, %(n)d, %(kernel_by)r, %(out)r, %(idfile)r
os.environ["BARTRT_KERNEL_BY"] = kernel_by
w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg), shard=(rank, N) if N else None, device=rank)
if N:
    if rank == 0:
        uid = engine.comm_unique_id()
        open(idfile + ".tmp", "wb").write(uid)
        os.rename(idfile + ".tmp", idfile)
    else:
        t0 = time.time()
        while not os.path.exists(idfile):
            assert time.time() - t0 < 120, "no id from rank 0"
            time.sleep(0.05)
        uid = open(idfile, "rb").read()
    engine.comm_attach(uid, rank, N)
data = np.load(%(data)r) if os.path.exists(%(data)r) else engine.step_batch(np.array([P0]), w.nfilters)[0][0]
bands = [engine.step_batch(pars[s], w.nfilters) for s in range(3)]
res, nbad = mcmc(w, data)
np.savez(out, band=np.array([b[0] for b in bands]), status=np.array([b[1] for b in bands]), chain=res["chain"],
         chisq=res["chisq"], nbad=np.array(nbad), data=data)
w.close()
print("ok")
"""


def _ranks(tmp_path, n, kernel_by):
    fmt = {"root": ROOT, "tmp": str(tmp_path / "case"), "nwave": 2424, "mols": MOLS, "p0": P0, "n": n,
           "kernel_by": kernel_by, "idfile": str(tmp_path / ("id_%s_%d" % (kernel_by, n))),
           "data": str(tmp_path / "data.npy")}
    outs = [str(tmp_path / ("%s_%d_%d.npz" % (kernel_by, n, r))) for r in range(max(n, 1))]
    procs = [subprocess.Popen([sys.executable, "-c", CHILD_RANK % dict(fmt, rank=r, out=outs[r])], env=_env(),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(max(n, 1))]
    fails = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        if p.returncode != 0:
            fails.append("exit %d\n%s\n%s" % (p.returncode, o[-1000:], e[-3000:]))
    assert not fails, fails
    return [dict(np.load(o)) for o in outs]


def test_sharded_ranks_against_unsharded(tmp_path):
    ngpu = _visible_gpus()
    if ngpu < 2:
        pytest.skip("needs two or more GPUs (%d visible)" % ngpu)
    ref = _ranks(tmp_path, 0, "whole")[0]
    np.save(tmp_path / "data.npy", ref["data"])
    for n in sorted({2, min(ngpu, 8)}):
        for r in _ranks(tmp_path, n, "whole"):                       # the unsharded bits on every rank
            for key in ("band", "status", "chain", "chisq", "nbad"):
                assert np.array_equal(r[key], ref[key]), (n, key)
        loc = _ranks(tmp_path, n, "local")
        for r in loc[1:]:                                             # the ranks agree with each other bit for bit
            for key in ("band", "status", "chain", "chisq", "nbad"):
                assert np.array_equal(r[key], loc[0][key]), (n, key)
        ok = loc[0]["status"] == 0
        assert np.array_equal(loc[0]["status"], ref["status"])
        np.testing.assert_allclose(loc[0]["band"][ok], ref["band"][ok], rtol=1e-10, atol=0)


def test_retrieve_native_sharded_under_torchrun(tmp_path):
    ngpu = _visible_gpus()
    if ngpu < 2:
        pytest.skip("needs two or more GPUs (%d visible)" % ngpu)
    n = min(ngpu, 8)
    sys.path.insert(0, ROOT)
    from bart_amd import synthcfg
    case, cfg = synthcfg.make_worker_case(str(tmp_path / "case"), nwave=2424, wnlow=1200.0, params=(-2.0, 0.0, 1.0,
                                                                                                      0.0, 0.98, -0.5))
    data = json.loads(_run([sys.executable, "-c",
                            "import sys; sys.path.insert(0, %r)\nimport json\nfrom bart_amd import BARTfunc\n"
                            "w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(%r))\n"
                            "print(json.dumps(w.step([-2.0, 0.0, 1.0, 0.0, 0.98, -0.5])[0].tolist()))" % (ROOT, cfg)],
                           300).stdout.strip().splitlines()[-1])
    with open(cfg, "a") as f:
        f.write("pmin = -5.0 -2.0 -2.0 0.0 0.55 -9.0\npmax = -1.0 1.0 1.0 1.0 1.2 1.5\n")
        f.write("stepsize = 0.01 0.0 0.0 0.0 0.001 0.05\n")
        f.write("data = " + " ".join("%.10e" % d for d in data) + "\n")
        f.write("uncert = " + " ".join("%.10e" % (0.01 * d) for d in data) + "\n")
        f.write("nchains = 8\nburnin = 2\nwalk = demc\nseed = 5\n")
    _run([sys.executable, "-m", "bart_amd.retrieve", "-c", cfg, "--numit", "160", "--out", str(tmp_path / "one")], 600,
         BARTRT_KERNEL_BY="whole", PYTHONPATH=ROOT)
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
          "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "-m", "bart_amd.retrieve", "--native-sharded",
          "-c", cfg, "--numit", "160", "--out", str(tmp_path / "many")], 900, BARTRT_KERNEL_BY="whole", PYTHONPATH=ROOT)
    a, b = np.load(tmp_path / "one" / "output.npy"), np.load(tmp_path / "many" / "output.npy")
    assert a.shape == b.shape and np.array_equal(a, b)
