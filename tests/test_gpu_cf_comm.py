"""GPU, RCCL world of ONE rank (after tests/test_gpu_rccl.py): the contribution-function calls with the library's
communicator attached (include/bartrt.h, bartrt_comm_init + bartrt_cf_*).  An unsharded engine with a one-rank
communicator takes the sharded code -- its sums into slot 0 of the receive buffer, one in-place all-gather per chunk,
cf_combine over one slot -- and must return the bits it returns without a communicator, for each of the six call
shapes (bartrt_cf_batch, _dev, _over, _over_dev, _params, _params_dev), whatever the chunking, and again after
bartrt_comm_free; bartrt_get_comm's collective count rises by one per chunk.  A sharded engine without a communicator
still refuses bartrt_cf_setup and the calls that combine.  The process that talks to RCCL is a child of pytest."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _env():
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT",
                                                           "BARTRT_CF_WORKSPACE_BYTES")}
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    e.setdefault("OMP_NUM_THREADS", "1")
    return e


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
import torch.distributed as dist
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%(port)d", rank=0, world_size=1, device_id=dev)
from bart_amd import BARTfunc, cf, engine, synthcfg, transit_module as trm

ENOTSUP = -4
case, cfg = synthcfg.make_worker_case(%(tmp)r, nwave=1777, wnlow=1200.0, nfilters=5, nlayers=60)
wcfg = BARTfunc.WorkerConfig.from_cfg(cfg)
w = BARTfunc.Worker(wcfg, carry=False)
win = cf.filter_windows(w.specwn, wcfg.filters)
rng = np.random.default_rng(3)
pars = np.array(wcfg.params) + rng.normal(0, [0.3, 0.2, 0.2, 0.0, 0.02, 0.5], (6, 6))
pars[4, 5] = 4.1                      # CH4 > 1: the converter rejects the sample (status 2)
d_par = torch.from_numpy(pars).cuda()
d_prof, _ = engine.step_profiles_dev(d_par)
torch.cuda.synchronize()
prof = d_prof.cpu().numpy()
prof[2, 7] = np.nan                   # a non-finite temperature: ok = 0
d_prof = torch.from_numpy(prof).cuda()
over = np.full((6, 3), np.nan)
over[3, 1] = -1.5
d_over = torch.from_numpy(over).cuda()


def six(n):
    # the six call shapes on the first n walkers -> a flat list of numpy arrays
    out = []
    for kind in ("cf", "tr"):
        host = engine.contribution if kind == "cf" else engine.transmittance
        devf = engine.contribution_dev if kind == "cf" else engine.transmittance_dev
        parf = engine.contribution_from_params if kind == "cf" else engine.transmittance_from_params
        pard = engine.contribution_from_params_dev if kind == "cf" else engine.transmittance_from_params_dev
        kw = {"normalize": False} if kind == "cf" else {}
        out += list(host(prof[:n], win, full=True, want_ok=True, **kw))                     # bartrt_cf_batch
        out += list(host(prof[:n], win, full=True, want_ok=True, over=over[:n], **kw))      # _over
        out += list(parf(pars[:n], win, full=True, **kw))                                   # _params
        ok = torch.zeros(n, dtype=torch.uint8, device=dev)
        out += list(devf(d_prof[:n].contiguous(), full=True, d_ok=ok)) + [ok.clone()]       # _dev
        out += list(devf(d_prof[:n].contiguous(), full=True, d_ok=ok, over=d_over[:n].contiguous())) + [ok.clone()]
        out += list(pard(d_par[:n].contiguous(), full=True))                                # _params_dev
        torch.cuda.synchronize()
    return [o.cpu().numpy() if torch.is_tensor(o) else np.asarray(o) for o in out]


def same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape, (what, i)
        if x.ndim == 3 and x.shape[1] == 1777:      # per-wavenumber rows of a flagged / rejected sample: undefined
            keep = [k for k in range(len(x)) if k not in (2, 4)]
            x, y = x[keep], y[keep]
        assert np.array_equal(x, y, equal_nan=True), (what, i)


CALLS = 12                            # six shapes, two kinds
plain6, plain3 = six(6), six(3)
assert np.isnan(plain6[0][2]).all() and np.isfinite(plain6[0][[0, 1, 3, 4, 5]]).all()
assert engine.comm_info() == {"rank": -1, "nranks": 0, "ncollectives": 0}

engine.comm_init()
assert engine.comm_info()["nranks"] == 1
c0 = engine.comm_info()["ncollectives"]
same(six(6), plain6, "communicator, one chunk")
c1 = engine.comm_info()["ncollectives"]
assert c1 - c0 == CALLS, (c0, c1)     # one chunk a call: one collective a call

os.environ["BARTRT_CF_WORKSPACE_BYTES"] = "1"       # one walker per chunk: three walkers, three chunks
same(six(3), plain3, "communicator, three chunks")
c2 = engine.comm_info()["ncollectives"]
assert c2 - c1 == 3 * CALLS, (c1, c2)
del os.environ["BARTRT_CF_WORKSPACE_BYTES"]

# the step shares the receive buffer with these calls: it still gives its own bits afterwards
band0, st0 = engine.step_batch(pars, w.nfilters)
engine.comm_free()
assert engine.comm_info()["nranks"] == 0 and engine.comm_info()["ncollectives"] == c2 + 1
band1, st1 = engine.step_batch(pars, w.nfilters)
assert np.array_equal(band0, band1, equal_nan=True) and np.array_equal(st0, st1)
same(six(6), plain6, "after comm_free")
assert engine.comm_info()["ncollectives"] == c2 + 1
w.close()

# a sharded engine without a communicator: bartrt_cf_setup refuses, and so do the calls that combine
engine.init(case.tcfg, shard=(0, 2))
try:
    idx0, npts, resp, _ = win
    L = trm.lib()
    assert L.bartrt_cf_setup(len(idx0), trm._ptr(idx0), trm._ptr(npts), trm._ptr(resp)) == ENOTSUP
    assert b"sharded" in L.bartrt_last_error()
    engine.cf_setup_block(win)
    band = torch.empty((6, len(idx0), 60), dtype=torch.float64, device=dev)
    import ctypes as C
    assert L.bartrt_cf_batch_dev(C.c_void_p(d_prof.data_ptr()), 6, 1, C.c_void_p(band.data_ptr()), None, None, None) == ENOTSUP
    assert b"sharded" in L.bartrt_last_error()
finally:
    trm.free_memory()
dist.barrier()
dist.destroy_process_group()
print("ok")
"""


def test_a_one_rank_communicator_changes_no_bit_of_the_six_call_shapes(tmp_path):
    code = CHILD % {"root": ROOT, "port": _free_port(), "tmp": str(tmp_path / "case")}
    r = subprocess.run([sys.executable, "-c", code], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout.splitlines(), r.stdout[-1500:] + r.stderr[-4000:]
