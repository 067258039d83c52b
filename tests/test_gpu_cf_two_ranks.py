"""Two real ranks on the contribution-function kernels (after tests/test_gpu_two_ranks.py): two processes, both on
device 0, each an engine on ITS wavenumber block (`--shard r 2`, 1777 = 888 + 889).  RCCL refuses two ranks on one
device, so the process group is gloo and the library's communicator is not used: each rank takes its part of the band
sums (bartrt_cf_partials_dev), the parts are exchanged through engine.allgather_blocks' pinned staging, and
bartrt_cf_combine_dev runs on both ranks.  The two ranks must end with identical bits, within 1e-11 (relative to the
row's largest |value|; the bound of tests/test_gpu_cf_blocks.py) of the unsharded engine's rows.  Every process is a
fresh child of pytest with a time limit of its own."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _env():
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    e.setdefault("OMP_NUM_THREADS", "1")
    return e


REF = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import numpy as np
import torch
from bart_amd import engine, synth, transit_module as trm
from test_gpu_cf import walkers
from test_gpu_step_blocks import _filters
case = synth.make_case(%(tmp)r + "/case", nlayers=60, nwave=1777, wnlow=1200.0, opmol=("CH4",), seed=11)
idx0, npts, resp, _ = _filters(1777, 2, np.random.default_rng(102))
profs = walkers(case, 5, seed=29)
profs[2, 7] = np.nan
over = np.full((5, 3), np.nan)
over[3, 1] = -1.5
engine.init(case.tcfg)
engine.cf_setup((idx0, npts, resp, None))
d, dov = torch.from_numpy(profs).cuda(), torch.from_numpy(over).cuda()
ok = torch.zeros(5, dtype=torch.uint8, device="cuda")
cfb = engine.contribution_dev(d, d_ok=ok, over=dov)
trb = engine.transmittance_dev(d, d_ok=ok, over=dov)
torch.cuda.synchronize()
assert ok.tolist() == [1, 1, 0, 1, 1]
np.savez(%(tmp)r + "/ref.npz", tcfg=case.tcfg, idx0=idx0, npts=npts, resp=resp, profs=profs, over=over,
         cf=cfb.cpu().numpy(), tr=trb.cpu().numpy())
trm.free_memory()
print("ok")
"""

CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
rank = int(sys.argv[1]); world = 2
import numpy as np
import torch
import torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=world)
from bart_amd import engine, transit_module as trm

ref = np.load(%(tmp)r + "/ref.npz")
win = (ref["idx0"], ref["npts"], ref["resp"], None)
engine.init(str(ref["tcfg"]), shard=(rank, world))
assert engine.local_range() == ((0, 888) if rank == 0 else (888, 1777))
nf, L = engine.cf_setup_block(win), engine.nlayers()
d, dov = torch.from_numpy(ref["profs"]).cuda(), torch.from_numpy(ref["over"]).cuda()
good = [0, 1, 3, 4]
out = {}
for kind, code in (("cf", engine.CF_CONTRIB), ("tr", engine.CF_TRANSMIT)):
    ok = torch.zeros(5, dtype=torch.uint8, device="cuda")
    part = engine.cf_partials_dev(d, code, d_ok=ok, over=dov)
    # every rank's part has the same size: the "blocks" of the exchange are the rows [5, nf * L] themselves
    both = engine.allgather_blocks(part.view(5, nf * L), total=world * nf * L)
    slots = both.view(5, world, nf * L).permute(1, 0, 2).contiguous()
    assert torch.equal(slots[rank].view(5, nf, L), part)
    band = engine.cf_combine_dev(slots, world, d_ok=ok)
    torch.cuda.synchronize()
    assert ok.tolist() == [1, 1, 0, 1, 1]
    got, want = band.cpu().numpy(), ref[kind]
    assert np.isnan(got[2]).all() and np.isfinite(got[good]).all()
    scale = np.max(np.abs(want[good]), axis=-1, keepdims=True)
    diff = float(np.max(np.abs(got[good] - want[good]) / np.where(scale > 0, scale, 1.0)))
    print("two ranks %%s rank %%d: largest difference from the unsharded rows %%.3e" %% (kind, rank, diff))
    assert diff < 1e-11, (kind, diff)
    out[kind] = got
np.savez(%(tmp)r + "/rank%%d.npz" %% rank, **out)
trm.free_memory()
dist.barrier()
dist.destroy_process_group()
print("ok %%d" %% rank)
"""


def test_two_ranks_combine_to_identical_bits_near_the_unsharded_rows(tmp_path):
    tmp = str(tmp_path)
    fmt = {"root": ROOT, "here": HERE, "tmp": tmp, "port": _free_port()}
    r = subprocess.run([sys.executable, "-c", REF % fmt], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout.splitlines(), r.stdout[-1500:] + r.stderr[-3000:]
    ps = [subprocess.Popen([sys.executable, "-c", CHILD % fmt, str(k)], env=_env(), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True) for k in range(2)]
    outs = []
    for p in ps:
        try:
            o, e = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in ps:
                q.kill()
            o, e = p.communicate()
        outs.append((p.returncode, o, e))
    for k, (rc, o, e) in enumerate(outs):
        assert rc == 0 and "ok %d" % k in o.splitlines(), o[-1500:] + e[-4000:]
        print(o)
    a, b = np.load(tmp + "/rank0.npz"), np.load(tmp + "/rank1.npz")
    for kind in ("cf", "tr"):
        assert np.array_equal(a[kind], b[kind], equal_nan=True), kind
