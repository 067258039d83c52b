"""Per-step time of the sharded MCMC step, parameters in -> band fluxes out, in two forms:

  native  bartrt_step_batch with the library's communicator attached (include/bartrt.h, bartrt_comm_init): one host
          call per step, the all-gather and the band integration inside the library;
  python  engine.step_batch_sharded(force=True) as Worker.step drives it: profiles launch, RT launch, padded torch
          all_gather_into_tensor, reassembly, band launch (four ctypes calls plus the torch copies).

Two shapes, ten walkers per step in total: the headline (100 layers x 1e4 samples, 4 molecules, 10 filters, energy
balance on) and WASP-12b (100 layers, 4 molecules, 4 filters) at 303 samples per rank, the block a rank holds at
N = 8.  At N = 1 the unsharded engine's plain bartrt_step_batch (no communicator) is timed too.

    python tools/sharded_step_bench.py [--steps 300] [--warmup 40] [--out profiles/sharded_step_bench.json]

runs N = 1 and, with more GPUs visible, N = all of them (8 at most), each under torch.distributed.run as a child
process with a time limit, and writes one JSON document."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOLS = ("H2O", "CO", "CO2", "CH4")
P0 = (-2.0, 0.0, 1.0, 0.0, 0.98, -0.5, -0.5, -0.5, -0.5)
NWALKERS = 10


def _shapes(world):
    return {"headline": dict(nwave=10000, wnlow=1000.0, nfilters=10, ebalance=True),
            "wasp12b_303_per_rank": dict(nwave=303 * world, wnlow=910.0, nfilters=4, ebalance=False)}


def _timed(fn, steps, warmup):
    import gc
    for i in range(warmup):
        fn(i)
    gc.collect()
    gc.disable()
    try:
        lat = np.zeros(steps)
        for i in range(steps):
            t = time.perf_counter()
            fn(i)
            lat[i] = time.perf_counter() - t
    finally:
        gc.enable()
    return {"median_us": float(np.median(lat) * 1e6), "mean_us": float(lat.mean() * 1e6),
            "p90_us": float(np.percentile(lat, 90) * 1e6)}


def worker(a):
    import torch
    import torch.distributed as dist
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    sys.path.insert(0, ROOT)
    from bart_amd import BARTfunc, engine, synthcfg
    out = {"nranks": world, "nwalkers": NWALKERS, "steps": a.steps, "warmup": a.warmup, "shapes": {}}
    for name, shp in _shapes(world).items():
        d = os.path.join(a.workdir, "%s_%d" % (name, world))
        if rank == 0:
            synthcfg.make_worker_case(d, nwave=shp["nwave"], wnlow=shp["wnlow"], opmol=MOLS, molfit=MOLS, params=P0,
                                      nfilters=shp["nfilters"], ebalance=shp["ebalance"])
        dist.barrier()
        w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(os.path.join(d, "BART.cfg")), shard=(rank, world),
                            device=local)
        nf = w.nfilters
        rng = np.random.default_rng(5)
        pars = np.array(P0) + rng.normal(0, [0.3, 0.2, 0.2, 0.05, 0.02, 0.5, 0.5, 0.5, 0.5], (16, NWALKERS, 9))
        pars[..., 3] = np.clip(pars[..., 3], 0, 1)
        res = {"nwave": shp["nwave"], "samples_per_rank": shp["nwave"] // world, "nfilters": nf}

        def python_step(i):
            d_par = torch.from_numpy(pars[i % 16]).cuda()
            band, status, _ = engine.step_batch_sharded(d_par, nf, force=True)
            return band.cpu().numpy(), status.cpu().numpy()

        res["python_sharded"] = _timed(python_step, a.steps, a.warmup)
        ref = python_step(0)
        if world == 1:
            res["plain_step_batch"] = _timed(lambda i: engine.step_batch(pars[i % 16], nf), a.steps, a.warmup)
        engine.comm_init()
        k0 = engine.comm_info()["ncollectives"]
        res["native_comm"] = _timed(lambda i: engine.step_batch(pars[i % 16], nf), a.steps, a.warmup)
        res["collectives_per_step"] = (engine.comm_info()["ncollectives"] - k0) / (a.steps + a.warmup)
        nb, ns = engine.step_batch(pars[0], nf)
        # (the Python path's band integration reads the reassembled spectra: the same bits as the native one)
        res["native_equals_python_bits"] = bool(np.array_equal(nb, ref[0]) and np.array_equal(ns, ref[1]))
        engine.comm_free()
        w.close()
        out["shapes"][name] = res
    if rank == 0:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dist.barrier()
    dist.destroy_process_group()


def _visible_gpus():
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c",
                        "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True)
    return int(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per torch.distributed.run child")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", help=argparse.SUPPRESS)
    ap.add_argument("--workdir", default=os.path.join(tempfile.gettempdir(), "bartrt_sharded_step_bench"))
    a = ap.parse_args()
    if a.worker:
        worker(a)
        return
    ngpu = _visible_gpus()
    if ngpu < 1:
        sys.exit("no GPU visible")
    runs = []
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for n in sorted({1, min(ngpu, 8)}):
        js = os.path.join(a.workdir, "n%d.json" % n)
        os.makedirs(a.workdir, exist_ok=True)
        if os.path.exists(js):
            os.remove(js)
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(29500 + n),
               os.path.abspath(__file__), "--worker", "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--json", js, "--workdir", a.workdir]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("N = %d failed (exit %d):\n%s\n%s" % (n, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
        runs.append(json.load(open(js)))
    doc = {"tool": "tools/sharded_step_bench.py", "visible_gpus": ngpu, "runs": runs}
    txt = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    for run in runs:
        for name, s in run["shapes"].items():
            print("N=%d %-22s native %7.1f us  python %7.1f us%s  (median per step)" % (
                run["nranks"], name, s["native_comm"]["median_us"], s["python_sharded"]["median_us"],
                "  plain %7.1f us" % s["plain_step_batch"]["median_us"] if "plain_step_batch" in s else ""))


if __name__ == "__main__":
    main()
