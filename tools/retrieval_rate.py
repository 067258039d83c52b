"""Iterations per second of the in-process batched sampler (DEMC / snooker, all chains evaluated by one model call per
iteration) in its three forms: the Python loop (sampler.run), the native host loop (sampler.run_native) and the loop
resident on the GPU (sampler.run_resident).

    python tools/retrieval_rate.py                        WASP-12b shape, 10 and 32 chains, every loop
    python tools/retrieval_rate.py --shape headline|wasp|demo [--loops native,resident,resident_nogr] [--repeat 3]
                                                          ten chains, snooker, 400 iterations after a warm-up run

Shapes: headline = 100 layers x 1e4 samples, 4 molecules, 10 filters, energy balance (the bench's step); wasp = the
WASP-12b retrieval grid (2424 samples, 4 molecules, 4 filters; BASELINE config 4's problem on one GPU); demo =
examples/demo (2501 samples, CH4, 10 filters).  With BARTRT_LIBPATH naming a library built from an earlier commit
(tools/ab_build.py) the resident row is left out: that library does not have the call."""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from bart_amd import BARTfunc, sampler, synthcfg, transit_module as trm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=("headline", "wasp", "demo"), default=None)
ap.add_argument("--loops", default="python,native,resident")
ap.add_argument("--repeat", type=int, default=1)
a = ap.parse_args()

mols = ("H2O", "CO", "CO2", "CH4")
truth = np.array([-1.5, -0.8, -0.8, 0.5, 1.0, -0.3, 0.2, -0.5, 0.1])
pmin, pmax = np.array([-5, -2, -2, 0, 0.55, -9, -9, -9, -9.0]), np.array([-1, 1, 1, 1, 1.2, 1.5, 1.5, 1.5, 1.5])
step = np.array([0.01, 0.01, 0.01, 0.01, 0.001, 0.05, 0.05, 0.05, 0.05])
shape = a.shape or "wasp"
if shape == "headline":
    label = "headline shape (100 layers x 10000 samples, 4 molecules, 10 filters, energy balance)"
    kw = dict(nwave=10000, wnlow=1000.0, opmol=mols, molfit=mols, params=tuple(truth), nfilters=10, ebalance=True)
elif shape == "wasp":
    label = "WASP-12b shape (100 layers x 2424 samples, 4 molecules, 4 filters)"
    kw = dict(nwave=2424, wnlow=910.0, opmol=mols, molfit=mols, params=tuple(truth), nfilters=4)
else:
    label = "demo shape (100 layers x 2501 samples, CH4, 10 filters)"
    truth, pmin, pmax, step = truth[:6], pmin[:6], pmax[:6], step[:6]
    kw = dict(params=tuple(truth))
d = os.path.join(tempfile.gettempdir(), "bartrt_retrate_" + shape)
case, cfg = synthcfg.make_worker_case(d, reuse=True, **kw)
w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
data = w.step(truth)[0]
loops = {"python": ("python loop", lambda c: sampler.run(w.step, c)),
         "native": ("native loop", lambda c: sampler.run_native(w, c)),
         "resident": ("resident loop", lambda c: sampler.run_resident(w, c)),
         # (the same loop without its Gelman-Rubin tests between blocks)
         "resident_nogr": ("resident loop, grtest off", lambda c: sampler.run_resident(w, dataclasses.replace(c, grtest=False)))}
if not hasattr(trm.lib(), "bartrt_mcmc_run_resident"):
    loops.pop("resident")
    loops.pop("resident_nogr")
build_id = trm.lib().bartrt_build_id().decode()
for nch in ((10, 32) if a.shape is None else (10,)):
    numit = 400 * nch
    scfg = sampler.SamplerConfig(params=truth + 0.02, pmin=pmin, pmax=pmax, stepsize=step, data=data,
                                 uncert=data * 0.01, nchains=nch, numit=numit, burnin=50, walk="snooker", seed=1)
    for key in a.loops.split(","):
        if key not in loops:
            continue
        name, fn = loops[key]
        fn(scfg)                                       # warm-up
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            res = fn(scfg)
            dt = time.perf_counter() - t0
            print(json.dumps({"workload": "%s, snooker DEMC, %d chains, %s" % (label, nch, name),
                              "iterations_per_s": round(numit / nch / dt, 1),
                              "model_evaluations_per_s": round(numit / dt),
                              "acceptance": round(res["accept_rate"], 3), "build_id": build_id}), flush=True)
w.close()
