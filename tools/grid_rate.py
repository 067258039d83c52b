"""Models per second of a model grid (`walk = unif`: sampler.run_grid, bartrt_grid_run, csrc/grid.hip) on the headline
grid (100 layers x 1e4 wavenumbers) at 10, 64 and 256 rows per iteration: whole spectra as double and as float, and
band fluxes, each with a sink that discards its chunks.  The comparison, in the same process and alternating with the
grid runs, is a bare loop of bartrt_step_batch_dev on the same row count with one device synchronise at the end: the
fastest way to the same models before there was a grid call, WITHOUT their output -- no draw, no pack, no copy to the
host.  ratio = grid / bare step says what drawing, packing and handing the rows over costs.

    python tools/grid_rate.py [--iters 200] [--chunk 16] [--repeat 3] [--rows 10 64 256]

One JSON line per measurement: a warm-up run, then `repeat` timed runs of `iters` iterations each (host clock around
work that ends in a device synchronise), median and spread (max - min) of the rate."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from bart_amd import BARTfunc, engine, sampler, synthcfg, transit_module as trm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--chunk", type=int, default=16)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--rows", type=int, nargs="+", default=[10, 64, 256])
a = ap.parse_args()

import torch  # noqa: E402

mols = ("H2O", "CO", "CO2", "CH4")
truth = np.array([-1.5, -0.8, -0.8, 0.5, 1.0, -0.3, 0.2, -0.5, 0.1])
pmin, pmax = np.array([-5, -2, -2, 0, 0.55, -9, -9, -9, -9.0]), np.array([-1, 1, 1, 1, 1.2, 1.5, 1.5, 1.5, 1.5])
step = np.array([0.01, 0.01, 0.01, 0.01, 0.001, 0.05, 0.05, 0.05, 0.05])
label = "headline shape (100 layers x 10000 samples, 4 molecules, 10 filters, energy balance)"
kw = dict(nwave=10000, wnlow=1000.0, opmol=mols, molfit=mols, params=tuple(truth), nfilters=10, ebalance=True)
d = os.path.join(tempfile.gettempdir(), "bartrt_gridrate_headline")
case, cfg = synthcfg.make_worker_case(d, reuse=True, **kw)
w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
build_id = trm.lib().bartrt_build_id().decode()
discard = lambda k, t0, params, status, models: None


def timed(fn, models):
    fn()                                                 # warm-up: every shape of the timed window
    rates = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        fn()
        rates.append(models / (time.perf_counter() - t0))
    return float(np.median(rates)), max(rates) - min(rates)


for rows in a.rows:
    scfg = sampler.SamplerConfig(params=truth, pmin=pmin, pmax=pmax, stepsize=step, data=np.zeros(0), uncert=np.zeros(0),
                                 nchains=rows, numit=rows * a.iters, walk="unif", seed=1, modelper=a.chunk)
    models = rows * a.iters
    # the bare step on one iteration's rows of the same grid (the samples of iteration 0), resident in device memory
    d_par = torch.tensor(sampler.grid_draws(1, 0, rows, truth, pmin, pmax, step), dtype=torch.float64, device="cuda")

    def bare():
        for _ in range(a.iters):
            engine.step_batch_dev(d_par, w.nfilters)
        torch.cuda.synchronize()

    runs = [("bare loop of step_batch_dev, no output", bare),
            ("grid, whole spectra f64", lambda: sampler.run_grid(w, scfg, sink=discard, spectra=True, f32=False)),
            ("grid, whole spectra f32", lambda: sampler.run_grid(w, scfg, sink=discard, spectra=True, f32=True)),
            ("grid, band fluxes f64", lambda: sampler.run_grid(w, scfg, sink=discard, spectra=False, f32=False))]
    base = None
    for name, fn in runs:
        med, spread = timed(fn, models)
        base = med if base is None else base
        print(json.dumps({"workload": "%s, %d rows, %s" % (label, rows, name), "models_per_s": round(med, 1),
                          "spread": round(spread, 1), "iterations": a.iters, "chunk": a.chunk,
                          "ratio_to_bare_step": round(med / base, 3), "build_id": build_id}), flush=True)
    # the bare step again, after the grid runs: how far the reference itself moved within the process
    med, spread = timed(bare, models)
    print(json.dumps({"workload": "%s, %d rows, bare loop again" % (label, rows), "models_per_s": round(med, 1),
                      "spread": round(spread, 1), "ratio_to_first_bare": round(med / base, 3)}), flush=True)
w.close()
