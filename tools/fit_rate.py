"""Wall time of a converged least-squares fit (bart_amd.fit: bartrt_fit, csrc/fit.hip) at one start and at sixteen,
against what MC3's `leastsq` does with the same engine: scipy.optimize.least_squares (trf, the same box and
tolerances, scipy's own relative forward-difference step, x_scale = stepsize) calling engine.step_batch one model at a
time from the same start.  The two do not end at the same chisq; each line carries the one it reached.

    python tools/fit_rate.py [--shape headline|wasp|demo] [--repeat 3]

Shapes as tools/retrieval_rate.py.  The data are the engine's own band fluxes at a known point with a fixed 1 %
pattern on them (a zero-residual problem converges in a way no measured spectrum does); the start is 2 stepsizes off.
One JSON line per measurement: a warm-up, then `repeat` runs, median and spread (max - min)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from bart_amd import BARTfunc, engine, fit, sampler, synthcfg, transit_module as trm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=("headline", "wasp", "demo"), default="wasp")
ap.add_argument("--repeat", type=int, default=3)
a = ap.parse_args()

mols = ("H2O", "CO", "CO2", "CH4")
truth = np.array([-1.5, -0.8, -0.8, 0.5, 1.0, -0.3, 0.2, -0.5, 0.1])
pmin, pmax = np.array([-5, -2, -2, 0, 0.55, -9, -9, -9, -9.0]), np.array([-1, 1, 1, 1, 1.2, 1.5, 1.5, 1.5, 1.5])
step = np.array([0.01, 0.01, 0.01, 0.01, 0.001, 0.05, 0.05, 0.05, 0.05])
if a.shape == "headline":
    label = "headline shape (100 layers x 10000 samples, 4 molecules, 10 filters, energy balance)"
    kw = dict(nwave=10000, wnlow=1000.0, opmol=mols, molfit=mols, params=tuple(truth), nfilters=10, ebalance=True)
elif a.shape == "wasp":
    label = "WASP-12b shape (100 layers x 2424 samples, 4 molecules, 4 filters)"
    kw = dict(nwave=2424, wnlow=910.0, opmol=mols, molfit=mols, params=tuple(truth), nfilters=4)
else:
    label = "demo shape (100 layers x 2501 samples, CH4, 10 filters)"
    truth, pmin, pmax, step = truth[:6], pmin[:6], pmax[:6], step[:6]
    kw = dict(params=tuple(truth))
d = os.path.join(tempfile.gettempdir(), "bartrt_fitrate_" + a.shape)
case, cfg = synthcfg.make_worker_case(d, reuse=True, **kw)
w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
clean = w.step(truth)[0]
nf = len(clean)
data = clean * (1.0 + 0.01 * np.cos(1.0 + 2.0 * np.arange(nf)))
scfg = sampler.SamplerConfig(params=truth + 2.0 * step, pmin=pmin, pmax=pmax, stepsize=step, data=data,
                             uncert=0.01 * clean, nchains=16, seed=1)
free = np.where(step > 0)[0]
build_id = trm.lib().bartrt_build_id().decode()


def timed(fn):
    fn()                                                 # warm-up
    ts, out = [], None
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), max(ts) - min(ts), out


rows = {}
for S in (1, 16):
    med, spread, res = timed(lambda: fit.fit(w, scfg, nstarts=S, seed=1))
    iters = int(res["niter"].max())
    rows[S] = med
    print(json.dumps({"workload": "%s, least-squares fit, %d start(s)" % (label, S), "wall_ms": round(1e3 * med, 3),
                      "spread_ms": round(1e3 * spread, 3), "iterations": iters, "model_launches": 1 + 2 * iters,
                      "models": S * (1 + iters * (len(free) + 4)), "status": [fit.STATUS[s] for s in res["status"]],
                      "chisq_first_start": float(res["chisq"][0]), "best_chisq": res["best_chisq"],
                      "build_id": build_id}), flush=True)
    if S == 1:
        target = float(res["chisq"][0])
print(json.dumps({"workload": "%s, sixteen starts against one" % label, "ratio": round(rows[16] / rows[1], 3)}))

try:
    from scipy.optimize import least_squares
except ImportError:
    least_squares = None
if least_squares is not None:
    calls = [0]

    def residuals(v):
        p = scfg.params.copy()
        p[free] = v
        calls[0] += 1
        band, status = engine.step_batch(p[None, :], nf)
        return (band[0] - data) / scfg.uncert if status[0] == 0 else np.full(nf, 1e6)

    def scipy_fit():
        calls[0] = 0
        return least_squares(residuals, scfg.params[free], method="trf", bounds=(pmin[free], pmax[free]),
                             diff_step=None, x_scale=step[free], ftol=1e-10, xtol=1e-10, gtol=1e-10)
    med, spread, r = timed(scipy_fit)
    print(json.dumps({"workload": "%s, scipy least_squares (trf) on engine.step_batch, one model per call" % label,
                      "wall_ms": round(1e3 * med, 3), "spread_ms": round(1e3 * spread, 3), "models": calls[0],
                      "chisq": float(2.0 * r.cost), "chisq_of_the_fit": target, "scipy_status": int(r.status),
                      "speedup_one_start": round(med / rows[1], 2), "build_id": build_id}), flush=True)
w.close()
