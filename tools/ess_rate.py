"""What one effective-sample-size test costs (csrc/mcmc.hip: mcmc_ess_lags, mcmc_ess_finish), next to the Gelman-Rubin
test on the same rows and to one block of the resident loop.

    python tools/ess_rate.py [--rows 100000] [--chains 10] [--pars 9] [--maxlag 1024] [--repeat 3]
    python tools/ess_rate.py --probe-only       the two probe calls alone, once each after a warm-up: the run to put
                                                under a kernel trace, which gives the launches without the upload

Prints one JSON line per figure.  The probe calls (bartrt_mcmc_ess, bartrt_mcmc_gr) are timed whole: upload of the
chain, allocation of scratch and records, the launches, the read-back.  The block is the resident loop on the headline
shape (100 layers x 1e4 samples, 4 molecules, 10 filters, energy balance; ten chains, snooker, no tests): the median
interval between the progress reports of consecutive blocks of 256 iterations."""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from bart_amd import sampler  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--chains", type=int, default=10)
ap.add_argument("--pars", type=int, default=9)
ap.add_argument("--maxlag", type=int, default=1024)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--probe-only", action="store_true")
a = ap.parse_args()

rng = np.random.default_rng(3)
e = rng.normal(size=(a.chains, a.rows, a.pars))
chain = np.empty_like(e)
chain[:, 0] = e[:, 0]
for r in range(1, a.rows):                               # a first-order autoregression, coefficient 0.9: tau = 19
    chain[:, r] = 0.9 * chain[:, r - 1] + e[:, r]
step = np.full(a.pars, 0.1)
what = "%d chains x %d rows x %d free parameters" % (a.chains, a.rows, a.pars)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


ess_call = lambda: sampler.ess(chain, step, 0, a.rows, a.maxlag, 1000.0)
gr_call = lambda: sampler.gelman_rubin_dev(chain, step, 0, a.rows)
ess_call()
gr_call()
for _ in range(1 if a.probe_only else a.repeat):
    (tau, ess, trunc, _, reached), ms = timed(ess_call)
    print(json.dumps({"what": "bartrt_mcmc_ess, whole call, %s, %d lags" % (what, a.maxlag), "ms": round(ms, 3),
                      "tau_median": round(float(np.median(tau)), 2), "ess_min": round(float(ess.min()), 1),
                      "truncated": int(trunc.sum()), "reached_1000": reached}), flush=True)
    _, ms = timed(gr_call)
    print(json.dumps({"what": "bartrt_mcmc_gr, whole call, %s" % what, "ms": round(ms, 3)}), flush=True)
if a.probe_only:
    sys.exit(0)

from bart_amd import BARTfunc, synthcfg  # noqa: E402

mols = ("H2O", "CO", "CO2", "CH4")
truth = np.array([-1.5, -0.8, -0.8, 0.5, 1.0, -0.3, 0.2, -0.5, 0.1])
pmin, pmax = np.array([-5, -2, -2, 0, 0.55, -9, -9, -9, -9.0]), np.array([-1, 1, 1, 1, 1.2, 1.5, 1.5, 1.5, 1.5])
stepsize = np.array([0.01, 0.01, 0.01, 0.01, 0.001, 0.05, 0.05, 0.05, 0.05])
d = os.path.join(tempfile.gettempdir(), "bartrt_retrate_headline")
case, cfg = synthcfg.make_worker_case(d, reuse=True, nwave=10000, wnlow=1000.0, opmol=mols, molfit=mols,
                                      params=tuple(truth), nfilters=10, ebalance=True)
w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
data = w.step(truth)[0]
nch, blocks = 10, 6
scfg = sampler.SamplerConfig(params=truth + 0.02, pmin=pmin, pmax=pmax, stepsize=stepsize, data=data,
                             uncert=data * 0.01, nchains=nch, numit=blocks * 256 * nch, burnin=50, walk="snooker",
                             seed=1, grtest=False)
sampler.run_resident(w, dataclasses.replace(scfg, numit=256 * nch))          # warm-up
for _ in range(a.repeat):
    stamps = []
    sampler.run_resident(w, scfg, log=lambda m: stamps.append(time.perf_counter()) if m.startswith("step ") else None)
    gaps = np.diff(stamps[:blocks]) * 1e3
    print(json.dumps({"what": "one block of 256 iterations, resident loop, headline shape, ten chains, snooker",
                      "ms_median": round(float(np.median(gaps)), 3), "ms_all": [round(float(g), 3) for g in gaps]}),
          flush=True)
w.close()
