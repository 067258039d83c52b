"""GPU: what every retrieval entry point refuses alike (csrc/retrieval_host.hpp: check_retrieval), through the C
calls themselves: bartrt_mcmc_run_resident, bartrt_fit and -- where no engine is needed to tell -- bartrt_fit_probe
return BARTRT_EINVAL with a message under their own name, on the whole-grid engine of tests/test_gpu_mcmc_resident.py.
(A fresh process for the engine, with a time limit of its own.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import test_gpu_mcmc_resident as T
from bart_amd import BARTfunc, synthcfg, transit_module as trm
from bart_amd.fit import FitOpts
from bart_amd.sampler import McmcOpts
case, cfg = synthcfg.make_worker_case(%(tmp)r, **T.CASE)
worker = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
data = worker.step(np.array(T.P0))[0].copy()
sc = T.scfg(data, 4, "demc")
a = lambda v: np.ascontiguousarray(v, np.double)
p = lambda v: v.ctypes.data_as(C.c_void_p)
par, pmin, pmax, step, dat, unc = (a(v) for v in (sc.params, sc.pmin, sc.pmax, sc.stepsize, sc.data, sc.uncert))
NP, ND, S = 7, len(dat), 2
zeros = np.zeros(NP)
shared = step.copy()
shared[5], shared[6] = -1.0, -7.0       # parameter 6 (from 1) is a copy of the first; the last one names itself
lib = trm.lib()
chain, chis = np.zeros((4, 3, NP)), np.zeros((4, 3))
starts, best, chisq = a(np.tile(par, (S, 1))), np.zeros((S, NP)), np.zeros(S)
lam, D, cur, pband = np.ones(S), np.zeros((S, NP)), np.zeros((S, ND)), np.zeros((S, NP, ND))
pstatus, trial, valid = np.zeros((S, NP), np.intc), np.zeros((S, 4, NP)), np.zeros(S, np.intc)
out = {}
for name, stepsize, prior_fields, ndata in (("priors", step, ("prior", "priorup"), ND), ("stepsize", shared, (), ND),
                                            ("ndata", step, (), ND - 1)):
    mo, fo = McmcOpts(size=C.sizeof(McmcOpts), thin=1, block=8), FitOpts(size=C.sizeof(FitOpts), maxiter=3)
    for f in prior_fields:
        setattr(mo, f, zeros.ctypes.data)
        setattr(fo, f, zeros.ctypes.data)
    calls = {"mcmc_run_resident": lambda: lib.bartrt_mcmc_run_resident(
                 4, NP, C.c_long(3), p(par), p(pmin), p(pmax), p(stepsize), ndata, p(dat), p(unc),
                 C.cast(C.byref(mo), C.c_void_p), p(chain), p(chis), None, None, None),
             "fit": lambda: lib.bartrt_fit(S, NP, p(starts), p(pmin), p(pmax), p(stepsize), ndata, p(dat), p(unc),
                                           C.cast(C.byref(fo), C.c_void_p), p(best), p(chisq), None, None, None)}
    if name != "ndata":
        calls["fit_probe"] = lambda: lib.bartrt_fit_probe(
            S, NP, p(pmin), p(pmax), p(stepsize), ndata, p(dat), p(unc), C.cast(C.byref(fo), C.c_void_p), p(starts),
            p(lam), p(D), p(cur), p(pband), p(pstatus), p(trial), p(valid))
    for who, call in calls.items():
        rc = call()
        out[name + " " + who] = [rc, lib.bartrt_last_error().decode() if rc < 0 else ""]
# the engine is as it was: the unrefused problem runs
mo = McmcOpts(size=C.sizeof(McmcOpts), thin=1, block=8)
out["ok"] = [lib.bartrt_mcmc_run_resident(4, NP, C.c_long(3), p(par), p(pmin), p(pmax), p(step), ND, p(dat), p(unc),
                                          C.cast(C.byref(mo), C.c_void_p), p(chain), p(chis), None, None, None), ""]
worker.close()
print("RESULT " + json.dumps(out))
"""

WANT = {"priors": "prior, priorlow and priorup come together", "stepsize": "stepsize[6] = -7",
        "ndata": "data length must equal the number of filters"}


def test_the_entry_points_refuse_alike_under_their_own_names(tmp_path):
    code = CHILD % {"root": ROOT, "tmp": str(tmp_path / "case")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert out.pop("ok") == [0, ""]
    assert sorted(out) == sorted("%s %s" % (v, w) for v in WANT for w in ("mcmc_run_resident", "fit", "fit_probe")
                                 if (v, w) != ("ndata", "fit_probe"))
    for key, (rc, msg) in out.items():
        vector, who = key.split()
        print("%-28s %d  %s" % (key, rc, msg))
        assert rc == EINVAL, (key, rc, msg)
        assert msg.startswith(who + ": ") and WANT[vector] in msg, (key, msg)
    assert "shared" in out["stepsize fit"][1]
