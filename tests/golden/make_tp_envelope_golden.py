"""Generates tp_envelopes.npz in this directory by IMPORTING the reference's own PT.py (as make_golden.py does; nothing
of it is copied): the T(p) envelopes of two small synthetic posteriors, taken as code/bestFit.py:429-466 takes them --
chains stacked after the burn-in, PT_generator on every sample, np.percentile / np.median over the samples.

    python tests/golden/make_tp_envelope_golden.py

Per model ("line", and the Madhusudhan model without inversion, "noinv") the file holds, data only:
    <m>_chain [nchains, nfree, niter]   an output.npy in MC3's layout; <m>_params, <m>_stepsize [npars]; <m>_burnin
    <m>_accepted [nsamples]             1 where PT_generator returned a profile inside Tmin ... Tmax (the reference's
                                        worker rejects the others, BARTfunc.py:318-330; the envelope is over these)
    <m>_median, _lo1, _hi1, _lo2, _hi2 [L]
    p [L], line_args [5], Tmin, Tmax
LAYER ORDER: the fixture's curves run TOP TO BOTTOM, the order of p (bar, ascending), which is how PT_generator
receives the pressure; the engine's atm order is the reverse.  The pressure grid and the TEP values are those of
bart_amd.synthcfg.make_worker_case(nwave=601, nlayers=60), which the test rebuilds.
"""
import os
import sys
import tempfile

import numpy as np

np.float = float  # noqa
np.int = int      # noqa
REF = "/root/reference"
sys.dont_write_bytecode = True   # nothing is written into the (read-only) reference tree
sys.path.insert(0, os.path.join(REF, "code"))
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import PT as pt               # noqa: E402
import reader as rd           # noqa: E402
import constants as c         # noqa: E402
import scipy.constants as sc  # noqa: E402

from bart_amd import synthcfg  # noqa: E402

CASE = dict(nwave=601, nlayers=60)
TMIN, TMAX = 400.0, 3000.0
NCHAINS, NITER, BURNIN = 4, 90, 15
LEVELS = (("lo1", 15.87), ("hi1", 84.13), ("lo2", 2.28), ("hi2", 97.72))

rng = np.random.default_rng(20261020)
with tempfile.TemporaryDirectory() as d:
    case, cfg = synthcfg.make_worker_case(d, **CASE)
    tep = rd.File(os.path.join(d, "planet.tep"))
    v = lambda k: float(tep.getvalue(k)[0])
    # BARTfunc.py:171-208
    tstar, rstar, sma = v("Ts"), v("Rs") * c.Rsun, v("a") * sc.au
    rplanet, mplanet = v("Rp") * c.Rjup, v("Mp") * c.Mjup
    gplanet = 100.0 * sc.G * mplanet / rplanet ** 2
    p = np.ascontiguousarray(case.press_bar[::-1])       # top -> bottom
out = {"p": p, "line_args": np.array([rstar, tstar, 100.0, sma, gplanet]), "Tmin": TMIN, "Tmax": TMAX}

MODELS = {
    # kappa, g1, g2, alpha, beta (box around the demo's starting point, BART_eclipse.cfg:80-83), log10 CH4 factor
    "line": dict(func=pt.PT_line, args=[rstar, tstar, 100.0, sma, gplanet, "const"],
                 params=[-2.0, 0.0, 1.0, 0.0, 0.98, -0.5], stepsize=[0.01, 0.01, 0.0, 0.01, 0.01, 0.1],
                 lo=[-2.6, -0.6, 1.0, 0.0, 0.70, -2.0], hi=[-1.6, 0.6, 1.0, 1.0, 1.90, 1.0]),
    # a1, a2, p1, p3, T3 (make_golden.py's ranges), log10 CH4 factor
    "noinv": dict(func=pt.PT_NoInversion, args=None,
                  params=[0.4, 0.2, 0.005, 2.0, 1600.0, -0.5], stepsize=[0.01, 0.01, 0.001, 0.0, 10.0, 0.1],
                  lo=[0.2, 0.04, 0.001, 2.0, 1500.0, -2.0], hi=[0.6, 0.5, 0.01, 2.0, 1700.0, 1.0]),
}
for name, m in MODELS.items():
    params, stepsize = np.array(m["params"]), np.array(m["stepsize"])
    lo, hi = np.array(m["lo"]), np.array(m["hi"])
    free = np.nonzero(stepsize)[0]
    chain = lo[free, None] + (hi - lo)[free, None] * rng.random((NCHAINS, len(free), NITER))
    # bestFit.py:436-438: chain after chain, past the burn-in
    stack = np.hstack([chain[k, :, BURNIN:] for k in range(NCHAINS)])
    nPT = len(params) - 1
    prof, accepted = [], []
    for k in range(stack.shape[1]):
        cur = params.copy()
        cur[free] = stack[:, k]                          # bestFit.py:449-456
        try:
            T = pt.PT_generator(p, cur[:nPT], m["func"], m["args"])
            ok = not (np.any(T < TMIN) or np.any(T > TMAX) or not np.all(np.isfinite(T)))
        except ValueError:
            T, ok = np.zeros(len(p)), False
        prof.append(T)
        accepted.append(ok)
    prof, accepted = np.array(prof), np.array(accepted)
    good = prof[accepted]
    print("%s: %d samples, %d accepted" % (name, len(prof), len(good)))
    assert 0 < len(good) and (name == "line" or len(good) < len(prof))
    out.update({name + "_chain": chain, name + "_params": params, name + "_stepsize": stepsize,
                name + "_burnin": BURNIN, name + "_accepted": accepted.astype(np.uint8),
                name + "_median": np.median(good, axis=0)})
    for key, q in LEVELS:                                # bestFit.py:461-465
        out[name + "_" + key] = np.percentile(good, q, axis=0)
np.savez_compressed(os.path.join(HERE, "tp_envelopes.npz"), **out)
print("wrote", os.path.join(HERE, "tp_envelopes.npz"), os.path.getsize(os.path.join(HERE, "tp_envelopes.npz")), "bytes")
