"""Posterior T(p) envelopes: the ``MCMC_PTprofiles`` figure's curves (reference code/bestFit.py:429-466) from a
finished chain, without a pass over the samples on the host.

bestFit.callTransit stacks the chains after burn-in, runs the T(p) model on every sample and takes the median and the
15.87 / 84.13 / 2.28 / 97.72 percentiles of the temperature at every layer.  Here the samples go through the step's
batched T(p) converter in chunks, their temperature rows stay in HBM, and the percentiles come from exact order
statistics selected on the GPU (include/bartrt.h, bartrt_posterior_tp; csrc/quant_core.hpp) and interpolated by
np.percentile's default rule.

    tp_envelopes(output_npy, cfg, burnin)   median, lo1, hi1, lo2, hi2 [L], status, ngood, pressure

Plots stay out of scope.
"""
from __future__ import annotations

import os

import numpy as np

from . import cf

# the curves in the order they are computed: the median, then cf.PERCENTILES
LEVELS = {"median": 50.0, **cf.PERCENTILES}


def envelopes_of_samples(samples, chunk=4096):
    """The envelope of full parameter vectors [n, npars] on an engine whose step is set up (BARTfunc.Worker):
    -> dict of ``median``, ``lo1``, ``hi1``, ``lo2``, ``hi2`` [L] (atm layer order; NaN when no sample was accepted),
    ``status`` [n] (0, 1 temperature, 2 abundance), ``ngood``, ``pressure`` [L] (barye, atm order)."""
    from . import engine
    env, status, ngood = engine.posterior_tp(samples, list(LEVELS.values()), chunk=max(1, int(chunk)))
    out = {k: env[i] for i, k in enumerate(LEVELS)}
    out.update(status=status, ngood=int(ngood), pressure=engine.pressure())
    return out


def tp_envelopes(output_npy, cfg, burnin, thinning=1, layout=None, chunk=4096, shard=None, device=None, group=None):
    """The T(p) envelopes of an MCMC posterior.  ``output_npy``: the output.npy of MC3 or of bart_amd.retrieve (a path
    or the array); ``cfg``: the run's configuration, whose [MCMC] section gives ``params`` / ``stepsize`` and everything
    BARTfunc.Worker reads.  The samples are expanded exactly as cf.posterior does (cf.posterior_samples: burn-in,
    thinning, chains stacked, fixed parameters from the cfg).  The engine is initialised on the cfg's ``tconfig`` and
    freed afterwards -- an engine this process had is replaced.  The T(p) model needs no spectrum, so a sharded engine
    (``shard``, ``device``, ``group`` as BARTfunc.Worker takes them) gives the same curves on every rank.
    -> dict: ``median``, ``lo1``, ``hi1``, ``lo2``, ``hi2`` [L] in atm layer order (the 50 / 15.87 / 84.13 / 2.28 /
    97.72 percentiles of bestFit.py:461-465 over the accepted samples; NaN when none was accepted), ``status`` [n],
    ``ngood``, ``pressure`` [L] (barye) and ``samples`` [n, npars]."""
    from . import BARTfunc
    params, stepsize = cf._mcmc_vectors(cfg)
    data = np.load(output_npy) if isinstance(output_npy, (str, bytes, os.PathLike)) else output_npy
    samples = cf.posterior_samples(data, params, stepsize, burnin, thinning, layout)
    wcfg = BARTfunc.WorkerConfig.from_cfg(cfg)
    extra = {} if shard is None and device is None else {"shard": shard, "device": device, "group": group}
    w = BARTfunc.Worker(wcfg, carry=False, **extra)
    try:
        out = envelopes_of_samples(samples, chunk)
    finally:
        w.close()
    out["samples"] = samples
    return out


def save(path, env):
    """tp_envelopes' curves as an .npz (retrieve --tp-envelopes): every key but ``samples``."""
    np.savez(path, **{k: v for k, v in env.items() if k != "samples"})
