"""Posterior T(p) envelopes: the ``MCMC_PTprofiles`` figure's curves (reference code/bestFit.py:429-466) from a
finished chain, without a pass over the samples on the host.

bestFit.callTransit stacks the chains after burn-in, runs the T(p) model on every sample and takes the median and the
15.87 / 84.13 / 2.28 / 97.72 percentiles of the temperature at every layer.  Here the samples go through the step's
batched T(p) converter in chunks, their temperature rows stay in HBM, and the percentiles come from exact order
statistics selected on the GPU (include/bartrt.h, bartrt_posterior_tp; csrc/quant_core.hpp) and interpolated by
np.percentile's default rule.

    tp_envelopes(output_npy, cfg, burnin)   median, lo1, hi1, lo2, hi2 [L], status, ngood, pressure

And the numbers behind MC3's ``histogram`` and ``pairwise`` figures (reference code/mc3plots.py:45-82): one 1-D histogram
per free parameter, one 2-D histogram per pair and the highest-density credible regions, counted on the GPU in one pass
over the stacked samples and equal to np.histogram / np.histogram2d (include/bartrt.h, bartrt_marginals;
csrc/hist_core.hpp).  No engine is needed for these.

    marginals(output_npy, cfg_or_stepsize, burnin)   index, edges, hist, outside, pairs, hist2d, hpd_*, nsamples
    marginals(..., kde=True)                         and kde_x, kde_pdf, kde_bw, mean, std, cr_*: the Gaussian kernel
                                                     density of every parameter and its credible regions (bartrt_kde)

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
    """tp_envelopes' curves, or marginals' arrays, as an .npz (retrieve --tp-envelopes, --marginals): every key but
    ``samples``."""
    np.savez(path, **{k: v for k, v in env.items() if k != "samples"})


# MC3's 1- and 2-sigma credible fractions
HPD_LEVELS = (0.6827, 0.9545)


def marginals_of_samples(samples, index, nbins=20, ranges=None, levels=HPD_LEVELS, kde=False, kde_points=128,
                         kde_bw="scott"):
    """The marginals of the columns ``index`` of full parameter vectors [n, npars] (numpy: uploaded in chunks; or a
    float64 CUDA tensor): see marginals for what comes back.  Needs no engine."""
    from . import engine
    index = np.asarray(index, np.int64).ravel()
    nbins = int(nbins)
    if index.size < 1 or nbins < 1:
        raise ValueError("marginals: at least one free parameter and one bin")
    host = isinstance(samples, np.ndarray)
    if ranges is None:
        lohi, nfinite = engine.marginals_range(samples, index)
        lohi, nfinite = (lohi, nfinite) if host else (lohi.cpu().numpy(), nfinite.cpu().numpy())
        if np.any(nfinite == 0):
            raise ValueError("marginals: parameter %d has no finite sample to take a range from"
                             % index[int(np.argmax(nfinite == 0))])
    else:
        lohi = np.array(ranges, np.double).reshape(index.size, 2)
    lohi = lohi.copy()
    same = lohi[:, 0] == lohi[:, 1]              # a parameter that never moved: numpy's rule
    lohi[same, 0] -= 0.5
    lohi[same, 1] += 0.5
    edges = np.stack([np.linspace(lo, hi, nbins + 1) for lo, hi in lohi])
    pairs = nbins <= 128
    h1, outside, h2 = engine.marginals(samples, index, edges, pairs=pairs)
    if not host:
        h1, outside, h2 = h1.cpu().numpy(), outside.cpu().numpy(), (h2.cpu().numpy() if pairs else None)
    h1, outside = h1.astype(np.int64), outside.astype(np.int64)
    nfree, nlev = index.size, len(levels)
    out = dict(index=index, edges=edges, hist=h1, outside=outside,
               pairs=np.array([(index[a], index[b]) for a in range(nfree) for b in range(a + 1, nfree)],
                              np.int64).reshape(-1, 2),
               hist2d=(h2.astype(np.int64) if pairs else np.zeros((0, nbins, nbins), np.int64)),
               levels=np.array(levels, np.double), nsamples=int(samples.shape[0]),
               hpd_mask=np.zeros((nlev, nfree, nbins), bool), hpd_lo=np.full((nlev, nfree), np.nan),
               hpd_hi=np.full((nlev, nfree), np.nan), hpd_runs=np.zeros((nlev, nfree), np.int64))
    for l, p in enumerate(levels):
        for s in range(nfree):
            mask, _, _, runs = engine.hpd(h1[s], p)
            out["hpd_mask"][l, s], out["hpd_runs"][l, s] = mask, runs
            if mask.any():
                inc = np.nonzero(mask)[0]
                out["hpd_lo"][l, s], out["hpd_hi"][l, s] = edges[s, inc[0]], edges[s, inc[-1] + 1]
    if kde:
        out.update(_kde_fields(samples, index, lohi, levels, int(kde_points), kde_bw))
    return out


def _kde_fields(samples, index, lohi, levels, npoints, bw):
    """marginals' kde_* and cr_* fields: the density of every parameter on np.linspace over the histogram's range
    (include/bartrt.h, bartrt_kde) and the credible regions of it (bartrt_hpd_pdf)."""
    from . import engine
    if not 1 <= npoints <= 1024:
        raise ValueError("marginals: kde_points is a number of grid points: 1 .. 1024")
    grid = np.stack([np.linspace(lo, hi, npoints) for lo, hi in lohi])
    pdf, stat, _ = engine.kde(samples, index, grid, bw)
    if not isinstance(samples, np.ndarray):
        pdf, stat = pdf.cpu().numpy(), stat.cpu().numpy()
    nfree, nlev = index.size, len(levels)
    out = dict(kde_x=grid, kde_pdf=pdf, kde_bw=stat[:, 3].copy(), mean=stat[:, 1].copy(), std=stat[:, 2].copy(),
               cr_mask=np.zeros((nlev, nfree, npoints), bool), cr_lo=np.full((nlev, nfree), np.nan),
               cr_hi=np.full((nlev, nfree), np.nan), cr_runs=np.zeros((nlev, nfree), np.int64))
    for l, p in enumerate(levels):
        for s in range(nfree):
            mask, _, _, runs = engine.hpd_pdf(pdf[s], p)
            out["cr_mask"][l, s], out["cr_runs"][l, s] = mask, runs
            if mask.any():
                out["cr_lo"][l, s], out["cr_hi"][l, s] = grid[s, mask].min(), grid[s, mask].max()
    return out


def marginals(output_npy, cfg_or_stepsize, burnin, thinning=1, nbins=20, ranges=None, levels=HPD_LEVELS, layout=None,
              kde=False, kde_points=128, kde_bw="scott"):
    """The numbers behind MC3's ``histogram`` and ``pairwise`` figures (reference code/mc3plots.py:45-82) from a
    finished chain: one 1-D histogram per free parameter, one 2-D histogram per pair of them, and the highest-density
    credible region of every parameter at each of ``levels`` -- counted on the GPU (include/bartrt.h, bartrt_marginals),
    equal to np.histogram / np.histogram2d integer for integer.  No engine and no opacity grid are needed.
    ``output_npy``: the output.npy of MC3 or of bart_amd.retrieve (a path or the array).  ``cfg_or_stepsize``: the run's
    configuration (its [MCMC] section gives ``stepsize``), or the stepsize vector itself; free parameters are those
    with stepsize > 0.  The samples are stacked as cf.posterior_samples does (burn-in, thinning, chain after chain).
    ``nbins``: 20 is MC3's own value (at most 1024; above 128 the pairs are left out).  ``ranges`` [nfree, 2]: the
    histogram ranges; None takes each parameter's smallest and largest finite sample (found on the GPU), and where the
    two are equal lo - 0.5, hi + 0.5, as numpy does.  The edges are np.linspace(lo, hi, nbins + 1).
    -> dict: ``index`` [nfree] (the free parameters), ``edges`` [nfree, nbins + 1], ``hist`` [nfree, nbins],
    ``outside`` [nfree, 3] (samples below the range, above it, NaN), ``pairs`` [npairs, 2] (parameter indices, a < b,
    a-major), ``hist2d`` [npairs, nbins, nbins] (first bin index: the first parameter of the pair), ``levels``, and per
    level ``hpd_mask`` [nlevels, nfree, nbins], ``hpd_lo`` / ``hpd_hi`` [nlevels, nfree] (the outer edges of the lowest
    and highest bin of the region, which ``hpd_runs`` [nlevels, nfree] says is one interval or several), ``nsamples``.
    The hpd_* region is taken on the histogram (csrc/hist_core.hpp).  ``kde`` = True adds the region MC3 reports, taken
    on a Gaussian kernel density estimate of the samples (include/bartrt.h, bartrt_kde; csrc/kde_core.hpp): ``kde_x``
    [nfree, kde_points] (np.linspace over the histogram's range of each parameter; at most 1024 points), ``kde_pdf``
    (scipy.stats.gaussian_kde(samples, kde_bw)(kde_x) over the finite samples; ``kde_bw``: 'scott', 'silverman' or a
    factor; NaN for a parameter that never moved), ``kde_bw`` [nfree] (the bandwidth h), ``mean``, ``std`` (ddof 1), and
    per level ``cr_mask`` [nlevels, nfree, kde_points], ``cr_lo`` / ``cr_hi`` (the smallest and largest grid value in
    the region) and ``cr_runs``.  The region's rule (bartrt_hpd_pdf) is this project's, stated against SciPy's density:
    MC3's own could not be read.  Every other key is what it is without ``kde``.  Pairwise panels stay histograms (MC3
    draws them from histogram2d); weighted samples are not served."""
    if isinstance(cfg_or_stepsize, (str, bytes, os.PathLike)):
        params, stepsize = cf._mcmc_vectors(cfg_or_stepsize)
    else:
        stepsize = np.asarray(cfg_or_stepsize, np.double)
        params = np.zeros_like(stepsize)         # (fixed parameters are not histogrammed: any value serves)
    data = np.load(output_npy) if isinstance(output_npy, (str, bytes, os.PathLike)) else output_npy
    samples = cf.posterior_samples(data, params, stepsize, burnin, thinning, layout)
    return marginals_of_samples(samples, np.nonzero(stepsize > 0)[0], nbins, ranges, levels, kde, kde_points, kde_bw)
