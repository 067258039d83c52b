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

And the curves of the best-fit spectrum figure (reference code/bestFit.py:528-688) as envelopes over the posterior: what
the figure plots is the DISPLAY quantity, gaussian_filter1d(spectrum / sflux * rprs * rprs, 2) for an eclipse (:645-648)
and gaussian_filter1d(spectrum, 2) otherwise (:655, :662), beside the band-integrated points.  Every sample goes through
the step's whole run in chunks, one kernel turns a chunk's spectra into rows of the display quantity in HBM
(include/bartrt.h, bartrt_posterior_spectrum; csrc/specenv_core.hpp has the rule), and the percentiles of every grid
sample and of every band flux come from the same selection as T(p)'s.  The sample matrix takes nsamples * Wk * 8 bytes
of device memory, Wk = ceil(nwave / stride).

    spectrum_envelopes(output_npy, cfg, burnin)   wn, wl, median .. hi2 [Wk], band_median .. band_hi2 [F], meanwn, meanwl,
                                                  data, uncert, status, ngood (best=...: best_spectrum, best_band)

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
    """tp_envelopes' or spectrum_envelopes' curves, or marginals' arrays, as an .npz (retrieve --tp-envelopes,
    --spectrum-envelopes, --marginals): every key but ``samples``."""
    np.savez(path, **{k: v for k, v in env.items() if k != "samples"})


def gauss_half(sigma, truncate=4.0):
    """The half k = 0 .. radius of the weights scipy.ndimage.gaussian_filter1d(x, sigma, truncate=truncate) smooths
    with, made as SciPy makes them (_gaussian_kernel1d): radius = int(truncate * sigma + 0.5), exp(-0.5 / sigma**2 *
    k**2) over k = -radius .. radius, divided by their sum.  sigma 2 gives radius 8.  The library takes radii 0 .. 64."""
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError("gauss_half: sigma must be positive")
    radius = int(float(truncate) * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:])


def display_of_samples(samples, sigma=2.0, stride=1, chunk=4096, sflux=None, want_order=False):
    """The envelopes of the display quantity and of the band fluxes of full parameter vectors [n, npars] on an engine
    whose step is set up (BARTfunc.Worker) and holds the whole grid.  ``sflux`` [nwave]: the stellar flux on the
    engine's wavenumbers for an eclipse (stellar_flux), None for transit and direct geometry; ``sigma``: the smoothing
    (None or 0: none); ``stride``: every stride-th grid sample is kept.
    -> dict of ``median``, ``lo1``, ``hi1``, ``lo2``, ``hi2`` [Wk], ``band_median`` ... ``band_hi2`` [F] (NaN when no
    sample was accepted), ``status`` [n] (0, 1 temperature, 2 abundance, 3 energy balance), ``ngood``, ``wn`` [Wk];
    with ``want_order`` also ``ranks``, ``order``, ``band_order`` (None when no sample was accepted)."""
    from . import engine, transit_module as trm
    half = gauss_half(sigma) if sigma else np.ones(1)
    stride = int(stride)
    res = engine.posterior_spectrum(samples, list(LEVELS.values()), sflux, half, stride, chunk=max(1, int(chunk)),
                                    want_order=want_order)
    out = {k: res[0][i] for i, k in enumerate(LEVELS)}
    out.update({"band_" + k: res[1][i] for i, k in enumerate(LEVELS)})
    out.update(status=res[2], ngood=int(res[3]), wn=trm.get_waveno_arr(trm.get_no_samples())[::stride].copy())
    if want_order:
        out.update(ranks=res[4], order=res[5], band_order=res[6])
    return out


def stellar_flux(worker):
    """The stellar flux on the worker's wavenumber grid for an eclipse -- bestFit.py:645-646's
    si.interp1d(starwn, starfl)(specwn) of the Kurucz model the worker reads -- and None for the other geometries."""
    from . import hostio
    if worker.cfg.solution != "eclipse":
        return None
    starfl, starwn, _, _ = hostio.readkurucz(worker.cfg.kurucz, worker.tstar, worker.gstar)
    return np.interp(worker.specwn, starwn, starfl)


def read_best(best):
    """A full parameter vector from ``best``: the vector itself, or the path of a bestFit.txt as bart_amd.retrieve
    writes it (comment lines, then the parameters on one line)."""
    if isinstance(best, (str, bytes, os.PathLike)):
        best = np.loadtxt(best, comments="#")
    return np.ascontiguousarray(best, np.double).ravel()


def spectrum_envelopes_of_worker(worker, samples, sigma=2.0, stride=1, chunk=4096, best=None, data=None, uncert=None):
    """spectrum_envelopes on a live BARTfunc.Worker (retrieve --spectrum-envelopes): every key but ``samples``."""
    from . import hostio
    sflux = stellar_flux(worker)
    out = {}
    if best is not None:
        # the figure's blue curve and black points: one row through the same kernels (every percentile of one row is it)
        one = display_of_samples(read_best(best)[None], sigma, stride, 1, sflux)
        out.update(best_spectrum=one["median"], best_band=one["band_median"], best_status=int(one["status"][0]))
    out.update(display_of_samples(samples, sigma, stride, chunk, sflux))
    meanwn = []
    for f in worker.cfg.filters:
        fwn, ftr = hostio.readfilter(f)
        meanwn.append(np.sum(fwn * ftr) / sum(ftr))             # (bestFit.py:604)
    out.update(wl=1e4 / out["wn"], meanwn=np.array(meanwn), meanwl=1e4 / np.array(meanwn),
               data=np.asarray(data if data is not None else [], np.double),
               uncert=np.asarray(uncert if uncert is not None else [], np.double))
    return out


def spectrum_envelopes(output_npy, cfg, burnin, thinning=1, layout=None, sigma=2.0, stride=1, chunk=4096, best=None):
    """The envelopes of the best-fit spectrum figure's curves (bestFit.py:528-688) over an MCMC posterior.
    ``output_npy``, ``cfg``, ``burnin``, ``thinning``, ``layout``: as tp_envelopes takes them; the engine is initialised
    on the cfg's ``tconfig`` (the whole grid on one GPU: a wavenumber-sharded engine is refused) and freed afterwards.
    Every sample's spectrum becomes the display quantity -- for an eclipse gaussian_filter1d(spectrum / sflux * rprs *
    rprs, sigma) with sflux the Kurucz model interpolated onto the engine's wavenumbers, otherwise
    gaussian_filter1d(spectrum, sigma) -- on the GPU; ``stride`` keeps every stride-th grid sample (the smoothing runs
    on the full grid), and the sample matrix takes nsamples * ceil(nwave / stride) * 8 bytes of device memory.
    -> dict: ``wn``, ``wl`` (1e4 / wn) [Wk]; ``median``, ``lo1``, ``hi1``, ``lo2``, ``hi2`` [Wk] and ``band_median`` ...
    ``band_hi2`` [F] (the percentiles of LEVELS over the accepted samples; NaN when none was accepted); ``meanwn``,
    ``meanwl`` [F] (the filter-weighted mean wavenumber of bestFit.py:604, :618); ``data``, ``uncert`` from the cfg (read
    as bart_amd.retrieve reads it: the run's whole [MCMC] section is expected);
    ``status`` [n], ``ngood``, ``samples`` [n, npars].  ``best``: a full parameter vector or the path of a bestFit.txt
    adds ``best_spectrum`` [Wk] and ``best_band`` [F] (the figure's blue curve and black points; ``best_status`` says
    whether the vector was accepted), computed by the same kernels with one row."""
    from . import BARTfunc, sampler
    params, stepsize = cf._mcmc_vectors(cfg)
    data = np.load(output_npy) if isinstance(output_npy, (str, bytes, os.PathLike)) else output_npy
    samples = cf.posterior_samples(data, params, stepsize, burnin, thinning, layout)
    scfg = sampler.SamplerConfig.from_cfg(cfg)      # (the reader retrieve uses: `data` and `uncert` as the run had them)
    obs = (scfg.data, scfg.uncert)
    w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg), carry=False)
    try:
        out = spectrum_envelopes_of_worker(w, samples, sigma, stride, chunk, best, *obs)
    finally:
        w.close()
    out["samples"] = samples
    return out


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
