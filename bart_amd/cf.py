"""Contribution functions and band transmittance: BART's last stage (reference code/cf.py,
called at BART.py:626-644) on the engine's own optical depths.

The reference reruns ``transit`` with ``toomuch 1e100`` and ``savefiles yes``, parses the
``tau.dat`` it writes and band-averages the result in Python loops.  Here one batched kernel
walks the same layer records and opacity table the RT kernels read (include/bartrt.h,
bartrt_cf_batch) and returns the band-averaged curves of any number of profiles:

    filter_windows(wn, filter_files)   the filter windows of filter_cf, in numpy
    normalize(filt_cf)                 filt_cf_norm of filter_cf(..., normalize=True)
    cf(date_dir, atmfile, filters)     drop-in for cf.cf(..., plot=False)
    transmittance(date_dir, atmfile, filters)
                                       drop-in for cf.transmittance(..., plot=False)

    posterior(output_npy, cfg, filters, burnin)
                                       the curves of a whole MCMC posterior and their percentile envelopes
                                       (the CF / transmittance panel of bestFit.callTransit's figure)

The batched calls on an initialised engine are ``bart_amd.engine.contribution`` /
``transmittance`` (host arrays; ``over=`` gives every walker its own radius, cloud top and
scattering), ``contribution_dev`` / ``transmittance_dev`` (torch) and, from parameter vectors,
``contribution_from_params`` / ``transmittance_from_params``.  Plots stay out of scope.
"""
from __future__ import annotations

import os
import warnings

import numpy as np

from . import hostio


def filter_windows(wn, filter_files):
    """The windows filter_cf (code/cf.py:137-184) integrates over, on the grid ``wn`` (ascending):
    the samples strictly inside each filter's wavenumber range, the filter's response linearly
    interpolated onto them.  -> (idx0[nf], npts[nf], resp (the windows concatenated), trapz_resp[nf]),
    trapz_resp = np.trapz(resp) with unit spacing.  A filter with fewer than two grid samples inside
    it (the reference divides by a zero or empty trapz) raises ValueError."""
    wn = np.asarray(wn, np.double)
    if wn.ndim != 1 or wn.size < 2 or not np.all(np.diff(wn) > 0):
        raise ValueError("filter_windows: the wavenumber grid must be one-dimensional and ascending")
    idx0, npts, resp, trapz = [], [], [], []
    for path in filter_files:
        fwn, fresp = hostio.readfilter(path)
        order = np.argsort(fwn, kind="stable")
        fwn, fresp = fwn[order], fresp[order]
        inside = np.nonzero((wn > fwn[0]) & (wn < fwn[-1]))[0]
        if inside.size < 2:
            raise ValueError("filter %s: %s of the wavenumber grid (%g-%g cm-1) inside it (%g-%g cm-1)"
                             % (path, "no sample" if inside.size == 0 else "only one sample",
                                wn[0], wn[-1], fwn[0], fwn[-1]))
        r = np.interp(wn[inside], fwn, fresp)
        t = float(np.sum(0.5 * (r[:-1] + r[1:])))
        if not np.isfinite(t) or t == 0.0:
            raise ValueError("filter %s: no response inside the wavenumber grid" % path)
        idx0.append(int(inside[0]))
        npts.append(int(inside.size))
        resp.append(r)
        trapz.append(t)
    if not idx0:
        raise ValueError("filter_windows: no filters")
    return (np.array(idx0, np.int32), np.array(npts, np.int32), np.concatenate(resp), np.array(trapz))


def band_average(x, windows):
    """filter_cf's band average of per-wavenumber values x[..., W] -> [..., nfilters]: trapz(x resp) /
    trapz(resp) with unit spacing over each window (the host form of what the kernels compute)."""
    idx0, npts, resp, trapz = windows
    x = np.asarray(x, np.double)
    out = np.empty(x.shape[:-1] + (len(idx0),))
    off = 0
    for f, (i0, n) in enumerate(zip(idx0, npts)):
        y = x[..., i0:i0 + n] * resp[off:off + n]
        out[..., f] = np.sum(0.5 * (y[..., :-1] + y[..., 1:]), axis=-1) / trapz[f]
        off += n
    return out


def normalize(filt_cf):
    """filt_cf_norm (code/cf.py:174-181): every row (last axis = layers) mapped to [0, 1] by its own
    minimum and maximum; a constant row is returned unchanged, with a warning, as the reference does."""
    x = np.asarray(filt_cf, np.double)
    mn, mx = x.min(axis=-1, keepdims=True), x.max(axis=-1, keepdims=True)
    flat = (mx == mn)
    if np.any(flat):
        rows = np.argwhere(flat[..., 0])
        warnings.warn("contribution from %s %s is 0" % ("filter" if len(rows) == 1 else "filters",
                                                         ", ".join(str(tuple(r)) for r in rows)))
    return np.where(flat, x, (x - mn) / np.where(flat, 1.0, mx - mn))


def _find_tcfg(date_dir, tcfg):
    if tcfg is not None:
        return tcfg
    for name in ("cf_tconfig.cfg", "bestFit_tconfig.cfg"):
        p = os.path.join(date_dir, name)
        if os.path.exists(p):
            return p
    raise FileNotFoundError("no cf_tconfig.cfg or bestFit_tconfig.cfg in %s" % date_dir)


def _atm_profile(date_dir, atmfile):
    """The atm file's (S+1)*L profile (temperature, abundances; atm layer order) checked against the engine."""
    from . import engine
    species, p_bar, temp, abund = hostio.readatm(os.path.join(date_dir, atmfile))
    if list(species) != engine.species():
        raise ValueError("atm file %s: species %s, the transit configuration's atmosphere has %s"
                         % (atmfile, species, engine.species()))
    if len(p_bar) != engine.nlayers() or not np.allclose(p_bar * 1e6, engine.pressure(), rtol=1e-12, atol=0):
        raise ValueError("atm file %s: its pressure grid is not the transit configuration's" % atmfile)
    return np.vstack([temp, abund.T]).ravel()


def _dropin(date_dir, atmfile, filters, plot, tcfg, kind):
    from . import engine, transit_module as trm
    if plot:
        raise NotImplementedError("bart_amd.cf: plots are out of scope; call with plot=False and plot the returned "
                                  "curves (bestFit.py:489-510 does)")
    engine.init(_find_tcfg(date_dir, tcfg))
    try:
        prof = _atm_profile(date_dir, atmfile)
        if kind == "cf":
            filt, norm = engine.contribution(prof[None], filters, normalize=True)
            return filt[0], norm[0]
        return engine.transmittance(prof[None], filters)[0]
    finally:
        trm.free_memory()


def cf(date_dir, atmfile, filters, fext=".png", plot=False, tcfg=None):
    """Drop-in for code/cf.py's cf(date_dir, atmfile, filters, fext, plot=False): -> (filt_cf, filt_cf_norm),
    each [nfilters, nlayers] in atm layer order.  The engine is initialised on ``tcfg`` (default: the
    directory's cf_tconfig.cfg, else bestFit_tconfig.cfg; its `toomuch` does not matter) and freed afterwards
    -- an engine this process had is replaced.  The model is the atm file's own profile.  No executable runs
    and no tau.dat is written."""
    return _dropin(date_dir, atmfile, filters, plot, tcfg, "cf")


def transmittance(date_dir, atmfile, filters, fext=".png", plot=False, tcfg=None):
    """Drop-in for code/cf.py's transmittance(date_dir, atmfile, filters, fext, plot=False): -> the
    band-averaged exp(-tau) [nfilters, nlayers] in atm layer order (vertical depth on an eclipse engine,
    chord depth on a transit engine).  As cf() otherwise."""
    return _dropin(date_dir, atmfile, filters, plot, tcfg, "transmit")


# ---- a whole posterior (code/bestFit.py:429-525) ---------------------------------------------
# the 1- and 2-sigma levels of bestFit.py:461-465
PERCENTILES = {"lo1": 15.87, "hi1": 84.13, "lo2": 2.28, "hi2": 97.72}


def posterior_samples(output, params, stepsize, burnin, thinning=1, layout=None):
    """The full parameter vectors of a posterior: ``output`` as MC3 writes output.npy, [nchains, nfree, niter]
    (free parameters only), or as bart_amd.retrieve writes it, [nchains, nsteps, npars] (all parameters).  The
    two are told apart by the parameter count against ``stepsize`` (nfree = its non-zero entries, npars = its
    length); an array that fits both needs ``layout`` = 'mc3' or 'retrieve'.  The first ``burnin`` iterations of
    every chain are dropped, every ``thinning``-th of the rest is kept, and the chains are stacked one after the
    other (bestFit.py:436-438).  Free parameters are expanded to full ones as bestFit.callTransit does: entry i
    comes from the sample where stepsize[i] != 0 and from ``params`` where it is 0 (bestFit.py:449-456).  A
    negative stepsize (MC3's shared parameter) raises, as the sampler does.  -> [nsamples, npars]."""
    from .sampler import _check_stepsize
    stepsize = np.asarray(stepsize, np.double)
    params = np.asarray(params, np.double)
    _check_stepsize(stepsize)
    if params.shape != stepsize.shape or params.ndim != 1:
        raise ValueError("posterior: params (%d) and stepsize (%d) must be vectors of one length"
                         % (params.size, stepsize.size))
    data = np.asarray(output, np.double)
    if data.ndim != 3:
        raise ValueError("posterior: output.npy must be three-dimensional, not %s" % (data.shape,))
    free = np.nonzero(stepsize != 0.0)[0]
    npars, nfree = stepsize.size, free.size
    is_mc3, is_own = data.shape[1] == nfree, data.shape[2] == npars
    if layout is None:
        if is_mc3 and is_own:
            raise ValueError("posterior: an array of shape %s is both [nchains, nfree, niter] and [nchains, nsteps, "
                             "npars] for %d free of %d parameters; say layout='mc3' or layout='retrieve'"
                             % (data.shape, nfree, npars))
        if not (is_mc3 or is_own):
            raise ValueError("posterior: an array of shape %s is neither [nchains, nfree = %d, niter] nor [nchains, "
                             "nsteps, npars = %d]" % (data.shape, nfree, npars))
        layout = "mc3" if is_mc3 else "retrieve"
    if layout not in ("mc3", "retrieve") or not {"mc3": is_mc3, "retrieve": is_own}[layout]:
        raise ValueError("posterior: layout %r does not fit an array of shape %s" % (layout, data.shape))
    burnin, thinning = int(burnin), int(thinning)
    if burnin < 0 or thinning < 1:
        raise ValueError("posterior: burnin >= 0 and thinning >= 1")
    if layout == "mc3":
        kept = data[:, :, burnin::thinning].transpose(0, 2, 1).reshape(-1, nfree)    # chain after chain
        full = np.tile(params, (kept.shape[0], 1))
        full[:, free] = kept
    else:
        full = data[:, burnin::thinning, :].reshape(-1, npars).copy()
        full[:, stepsize == 0.0] = params[stepsize == 0.0]
    if full.shape[0] == 0:
        raise ValueError("posterior: no sample is left after a burn-in of %d iterations" % burnin)
    return np.ascontiguousarray(full)


def _mcmc_vectors(cfg):
    """``params`` and ``stepsize`` of the [MCMC] section."""
    import configparser
    cp = configparser.ConfigParser()
    cp.optionxform = str
    if not cp.read([cfg]):
        raise FileNotFoundError(cfg)
    d = dict(cp.items("MCMC"))
    for key in ("params", "stepsize"):
        if not d.get(key):
            raise ValueError("posterior: %s has no `%s` in its [MCMC] section" % (cfg, key))
    return (np.array([float(x) for x in d["params"].split()]), np.array([float(x) for x in d["stepsize"].split()]))


def _sharding(shard, group):
    """The (rank, count) of this process's wavenumber block: ``shard`` as Worker / engine.init take it, else
    BARTRT_GPUS = G > 1 over the G ranks of the process group (BARTfunc.main's convention), else None."""
    if shard is not None:
        return (int(shard[0]), int(shard[1]))
    ngpu = int(os.environ.get("BARTRT_GPUS", "1"))
    if ngpu <= 1:
        return None
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) != ngpu:
        raise ValueError("posterior: BARTRT_GPUS = %d needs a torch process group of that many ranks" % ngpu)
    return (dist.get_rank(group), ngpu)


def _device_envelopes(samples, win, kind, chunk):
    """The band curves of the samples kept in HBM as one [n, nfilters L] matrix, and their envelopes from order
    statistics selected there (engine.percentiles_dev) under the mask status == 0.  -> (band, status, envelopes): the
    host copies of the curves and flags, and the dict of median / lo1 / hi1 / lo2 / hi2 [nfilters, L]."""
    import torch
    from . import engine
    nf, L, n = engine.cf_setup(win), engine.nlayers(), len(samples)
    dev = torch.device("cuda", torch.cuda.current_device())
    band = torch.empty((n, nf * L), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    call = engine.contribution_from_params_dev if kind == "contribution" else engine.transmittance_from_params_dev
    for off in range(0, n, chunk):
        p = torch.from_numpy(np.ascontiguousarray(samples[off:off + chunk])).to(dev)
        b, st = call(p)
        band[off:off + len(p)] = b.reshape(len(p), nf * L)
        status[off:off + len(p)] = st
    ok = (status == 0).to(torch.uint8)
    levels = {"median": 50.0, **PERCENTILES}
    vals, _, _ = engine.percentiles_dev(band, list(levels.values()), ok)
    env = {k: vals[i].reshape(nf, L) for i, k in enumerate(levels)}
    return band.cpu().numpy().reshape(n, nf, L), status.cpu().numpy(), env


def _run_samples(cfg, samples, filters, kind, chunk, shard=None, device=None, group=None, envelopes="host"):
    """Worker, step and CF set up from the [MCMC] configuration as BARTfunc.Worker does; the samples in chunks.
    -> (band [nsamples, nfilters, L], status [nsamples], kind); with ``envelopes`` = "device" (band, status, the
    envelopes' dict, kind: _device_envelopes).  ``shard`` (rank, count) with count > 1: the engine
    holds its wavenumber block, the library's communicator is attached over ``group`` (engine.comm_init) and every
    rank, making the same calls, gets the same rows."""
    from . import BARTfunc, engine
    wcfg = BARTfunc.WorkerConfig.from_cfg(cfg)
    if kind is None:
        kind = "transmittance" if wcfg.solution == "transit" else "contribution"     # BART.py:637-644
    if kind not in ("contribution", "transmittance"):
        raise ValueError("posterior: kind is 'contribution' or 'transmittance'")
    w = BARTfunc.Worker(wcfg, shard=shard, device=device, group=group, carry=False)
    try:
        if shard is not None and shard[1] > 1:
            engine.comm_init(group)
        win = filter_windows(w.specwn, list(filters if filters is not None else wcfg.filters))
        if envelopes == "device":
            return _device_envelopes(samples, win, kind, chunk) + (kind,)
        bands, stats = [], []
        for off in range(0, len(samples), chunk):
            p = samples[off:off + chunk]
            if kind == "contribution":
                b, st = engine.contribution_from_params(p, win, normalize=False)
            else:
                b, st = engine.transmittance_from_params(p, win)
            bands.append(b)
            stats.append(st)
        return np.concatenate(bands), np.concatenate(stats), kind
    finally:
        w.close()


def posterior(output_npy, cfg, filters, burnin, thinning=1, kind=None, chunk=4096, layout=None, shard=None,
              device=None, group=None, envelopes="host"):
    """The band-averaged contribution functions or transmittance of every sample of an MCMC posterior, and their
    envelopes: what bestFit.callTransit (code/bestFit.py:429-525) draws beside the T(p) envelopes, for the whole
    posterior instead of the best fit.  ``output_npy``: the output.npy of MC3 or of bart_amd.retrieve (a path or the
    array; posterior_samples); ``cfg``: the run's configuration, whose [MCMC] section gives ``params`` /
    ``stepsize`` and everything BARTfunc.Worker reads; ``filters``: filter files (None: the cfg's).  ``kind``:
    'contribution' or 'transmittance'; default contribution for eclipse / direct, transmittance for transit
    (BART.py:637-644).  The engine is initialised on the cfg's ``tconfig`` and freed afterwards -- an engine this
    process had is replaced.  Every sample runs under its own radius, cloud top and scattering where the cfg fits
    them.  -> dict: ``samples`` [n, npars] (full parameters), ``band`` [n, nfilters, L] (atm layer order; NaN rows
    for rejected samples), ``status`` [n] (0, 1 temperature, 2 abundance), ``kind``, and over the accepted samples
    ``median``, ``lo1``, ``hi1``, ``lo2``, ``hi2`` [nfilters, L] (the 15.87 / 84.13 / 2.28 / 97.72 percentiles of
    bestFit.py:461-465; NaN when no sample was accepted).  No plots.
    ``shard`` = (rank, count), ``device``, ``group``: the sharding BARTfunc.Worker and engine.init take (or
    BARTRT_GPUS = G over a torch process group of G ranks) -- each rank's engine holds one wavenumber block, every
    rank calls posterior with the same arguments and returns the same curves and envelopes.
    ``envelopes``: 'host' (default) takes them with np.percentile on the host copy of the curves; 'device' keeps the
    curves in HBM as one [n, nfilters L] matrix and interpolates the envelopes from exact order statistics selected
    there (engine.percentiles_dev; csrc/quant_core.hpp) -- the same keys, ``band`` and ``status`` the same bits, the
    envelopes np.percentile's values (the same rule and expression).  'device' is not served on sharded engines
    (NotImplementedError)."""
    if envelopes not in ("host", "device"):
        raise ValueError("posterior: envelopes is 'host' or 'device'")
    params, stepsize = _mcmc_vectors(cfg)
    data = np.load(output_npy) if isinstance(output_npy, (str, bytes, os.PathLike)) else output_npy
    samples = posterior_samples(data, params, stepsize, burnin, thinning, layout)
    shard = _sharding(shard, group)
    extra = {} if shard is None and device is None else {"shard": shard, "device": device, "group": group}
    if envelopes == "device":
        if shard is not None and shard[1] > 1:
            raise NotImplementedError("posterior: envelopes='device' is not served on sharded engines; "
                                      "envelopes='host' is")
        band, status, env, kind = _run_samples(cfg, samples, filters, kind, max(1, int(chunk)), envelopes="device",
                                               **extra)
        return {"samples": samples, "band": band, "status": status, "kind": kind, **env}
    band, status, kind = _run_samples(cfg, samples, filters, kind, max(1, int(chunk)), **extra)
    out = {"samples": samples, "band": band, "status": status, "kind": kind}
    good = band[status == 0]
    if len(good):
        out["median"] = np.median(good, axis=0)
        for k, q in PERCENTILES.items():
            out[k] = np.percentile(good, q, axis=0)
    else:
        for k in ("median", *PERCENTILES):
            out[k] = np.full(band.shape[1:], np.nan)
    return out
