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

The batched calls on an initialised engine are ``bart_amd.engine.contribution`` /
``transmittance`` (host arrays) and ``contribution_dev`` / ``transmittance_dev`` (torch).
Plots stay out of scope.
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
