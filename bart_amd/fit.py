"""Least-squares fit before the chain: MC3's ``leastsq`` and ``chisqscale`` keys (examples/demo/BART_eclipse.cfg:98-100).

``fit`` runs a batched multi-start Levenberg-Marquardt optimisation inside the box through ``bartrt_fit``
(csrc/fit.hip, csrc/fit_core.hpp): every start's forward-difference Jacobian rows go to the model in one launch, every
start's ladder of damped trial points in the next, and a small kernel (one wave per start) decides in between.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .sampler import need_whole_grid_or_comm, problem_arrays

STATUS = ("running", "converged", "stalled", "iteration limit", "no physical start")
RUNNING, CONVERGED, STALLED, ITER_LIMIT, NO_START = range(5)


class FitOpts(C.Structure):
    """``bartrt_fit_opts`` of include/bartrt.h."""
    _fields_ = [("size", C.c_ulong), ("maxiter", C.c_long), ("nrungs", C.c_int), ("check", C.c_long),
                ("fdstep", C.c_double), ("ftol", C.c_double), ("xtol", C.c_double), ("lambda0", C.c_double),
                ("prior", C.c_void_p), ("priorlow", C.c_void_p), ("priorup", C.c_void_p), ("trace", C.c_void_p)]


DEFAULTS = dict(maxiter=50, nrungs=4, check=4, fdstep=1e-2, ftol=1e-10, xtol=1e-10, lambda0=1e-3)
_a = lambda v: np.ascontiguousarray(v, np.double)
_ptr = lambda v: v.ctypes.data_as(C.c_void_p)


def _options(pri, who, opts):
    unknown = set(opts) - set(DEFAULTS)
    if unknown:
        raise TypeError("%s: unknown option(s) %s" % (who, ", ".join(sorted(unknown))))
    o = dict(DEFAULTS, **opts)
    st = FitOpts(size=C.sizeof(FitOpts), maxiter=o["maxiter"] if o["maxiter"] > 0 else -1, nrungs=o["nrungs"],
                 check=o["check"], fdstep=o["fdstep"], ftol=o["ftol"], xtol=o["xtol"], lambda0=o["lambda0"])
    if pri is not None:
        st.prior, st.priorlow, st.priorup = (v.ctypes.data for v in pri)
    return o, st


def default_starts(cfg, nstarts: int, seed=None) -> np.ndarray:
    """``cfg.params`` first, then ``cfg.params + stepsize * N(0, 1)`` on the free parameters, clipped to the box; the
    draws come from ``numpy.random.default_rng(seed)``."""
    par, step = _a(cfg.params), _a(cfg.stepsize)
    free = np.where(step > 0)[0]
    x = np.tile(par, (nstarts, 1))
    rng = np.random.default_rng(seed)
    if nstarts > 1:
        x[1:, free] += step[free] * rng.normal(size=(nstarts - 1, len(free)))
        x[1:, free] = np.clip(x[1:, free], _a(cfg.pmin)[free], _a(cfg.pmax)[free])
    return x


def fit(worker, cfg, starts=None, nstarts=None, seed=None, **opts):
    """Levenberg-Marquardt from ``S`` starts at once, inside ``[cfg.pmin, cfg.pmax]``, on ``cfg.data`` / ``cfg.uncert``
    (and ``cfg.prior`` / ``priorlow`` / ``priorup`` when given); free, fixed and shared parameters as
    ``sampler.run_resident`` reads ``cfg.stepsize``.  ``starts`` [S, npars], or ``nstarts`` of :func:`default_starts`
    (default ``cfg.nchains``).  Options: ``maxiter`` 50, ``nrungs`` 4 (trial dampings per iteration), ``check`` 4
    (iterations between the host's looks at the starts still running), ``fdstep`` 1e-2 (of ``stepsize``: the forward
    difference), ``ftol`` = ``xtol`` 1e-10, ``lambda0`` 1e-3.  Needs an unsharded engine or the library's communicator
    (every rank then makes this call in lockstep and gets the same bits).

    Returns ``dict(best [S, npars], chisq [S], status [S] (indices of fit.STATUS), niter [S], bestp, best_chisq,
    trace [S, maxiter + 1, npars + 4])``: ``bestp`` is the lowest-chisq point among the starts that ran; a trace
    record holds x, chisq, lambda, the rung taken (-1: none) and the status after the start's own model (record 0) and
    after every iteration.

    Speed as measured (MEASUREMENTS.md row 18; one MI355X, tools/fit_rate.py, maxiter 50, medians of three): one start
    takes 10.6 ms on the WASP-12b shape (50 iterations, 101 model launches), 8.4 ms on the demo shape (50, 101) and
    11.7 ms on the headline shape (39, 79); scipy.optimize.least_squares calling engine.step_batch one model at a time
    from the same start takes 466 ms, 82 ms and 33 ms -- but ends at a LOWER chi-square on two of the three (8.5e-25
    against 2.5e-5, 2.564 against 3.350, 2.59988 against 2.60000), and most starts here run into the iteration limit
    on these degenerate problems.  Sixteen starts cost 2.27, 2.21 and 5.84 times one start, not "little more"; the
    best of the sixteen is better than the single start on every shape."""
    from . import transit_module as trm
    need_whole_grid_or_comm(worker, "fit")
    par, pmin, pmax, step, data, unc, pri = problem_arrays(cfg, "fit")
    npars = len(par)
    if starts is None:
        starts = default_starts(cfg, int(nstarts or cfg.nchains), seed)
    starts = _a(np.atleast_2d(starts))
    if starts.ndim != 2 or starts.shape[1] != npars or len(starts) < 1:
        raise ValueError("fit: starts is [nstarts, npars]")
    S = len(starts)
    o, st = _options(pri, "fit", opts)
    trace = np.zeros((S, max(o["maxiter"], 0) + 1, npars + 4))
    st.trace = trace.ctypes.data
    best, chisq = np.zeros((S, npars)), np.zeros(S)
    status, niter = np.zeros(S, np.intc), np.zeros(S, np.int64)
    nbad = (C.c_long * 4)()
    trm.check(trm.lib().bartrt_fit(S, npars, _ptr(starts), _ptr(pmin), _ptr(pmax), _ptr(step), len(data), _ptr(data),
                                   _ptr(unc), C.cast(C.byref(st), C.c_void_p), _ptr(best), _ptr(chisq), _ptr(status),
                                   _ptr(niter), C.cast(nbad, C.c_void_p)))
    for k in (1, 2, 3):
        worker.nbad[k] += int(nbad[k])
    ran = np.isfinite(chisq)
    if not ran.any():
        raise RuntimeError("fit: no start lies on a physical model: check params/pmin/pmax")
    ib = int(np.argmin(np.where(ran, chisq, np.inf)))
    return {"best": best, "chisq": chisq, "status": status, "niter": niter, "bestp": best[ib].copy(),
            "best_chisq": float(chisq[ib]), "trace": trace, "nbad": [int(nbad[k]) for k in range(4)]}


def covariance(worker, cfg, p, fdstep: float = 1e-2):
    """``(J^T J)^-1`` at the point ``p`` over the free parameters, J the forward-difference Jacobian of the residuals
    (data rows, then prior rows) from one more batch of ``nfree + 1`` models: MC3's "best-fit uncertainties" are the
    square roots of its diagonal.  Steps as the fit takes them (``fdstep * stepsize``, backwards at the upper bound)."""
    _, pmin, pmax, step, data, unc, pri = problem_arrays(cfg, "covariance")
    p = _a(p).copy()
    free = np.where(step > 0)[0]

    def shared(row):
        for j in np.where(step < 0)[0]:
            row[j] = row[int(-step[j]) - 1]
        return row

    def residuals(band, point):
        r = list((band - data) / unc)
        if pri is not None:
            for j in np.where((pri[1] != 0) | (pri[2] != 0))[0]:
                d = point[j] - pri[0][j]
                w = pri[1][j] if d < 0 else pri[2][j]
                r.append(d / w if w != 0 else 0.0)
        return np.array(r)
    rows, h = [shared(p.copy())], []
    for j in free:
        hj = fdstep * step[j]
        if p[j] + hj > pmax[j] or p[j] + hj < pmin[j]:
            hj = -hj
        row = p.copy()
        row[j] += hj
        rows.append(shared(row))
        h.append(hj)
    band = np.asarray(worker.step(np.array(rows)))
    if (band == -1.0).all(axis=1).any():
        raise RuntimeError("covariance: the model rejects the point or one of its forward-difference rows")
    r0 = residuals(band[0], rows[0])
    J = np.stack([(residuals(band[1 + q], rows[1 + q]) - r0) / h[q] for q in range(len(free))], axis=1)
    return np.linalg.inv(J.T @ J)
