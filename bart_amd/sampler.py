"""In-process batched MCMC driver for the GPU worker.

The reference runs one OS process per chain and MC3 moves 6-9 doubles per step
over MPI (code/BARTfunc.py:309-399).  With the forward model batched on the GPU
the natural shape is the opposite: ONE process per GPU evaluates every chain of
the ensemble in a single ``Worker.step`` call.  This module is that loop:
differential-evolution MCMC (ter Braak 2006; the reference's ``walk = demc``)
and its snooker variant (ter Braak & Vrugt 2008; ``walk = snooker``) over the
keys of the reference's ``[MCMC]`` section -- ``params, pmin, pmax, stepsize,
nchains, numit, burnin, data, uncert, walk, grtest`` (examples/demo/
BART_eclipse.cfg:43-102).  ``stepsize = 0`` keeps a parameter fixed; proposals
outside [pmin, pmax] and models the worker rejects (``-1`` sentinels) are
refused, as in the reference.

On a wavenumber-sharded node every rank runs this same loop with the same seed:
the proposals are identical everywhere, each rank computes its block of every
spectrum and the all-gather inside the model call reassembles them.
"""
from __future__ import annotations

import configparser
import ctypes as C
from dataclasses import dataclass

import numpy as np


@dataclass
class SamplerConfig:
    params: np.ndarray
    pmin: np.ndarray
    pmax: np.ndarray
    stepsize: np.ndarray
    data: np.ndarray
    uncert: np.ndarray
    nchains: int = 10
    numit: int = 10000
    burnin: int = 500
    walk: str = "demc"
    grtest: bool = True
    seed: int = 0
    # read by run_resident alone (MC3's keys of the same names; `thinning`, `savemodel`)
    prior: np.ndarray | None = None
    priorlow: np.ndarray | None = None
    priorup: np.ndarray | None = None
    thinning: int = 1
    savemodel: str | None = None
    # read by retrieve (MC3's keys of the same names): a least-squares fit before the chain (fit.fit), and the
    # uncertainties rescaled to a reduced chi-square of one at its optimum
    leastsq: bool = False
    chisqscale: bool = False
    # read by run_resident alone: stop at the first Gelman-Rubin test that finds convergence (MC3's `grexit`); a test
    # every `grcheck` iterations (None: the multiple of the block nearest above nsteps / 10) against `grthreshold`
    grexit: bool = False
    grcheck: int | None = None
    grthreshold: float = 1.01
    # read by run_grid alone (`walk = unif`; MC3's key of the same name): iterations per chunk and per model file
    modelper: int = 0

    @classmethod
    def from_cfg(cls, path: str, section: str = "MCMC") -> "SamplerConfig":
        cp = configparser.ConfigParser()
        cp.optionxform = str
        cp.read([path])
        d = dict(cp.items(section))
        arr = lambda k: np.array([float(x) for x in d[k].split()])
        # a model grid (`walk = unif`) has no data: the reference fills the two keys with dummies, here they go unread
        none = np.zeros(0) if d.get("walk", "demc") == "unif" else None
        obs = lambda k: arr(k) if none is None or k in d else none
        return cls(params=arr("params"), pmin=arr("pmin"), pmax=arr("pmax"),
                   stepsize=arr("stepsize"), data=obs("data"), uncert=obs("uncert"),
                   nchains=int(d.get("nchains", 10)), numit=int(float(d.get("numit", 10000))),
                   burnin=int(d.get("burnin", 500)), walk=d.get("walk", "demc"),
                   grtest=d.get("grtest", "True").strip() == "True",
                   seed=int(d.get("seed", 0)),
                   prior=arr("prior") if "prior" in d else None,
                   priorlow=arr("priorlow") if "priorlow" in d else None,
                   priorup=arr("priorup") if "priorup" in d else None,
                   thinning=int(d.get("thinning", 1)), savemodel=d.get("savemodel") or None,
                   leastsq=d.get("leastsq", "False").strip() == "True",
                   chisqscale=d.get("chisqscale", "False").strip() == "True",
                   grexit=d.get("grexit", "False").strip() == "True",
                   grcheck=int(d["grcheck"]) if "grcheck" in d else None,
                   grthreshold=float(d.get("grthreshold", 1.01)),
                   modelper=int(float(d.get("modelper", 0))))


def gelman_rubin(chains: np.ndarray) -> np.ndarray:
    """chains [nchains, nsamples, npar] -> potential scale reduction per parameter."""
    m, n, _ = chains.shape
    mean_c = chains.mean(axis=1)
    W = chains.var(axis=1, ddof=1).mean(axis=0)
    B = n * mean_c.var(axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(((n - 1) / n * W + B / n) / W)


def gelman_rubin_dev(chain: np.ndarray, stepsize, r0: int = 0, r1: int | None = None, threshold: float = 0.0):
    """The resident loop's convergence test once on the device (``bartrt_mcmc_gr``; csrc/gr_core.hpp states the
    formula and the order of every sum): chain [nchains, nkept, npars], rows [r0, r1) of every chain ->
    (psrf [npars], 0 where ``stepsize <= 0``; triples [nchains, npars, 3] = n, mean, sum of squared deviations;
    converged).  Needs no engine."""
    from . import transit_module as trm
    chain = np.ascontiguousarray(chain, np.double)
    step = np.ascontiguousarray(stepsize, np.double)
    nch, nkept, npars = chain.shape
    if step.shape != (npars,):
        raise ValueError("gelman_rubin_dev: stepsize has one value per parameter")
    psrf, triples, conv = np.zeros(npars), np.zeros((nch, npars, 3)), C.c_int(0)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    trm.check(trm.lib().bartrt_mcmc_gr(ptr(chain), nch, C.c_long(nkept), npars, ptr(step), C.c_long(r0),
                                       C.c_long(nkept if r1 is None else r1), float(threshold), ptr(psrf),
                                       ptr(triples), C.cast(C.byref(conv), C.c_void_p)))
    return psrf, triples, bool(conv.value)


def ess(chain: np.ndarray, stepsize, r0: int = 0, r1: int | None = None, maxlag: int = 0, target: float = 0.0):
    """The resident loop's effective-sample-size test once on the device (``bartrt_mcmc_ess``; csrc/ess_core.hpp
    states the lagged sums, their order and Geyer's initial positive sequence): chain [nchains, nkept, npars], rows
    [r0, r1) of every chain, at most ``maxlag`` lags (0: 1024) -> (tau [nchains, npars] the integrated autocorrelation
    times, ess [npars] = sum over the chains of n / tau, truncated [nchains, npars] (the sequence ran out at the last
    lag), acf [nchains, npars, K + 1] the lagged sums S_k with K = min(maxlag, n - 1), reached: every free ess finite
    and >= ``target`` and nothing truncated).  Zeros where ``stepsize <= 0``.  One chain is enough.  Needs no engine."""
    from . import transit_module as trm
    chain = np.ascontiguousarray(chain, np.double)
    step = np.ascontiguousarray(stepsize, np.double)
    nch, nkept, npars = chain.shape
    if step.shape != (npars,):
        raise ValueError("ess: stepsize has one value per parameter")
    r1 = nkept if r1 is None else int(r1)
    K = max(min(int(maxlag) if maxlag else 1024, r1 - int(r0) - 1), 0)
    tau, stat, trunc = np.zeros((nch, npars)), np.zeros(npars), np.zeros((nch, npars), np.int32)
    acf, reached = np.zeros((nch, npars, K + 1)), C.c_int(0)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    trm.check(trm.lib().bartrt_mcmc_ess(ptr(chain), nch, C.c_long(nkept), npars, ptr(step), C.c_long(int(r0)),
                                        C.c_long(r1), C.c_long(int(maxlag)), float(target), ptr(tau), ptr(stat),
                                        ptr(trunc), ptr(acf), C.cast(C.byref(reached), C.c_void_p)))
    return tau, stat, trunc, acf, bool(reached.value)


def _grexit_ignored(cfg, log, who):
    if cfg.grexit and log is not None:
        log("%s: grexit is honoured by run_resident alone; this loop runs all of numit" % who)


def _check_stepsize(stepsize):
    """MC3 reads a negative stepsize as "shared with parameter -stepsize" (its
    `stepsize` key, examples/demo/BART_eclipse.cfg:84-87); run and run_native do
    not implement shared parameters and must not mistake them for fixed ones."""
    if (np.asarray(stepsize) < 0).any():
        raise ValueError("stepsize < 0 (a parameter shared with another one, in MC3's convention) is served by "
                         "run_resident and fit.fit alone: here give every parameter its own stepsize, or 0 to fix it")


def _check_walk(walk, who: str):
    """run and run_native serve DEMC and snooker.  MC3's other two walks are not DEMC under another name."""
    if walk in ("mrw", "unif"):
        raise ValueError("%s: walk = %s is not served by this loop (it would run DEMC in its place): "
                         "run_resident serves mrw (retrieve --resident), run_grid serves unif" % (who, walk))


def problem_arrays(cfg, who: str):
    """The retrieval problem of ``cfg`` as the library takes it: contiguous double arrays ``params, pmin, pmax,
    stepsize, data, uncert`` and ``[prior, priorlow, priorup]`` (or None where ``cfg`` has no priors)."""
    a = lambda v: np.ascontiguousarray(v, np.double)
    par, pmin, pmax, step, data, unc = (a(v) for v in (cfg.params, cfg.pmin, cfg.pmax, cfg.stepsize, cfg.data, cfg.uncert))
    given = [v is not None for v in (cfg.prior, cfg.priorlow, cfg.priorup)]
    pri = None
    if any(given):
        if not all(given):
            raise ValueError("%s: prior, priorlow and priorup come together" % who)
        pri = [a(v) for v in (cfg.prior, cfg.priorlow, cfg.priorup)]
        if any(v.shape != par.shape for v in pri):
            raise ValueError("%s: prior, priorlow and priorup have one value per parameter" % who)
    if any(v.shape != par.shape for v in (pmin, pmax, step)) or unc.shape != data.shape:
        raise ValueError("%s: pmin, pmax and stepsize have one value per parameter, uncert one per datum" % who)
    return par, pmin, pmax, step, data, unc, pri


def need_whole_grid_or_comm(worker, who: str):
    """The library's retrieval loops evaluate whole spectra: on a sharded engine only over its communicator."""
    from . import engine
    lo, hi = engine.local_range()
    if hi - lo != worker.nwave and engine.comm_info()["nranks"] == 0:
        raise ValueError("%s: the engine is sharded and has no communicator (engine.comm_init); use run()" % who)


def _result(chain, chis, naccept, nsteps, nch, cfg, thin=1, burnin=None, **extra):
    """The result dictionary of the three loops, from chain [nch, nkept, npars] and chis [nch, nkept] (every
    ``thin``-th of ``nsteps`` iterations): best point, Gelman-Rubin statistic past the burn-in (``burnin`` iterations
    of this chain; None: cfg.burnin), acceptance rate."""
    free = np.where(cfg.stepsize > 0)[0]
    ib = np.unravel_index(np.argmin(chis), chis.shape)
    post = chain[:, min((cfg.burnin if burnin is None else burnin) // thin, chain.shape[1] - 1):]
    gr = gelman_rubin(post[:, :, free]) if cfg.grtest and post.shape[1] > 3 and nch > 1 else None
    return {"chain": chain, "chisq": chis, "bestp": chain[ib], "best_chisq": float(chis[ib]),
            "accept_rate": naccept / (nsteps * nch), "grstat": gr, "free": free, **extra}


def run(model, cfg: SamplerConfig, log=None):
    """model(params[nchains, npars]) -> bandflux[nchains, ndata] (-1 rows = rejected).
    Returns dict(chain [nchains, nsteps, npars], chisq [nchains, nsteps], bestp,
    best_chisq, accept_rate, grstat)."""
    _check_walk(cfg.walk, "run")
    rng = np.random.default_rng(cfg.seed)
    _check_stepsize(cfg.stepsize)
    _grexit_ignored(cfg, log, "run")
    free = np.where(cfg.stepsize > 0)[0]
    nfree, nch = len(free), cfg.nchains
    nsteps = max(1, int(np.ceil(cfg.numit / nch)))
    npars = len(cfg.params)

    inv_unc = 1.0 / np.asarray(cfg.uncert, float)

    def chisq_of(p):
        m = np.asarray(model(p))
        bad = (m == -1.0).all(axis=1)            # the worker's rejection sentinel
        r = (m - cfg.data) * inv_unc
        c = np.einsum("ij,ij->i", r, r)
        c[bad] = np.inf
        return c

    # start: the configured point jittered by the stepsizes, inside the box
    x = np.tile(cfg.params, (nch, 1))
    x[:, free] += cfg.stepsize[free] * rng.normal(size=(nch, nfree))
    # the box applies to the free parameters; a fixed one keeps its configured
    # value even outside [pmin, pmax]
    clip_free = lambda v: np.clip(v[:, free], cfg.pmin[free], cfg.pmax[free])
    x[:, free] = clip_free(x)
    x[0] = cfg.params
    c = chisq_of(x)
    for _ in range(20):                      # re-draw chains that start on a rejected model
        bad = ~np.isfinite(c)
        if not bad.any():
            break
        xb = np.tile(cfg.params, (int(bad.sum()), 1))
        xb[:, free] += 0.1 * cfg.stepsize[free] * rng.normal(size=(len(xb), nfree))
        x[bad] = xb
        x[:, free] = clip_free(x)
        c = chisq_of(x)
    if not np.isfinite(c).any():
        raise RuntimeError("no chain starts on a physical model: check params/pmin/pmax")
    chain = np.zeros((nch, nsteps, npars))
    chis = np.zeros((nch, nsteps))
    naccept = 0
    gamma0 = 2.38 / np.sqrt(2 * max(nfree, 1))
    idx = np.arange(nch)
    snooker = cfg.walk == "snooker" and nch > 3
    pmin, pmax, step_free = cfg.pmin, cfg.pmax, cfg.stepsize[free]

    def others(excluded):
        """[B, nch] chain indices drawn uniformly from the chains not listed in
        `excluded` [B, nch, k] (distinct entries per chain), all at once."""
        k = excluded.shape[-1]
        draw = rng.integers(0, nch - k, size=excluded.shape[:-1])
        ex = np.sort(excluded, axis=-1)
        for j in range(k):                 # skip over the excluded ones in ascending order
            draw += draw >= ex[..., j]
        return draw

    # random numbers for a block of iterations at a time: the per-iteration loop
    # is then a dozen small array operations around one model call
    B = 256
    for t0 in range(0, nsteps, B):
        nb = min(B, nsteps - t0)
        me = np.broadcast_to(idx, (nb, nch))
        # a lone chain has no partner: the difference term vanishes, the jitter moves it
        r1 = others(me[..., None]) if nch > 1 else me
        r2 = others(np.stack([me, r1], axis=-1)) if nch > 2 else r1
        z = others(np.stack([me, r1, r2], axis=-1)) if snooker else None
        jit = 1e-3 * step_free * rng.normal(size=(nb, nch, nfree))
        gsn = rng.uniform(1.2, 2.2, size=(nb, nch, 1))
        logu = np.log(rng.random((nb, nch)))
        for b in range(nb):
            t = t0 + b
            xf = x[:, free]
            prop = x.copy()
            logjac = 0.0
            if snooker and t % 10 != 0:
                # snooker update: move along the line through a third chain
                xz = xf[z[b]]
                d = xf - xz
                nd = np.sqrt(np.einsum("ij,ij->i", d, d))[:, None]
                nd[nd == 0] = 1.0
                u = d / nd
                proj = np.einsum("ij,ij->i", xf[r1[b]] - xf[r2[b]], u)[:, None]
                pf = xf + gsn[b] * proj * u
                dn = pf - xz
                nd_new = np.sqrt(np.einsum("ij,ij->i", dn, dn))
                logjac = (nfree - 1) * (np.log(np.maximum(nd_new, 1e-300)) - np.log(nd[:, 0]))
            else:
                gam = 1.0 if t % 10 == 0 else gamma0
                pf = xf + gam * (xf[r1[b]] - xf[r2[b]]) + jit[b]
            prop[:, free] = pf
            inside = ((pf >= pmin[free]) & (pf <= pmax[free])).all(axis=1)
            if inside.all():
                cp = chisq_of(prop)
            else:
                cp = np.full(nch, np.inf)
                if inside.any():
                    cp[inside] = chisq_of(prop[inside])
            with np.errstate(invalid="ignore", over="ignore"):
                acc = (logu[b] < -0.5 * (cp - c) + logjac) & np.isfinite(cp)
            x[acc], c[acc] = prop[acc], cp[acc]
            naccept += int(acc.sum())
            chain[:, t], chis[:, t] = x, c
            if log is not None and (t + 1) % max(1, nsteps // 10) == 0:
                log("step %d/%d  best chisq %.4f  acceptance %.2f" % (
                    t + 1, nsteps, float(np.min(chis[:, :t + 1])), naccept / ((t + 1) * nch)))
    return _result(chain, chis, naccept, nsteps, nch, cfg)


def run_native(worker, cfg: SamplerConfig, log=None):
    """The same sampler through ``bartrt_mcmc_run`` (csrc/mcmc.hip): the loop,
    its random draws and the chi-square in C++, one batched model call per
    iteration -- about twice the iterations per second of :func:`run` at ten
    chains.  Needs an unsharded engine or, on a sharded one, the library's
    communicator (engine.comm_init): every rank then runs this same seeded loop
    in lockstep and gets the same chains.  Same result dictionary as :func:`run`."""
    _check_walk(cfg.walk, "run_native")
    from . import transit_module as trm
    need_whole_grid_or_comm(worker, "run_native")
    nch = cfg.nchains
    _check_stepsize(cfg.stepsize)
    _grexit_ignored(cfg, log, "run_native")
    nsteps = max(1, int(np.ceil(cfg.numit / nch)))
    par, pmin, pmax, step, data, unc, _ = problem_arrays(cfg, "run_native")     # (this loop takes no priors)
    npars = len(par)
    chain = np.zeros((nch, nsteps, npars))
    chis = np.zeros((nch, nsteps))
    nacc = C.c_long(0)
    nbad = (C.c_long * 4)()
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    trm.check(trm.lib().bartrt_mcmc_run(
        nch, npars, C.c_long(nsteps), ptr(par), ptr(pmin), ptr(pmax), ptr(step), len(data), ptr(data),
        ptr(unc), int(cfg.walk == "snooker"), C.c_ulonglong(cfg.seed), ptr(chain), ptr(chis),
        C.cast(C.byref(nacc), C.c_void_p), C.cast(nbad, C.c_void_p)))
    for k in (1, 2, 3):
        worker.nbad[k] += int(nbad[k])
    if log is not None:
        log("%d iterations of %d chains; best chisq %.4f  acceptance %.2f" % (
            nsteps, nch, float(chis.min()), nacc.value / (nsteps * nch)))
    return _result(chain, chis, nacc.value, nsteps, nch, cfg)


class McmcOpts(C.Structure):
    """``bartrt_mcmc_opts`` of include/bartrt.h."""
    _fields_ = [("size", C.c_ulong), ("snooker", C.c_int), ("seed", C.c_ulonglong), ("thin", C.c_long),
                ("block", C.c_long), ("prior", C.c_void_p), ("priorlow", C.c_void_p), ("priorup", C.c_void_p),
                ("progress", C.c_void_p), ("progress_user", C.c_void_p),
                ("burnin", C.c_long), ("grcheck", C.c_long), ("grthreshold", C.c_double), ("grexit", C.c_int),
                ("grstat", C.c_void_p), ("grwhen", C.c_void_p), ("ngr", C.c_int), ("ngr_out", C.c_void_p),
                ("first", C.c_long), ("start", C.c_void_p), ("done", C.c_void_p),
                ("walk", C.c_int)]


class McmcOptsEss(McmcOpts):
    """``bartrt_mcmc_opts`` with the fields appended after ``walk`` (the effective-sample-size tests).  The struct
    carries its size: a caller that fills ``McmcOpts`` alone, with its size, leaves them zero."""
    _fields_ = [("esstarget", C.c_double), ("essexit", C.c_int), ("maxlag", C.c_long), ("essstat", C.c_void_p),
                ("esstau", C.c_void_p)]


PROGRESS = C.CFUNCTYPE(None, C.c_long, C.c_long, C.c_void_p)
WALK_MRW = 2    # bartrt_mcmc_opts.walk (include/bartrt.h: BARTRT_WALK_MRW)


def draws(seed: int, t: int, nchains: int, npars: int) -> np.ndarray:
    """The resident sampler's draws of every chain at iteration ``t``, evaluated on the device
    (``bartrt_mcmc_draws``): [nchains, 9 + npars], columns as csrc/mcmc_core.hpp's ``draws_row``."""
    from . import transit_module as trm
    out = np.zeros((nchains, 9 + npars))
    trm.check(trm.lib().bartrt_mcmc_draws(C.c_ulonglong(seed), C.c_ulonglong(t), nchains, npars,
                                          out.ctypes.data_as(C.c_void_p)))
    return out


def run_resident(worker, cfg: SamplerConfig, log=None, block: int = 256, first: int = 0, start=None,
                 esstarget: float = 0.0, essexit: bool = False, maxlag: int = 0):
    """The sampler resident on the GPU through ``bartrt_mcmc_run_resident`` (csrc/mcmc.hip, csrc/mcmc_core.hpp):
    population, chi-squares and counters stay in device memory and an iteration is one small sampler launch plus the
    model's launches, enqueued without a host wait, ``block`` iterations at a time.  Its draws come from a
    counter-based generator keyed by ``cfg.seed``: a run can be restated draw for draw (tests/mcmc_restate.py); the
    stream is not :func:`run_native`'s.  ``cfg.walk``: ``demc``, ``snooker`` or ``mrw`` (Metropolis random walk: every
    free parameter moves by its stepsize times a normal, no partner chains; only this loop serves it).  Of the three loops only this one takes shared parameters (``stepsize = -k``:
    a copy of parameter k, counted from 1), Gaussian priors (``prior``, ``priorlow``, ``priorup``; ``chisq`` then
    holds the data term plus the prior terms), ``thinning`` and the per-sample band fluxes of ``savemodel``.  At most
    1024 chains and 64 parameters.  Sharded engines as :func:`run_native`: with the library's communicator every rank
    makes this call in lockstep and gets the same chains.

    Convergence.  With ``cfg.grtest`` the Gelman-Rubin statistic of the rows past ``cfg.burnin`` is computed on the
    device every ``cfg.grcheck`` iterations and after the last one (csrc/gr_core.hpp; default spacing: the multiple
    of ``block`` nearest above nsteps / 10; ``block`` itself is lowered to a given ``cfg.grcheck`` and raised to a
    multiple of the thinning, which changes no byte of the chain), and with ``cfg.grexit`` the run stops at the first test in which every free parameter lies
    below ``cfg.grthreshold``.  ``first`` / ``start`` resume a run: ``start`` [nchains, npars] are the last rows of
    the run before, ``first`` (a multiple of the thinning) the iterations it made; the call continues to the same
    total ceil(numit / nchains) with the draws of those iterations, so that the rows of both calls together are the
    bytes of one uninterrupted run.  The tests of a resumed call see that call's rows alone.

    Effective sample size.  ``esstarget`` > 0: at every such test the integrated autocorrelation time of every chain
    and free parameter and the effective sample size per free parameter are computed on the device as well
    (csrc/ess_core.hpp; at most ``maxlag`` lags, 0: 1024), and with ``essexit`` the run stops at the first test at
    which every free parameter has ``esstarget`` effective samples and no chain's sequence ran out at ``maxlag``
    (together with ``cfg.grexit``: at the first test where both hold).  One chain is enough for these tests, so they
    are made with ``walk = mrw`` and one chain, and with ``cfg.grtest`` off.

    Speed: SLOWER than :func:`run_native` as measured (MEASUREMENTS.md row 17; one MI355X, ten chains, snooker):
    7 745 against 9 045 iterations/s on the headline shape, 10 948 against 15 528 on the WASP-12b shape, 11 163
    against 14 896 on the demo shape -- the one-lane-per-chain sampler launch costs more than the host round trip it
    removes.  Opt-in for what else it gives; :func:`run_native` stays the default.  What the convergence tests cost
    at their default spacing: about 1 % on the headline shape at 400 iterations (two tests), no more than the loop's
    own run-to-run spread (MEASUREMENTS.md row 21).

    Returns the dictionary of :func:`run_native` (``chain`` [nchains, nkept, npars], ``chisq`` [nchains, nkept],
    nkept = ceil(done / thinning)) plus ``models`` [nchains, nkept, ndata]: the band fluxes of each chain's current
    state at the kept iterations; ``done``: the iterations this call made; ``grhistory``: (when [ntests] global
    iteration counts, psrf [ntests, npars]); ``converged``: whether the last test made found convergence; ``accepted``: the proposals accepted in those
    iterations; with ``esstarget``: ``essstat`` [ntests, npars] and ``esstau`` [ntests, nchains, npars] (None
    without)."""
    from . import transit_module as trm
    if cfg.walk == "unif":
        raise ValueError("run_resident: walk = unif is not a chain: run_grid makes model grids")
    need_whole_grid_or_comm(worker, "run_resident")
    nch = cfg.nchains
    total = max(1, int(np.ceil(cfg.numit / nch)))
    first = int(first)
    nsteps = total - first
    if nsteps < 1:
        raise ValueError("run_resident: the run before already made %d of %d iterations" % (first, total))
    thin = max(1, int(cfg.thinning))
    nkept = -(-nsteps // thin)
    par, pmin, pmax, step, data, unc, pri = problem_arrays(cfg, "run_resident")
    npars = len(par)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    grcheck = 0
    esstarget = float(esstarget)
    if esstarget < 0 or (essexit and not esstarget > 0):
        raise ValueError("run_resident: esstarget is the effective samples asked of every free parameter: > 0 with "
                         "essexit, 0 for no ESS tests")
    if (cfg.grtest and nch > 1) or esstarget > 0:
        if cfg.grcheck:                      # a spacing of the caller's: no block is longer than it
            block = min(block, int(cfg.grcheck))
        block = -(-block // thin) * thin
        grcheck = int(cfg.grcheck) if cfg.grcheck else max(1, -(-nsteps // (10 * block))) * block
    opts = McmcOptsEss(size=C.sizeof(McmcOptsEss), snooker=int(cfg.walk == "snooker"), seed=cfg.seed, thin=thin,
                       block=block, burnin=int(cfg.burnin), grcheck=grcheck, grthreshold=float(cfg.grthreshold),
                       grexit=int(bool(cfg.grexit)), first=first, walk=WALK_MRW if cfg.walk == "mrw" else 0,
                       esstarget=esstarget, essexit=int(bool(essexit)), maxlag=int(maxlag) if esstarget > 0 else 0)
    if pri is not None:
        opts.prior, opts.priorlow, opts.priorup = (v.ctypes.data for v in pri)
    if start is not None:
        start = np.ascontiguousarray(start, np.double)
        if start.shape != (nch, npars):
            raise ValueError("run_resident: start holds one row per chain")
        opts.start = start.ctypes.data
    if log is not None:
        report = PROGRESS(lambda it, acc, _: log("step %d/%d  acceptance %.2f" % (first + it, total, acc / (it * nch))))
        opts.progress = C.cast(report, C.c_void_p)
    ngr = nsteps // grcheck + 1 if grcheck > 0 else 0
    grstat, grwhen = np.zeros((max(ngr, 1), npars)), np.zeros(max(ngr, 1), np.int64)
    made, done = C.c_int(0), C.c_long(0)
    opts.grstat, opts.grwhen, opts.ngr = grstat.ctypes.data, grwhen.ctypes.data, ngr
    opts.ngr_out, opts.done = C.addressof(made), C.addressof(done)
    essstat, esstau = np.zeros((max(ngr, 1), npars)), np.zeros((max(ngr, 1), nch, npars))
    if esstarget > 0:
        opts.essstat, opts.esstau = essstat.ctypes.data, esstau.ctypes.data
    chain = np.zeros((nch, nkept, npars))
    chis = np.zeros((nch, nkept))
    models = np.zeros((nch, nkept, len(data)))
    nacc = C.c_long(0)
    nbad = (C.c_long * 4)()
    trm.check(trm.lib().bartrt_mcmc_run_resident(
        nch, npars, C.c_long(nsteps), ptr(par), ptr(pmin), ptr(pmax), ptr(step), len(data), ptr(data), ptr(unc),
        C.cast(C.byref(opts), C.c_void_p), ptr(chain), ptr(chis), ptr(models),
        C.cast(C.byref(nacc), C.c_void_p), C.cast(nbad, C.c_void_p)))
    for k in (1, 2, 3):
        worker.nbad[k] += int(nbad[k])
    # the rows of the iterations done (all of them unless grexit stopped the run)
    kd = -(-done.value // thin)
    chain, chis, models = (np.ascontiguousarray(v[:, :kd]) for v in (chain, chis, models))
    when, psrf = grwhen[:made.value].copy(), grstat[:made.value].copy()
    free = step > 0
    last_ok = lambda r: bool(free.any() and np.all(np.isfinite(r[free])) and np.all(r[free] < cfg.grthreshold))
    converged = made.value > 0 and last_ok(psrf[-1])
    if esstarget > 0:
        essstat, esstau = essstat[:made.value].copy(), esstau[:made.value].copy()
    else:
        essstat = esstau = None
    ess_line = lambda k: "Effective sample size after %d iterations: %s  (smallest: %.1f)" % (
        when[k], " ".join("%.1f" % v for v in essstat[k][free]), essstat[k][free].min() if free.any() else 0.0)
    if log is not None:
        for k in range(made.value):
            if nch > 1:                      # (one chain: the test was an ESS test alone)
                log("Gelman-Rubin after %d iterations: %s" % (when[k], " ".join("%.4f" % g for g in psrf[k][free])))
                if last_ok(psrf[k]):
                    log("All parameters have converged to within %.3g%% of unity." % (100.0 * (cfg.grthreshold - 1.0)))
            if essstat is not None:
                log(ess_line(k))
        if done.value < nsteps:
            log("%s: stopped after %d of %d iterations" % (
                " and ".join(w for w, on in (("grexit", cfg.grexit), ("essexit", essexit)) if on),
                first + done.value, total))
        log("%d iterations of %d chains; best chisq %.4f  acceptance %.2f" % (
            done.value, nch, float(chis.min()), nacc.value / (done.value * nch)))
        if essstat is not None and made.value > 0:
            log("At the end: " + ess_line(made.value - 1))
    return _result(chain, chis, nacc.value, done.value, nch, cfg, thin, burnin=max(0, cfg.burnin - first),
                   models=models, done=done.value, grhistory=(when, psrf), converged=converged,
                   accepted=nacc.value, essstat=essstat, esstau=esstau)


class McmcGroup(C.Structure):
    """``bartrt_mcmc_group`` of include/bartrt.h."""
    _fields_ = [("size", C.c_ulong), ("params", C.c_void_p), ("pmin", C.c_void_p), ("pmax", C.c_void_p),
                ("stepsize", C.c_void_p), ("data", C.c_void_p), ("uncert", C.c_void_p), ("prior", C.c_void_p),
                ("priorlow", C.c_void_p), ("priorup", C.c_void_p), ("seed", C.c_ulonglong), ("start", C.c_void_p)]


# what the groups of one call share (the other keys of a SamplerConfig are each group's own)
GROUP_COMMON = ("nchains", "numit", "walk", "thinning", "burnin", "grtest", "grexit", "grcheck", "grthreshold")


def run_resident_groups(worker, cfgs, log=None, first: int = 0, start=None, block: int = 256):
    """An ensemble: ``len(cfgs)`` INDEPENDENT retrievals on one engine in one resident loop
    (``bartrt_mcmc_run_resident_groups``; csrc/mcmc.hip: mcmc_advance_groups).  Per iteration there is one sampler
    launch, a workgroup per retrieval, and one batched model evaluation over the chains of all of them, so the
    launches one ten-chain retrieval leaves half empty are filled.  ``cfgs`` is a list of :class:`SamplerConfig`: each
    carries its own params, box, stepsizes (fixed and shared patterns included), data, uncert, priors and seed; the
    keys of ``GROUP_COMMON`` must agree (ValueError naming the first that differs), as must the parameter and data
    counts.  At most 1024 chains in all.  Group g draws as :func:`run_resident` on ``cfgs[g]`` alone does, and where
    the model's kernels give a row the same bits in both batch sizes its arrays are that run's bytes.

    Convergence tests as in :func:`run_resident`, on every group's own rows; with ``grexit`` the call stops at the
    first test that finds EVERY group converged.  ``first`` / ``start`` [ngroups, nchains, npars] resume all groups.

    Speed as measured (MEASUREMENTS.md row 23; one MI355X, ten chains per group, snooker, against consecutive
    :func:`run_resident` calls on the same configurations): 1.27 / 1.63 / 1.80 / 1.90 x the models/s at 2 / 4 / 6 / 8
    groups on the headline shape (1.42e5 models/s at six), 1.86 / 2.99 / 3.33 / 3.77 x on the WASP-12b shape; one
    group costs what :func:`run_resident` costs.

    Returns a list of :func:`run_resident`'s dictionaries, one per group, each with ``nbad`` (that group's models
    rejected with status 1, 2, 3) and ``converged_at``: the global
    iteration count at the first test that found that group converged (None: no test did)."""
    from . import transit_module as trm
    cfgs = list(cfgs)
    if not cfgs:
        raise ValueError("run_resident_groups: at least one configuration")
    c0, G = cfgs[0], len(cfgs)
    for g, cfg in enumerate(cfgs):
        for key in GROUP_COMMON:
            if getattr(cfg, key) != getattr(c0, key):
                raise ValueError("run_resident_groups: `%s` is %r in group %d and %r in group 0: the groups of one call "
                                 "share it" % (key, getattr(cfg, key), g, getattr(c0, key)))
    if c0.walk == "unif":
        raise ValueError("run_resident_groups: walk = unif is not a chain: run_grid makes model grids")
    need_whole_grid_or_comm(worker, "run_resident_groups")
    nch = c0.nchains
    total = max(1, int(np.ceil(c0.numit / nch)))
    first = int(first)
    nsteps = total - first
    if nsteps < 1:
        raise ValueError("run_resident_groups: the run before already made %d of %d iterations" % (first, total))
    thin = max(1, int(c0.thinning))
    nkept = -(-nsteps // thin)
    arrays = [problem_arrays(cfg, "run_resident_groups: group %d" % g) for g, cfg in enumerate(cfgs)]
    npars, ndata = len(arrays[0][0]), len(arrays[0][4])
    if any(len(a[0]) != npars or len(a[4]) != ndata for a in arrays):
        raise ValueError("run_resident_groups: every group has the same number of parameters and of data")
    grcheck = 0
    if c0.grtest and nch > 1:
        if c0.grcheck:
            block = min(block, int(c0.grcheck))
        block = -(-block // thin) * thin
        grcheck = int(c0.grcheck) if c0.grcheck else max(1, -(-nsteps // (10 * block))) * block
    opts = McmcOpts(size=C.sizeof(McmcOpts), snooker=int(c0.walk == "snooker"), thin=thin, block=block,
                    burnin=int(c0.burnin), grcheck=grcheck, grthreshold=float(c0.grthreshold),
                    grexit=int(bool(c0.grexit)), first=first, walk=WALK_MRW if c0.walk == "mrw" else 0)
    if start is not None:
        start = np.ascontiguousarray(start, np.double)
        if start.shape != (G, nch, npars):
            raise ValueError("run_resident_groups: start holds one row per group and chain")
    groups = (McmcGroup * G)()
    for g, (cfg, (par, pmin, pmax, step, data, unc, pri)) in enumerate(zip(cfgs, arrays)):
        groups[g] = McmcGroup(size=C.sizeof(McmcGroup), params=par.ctypes.data, pmin=pmin.ctypes.data,
                              pmax=pmax.ctypes.data, stepsize=step.ctypes.data, data=data.ctypes.data,
                              uncert=unc.ctypes.data, seed=cfg.seed)
        if pri is not None:
            groups[g].prior, groups[g].priorlow, groups[g].priorup = (v.ctypes.data for v in pri)
        if start is not None:
            groups[g].start = start[g].ctypes.data
    if log is not None:
        report = PROGRESS(lambda it, acc, _: log("step %d/%d  acceptance %.2f" % (first + it, total, acc / (it * nch * G))))
        opts.progress = C.cast(report, C.c_void_p)
    ngr = nsteps // grcheck + 1 if grcheck > 0 else 0
    grstat, grwhen = np.zeros((max(ngr, 1), G, npars)), np.zeros(max(ngr, 1), np.int64)
    made, done = C.c_int(0), C.c_long(0)
    opts.grstat, opts.grwhen, opts.ngr = grstat.ctypes.data, grwhen.ctypes.data, ngr
    opts.ngr_out, opts.done = C.addressof(made), C.addressof(done)
    chain, chis = np.zeros((G, nch, nkept, npars)), np.zeros((G, nch, nkept))
    models = np.zeros((G, nch, nkept, ndata))
    nacc, nbad, conv = np.zeros(G, np.int64), np.zeros((G, 4), np.int64), np.zeros(G, np.intc)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    trm.check(trm.lib().bartrt_mcmc_run_resident_groups(
        G, C.cast(groups, C.c_void_p), nch, npars, C.c_long(nsteps), ndata, C.cast(C.byref(opts), C.c_void_p),
        ptr(chain), ptr(chis), ptr(models), ptr(nacc), ptr(nbad), ptr(conv)))
    for k in (1, 2, 3):
        worker.nbad[k] += int(nbad[:, k].sum())
    kd = -(-done.value // thin)
    when = grwhen[:made.value].copy()
    out = []
    for g, cfg in enumerate(cfgs):
        step = arrays[g][3]
        free = step > 0
        psrf = grstat[:made.value, g].copy()
        last_ok = lambda r: bool(free.any() and np.all(np.isfinite(r[free])) and np.all(r[free] < cfg.grthreshold))
        if log is not None:
            for k in range(made.value):
                log("group %d: Gelman-Rubin after %d iterations: %s" % (g, when[k], " ".join("%.4f" % v for v in psrf[k][free])))
            log("group %d: %d iterations of %d chains; best chisq %.4f  acceptance %.2f" % (
                g, done.value, nch, float(chis[g, :, :kd].min()), nacc[g] / (done.value * nch)))
        res = _result(np.ascontiguousarray(chain[g, :, :kd]), np.ascontiguousarray(chis[g, :, :kd]), int(nacc[g]),
                      done.value, nch, cfg, thin, burnin=max(0, cfg.burnin - first),
                      models=np.ascontiguousarray(models[g, :, :kd]), done=done.value, grhistory=(when, psrf),
                      converged=made.value > 0 and last_ok(psrf[-1]), accepted=int(nacc[g]),
                      converged_at=int(when[conv[g]]) if 0 <= conv[g] < len(when) else None,
                      nbad=[int(v) for v in nbad[g, 1:]])
        out.append(res)
    if log is not None and done.value < nsteps:
        log("grexit: every group converged; stopped after %d of %d iterations" % (first + done.value, total))
    return out


class GridOpts(C.Structure):
    """``bartrt_grid_opts`` of include/bartrt.h."""
    _fields_ = [("size", C.c_ulong), ("seed", C.c_ulonglong), ("chunk", C.c_long), ("first", C.c_long),
                ("spectra", C.c_int), ("f32", C.c_int), ("sink", C.c_void_p), ("user", C.c_void_p)]


SINK = C.CFUNCTYPE(C.c_int, C.c_long, C.c_long, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def grid_draws(seed: int, t: int, nrows: int, params, pmin, pmax, stepsize) -> np.ndarray:
    """The samples of iteration ``t`` of a model grid, rows 0 .. nrows - 1, evaluated on the device
    (``bartrt_grid_draws``; csrc/grid_core.hpp): [nrows, npars].  Needs no engine."""
    from . import transit_module as trm
    par, lo, hi, step = (np.ascontiguousarray(v, np.double) for v in (params, pmin, pmax, stepsize))
    if any(v.shape != par.shape for v in (lo, hi, step)):
        raise ValueError("grid_draws: pmin, pmax and stepsize have one value per parameter")
    out = np.zeros((nrows, len(par)))
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    trm.check(trm.lib().bartrt_grid_draws(C.c_ulonglong(seed), C.c_ulonglong(t), nrows, len(par), ptr(par), ptr(lo),
                                          ptr(hi), ptr(step), ptr(out)))
    return out


def run_grid(worker, cfg: SamplerConfig, sink=None, spectra=True, f32=False, first=0, chunk=None):
    """A model grid (MC3's ``walk = unif``) through ``bartrt_grid_run`` (csrc/grid.hip, csrc/grid_core.hpp):
    niter = ceil(numit / nchains) iterations of ``cfg.nchains`` parameter vectors drawn uniformly in
    [``cfg.pmin``, ``cfg.pmax``] (fixed and shared parameters as in :func:`run_resident`), each evaluated by the batched
    model and kept with its WHOLE model row: the spectrum on the engine's grid (``spectra``, the default, what the
    reference's model files hold) or the band fluxes, as double or (``f32``) float.  A row the model rejects is -1 in
    every entry and carries its status (1 temperature, 2 abundance, 3 energy).  ``cfg.data`` / ``cfg.uncert`` are not
    read.  The draws are the counter-based generator's, keyed by ``cfg.seed``: sample (t, row) depends on nothing
    else, so ``first`` (with ``cfg.numit`` still the whole grid's) makes the iterations first .. niter - 1 alone, the
    bytes they have in the whole grid.

    The run goes in chunks of ``chunk`` iterations (default ``cfg.modelper``), two in flight on the device.  With a
    callable ``sink(k, t0, params, status, models)`` every chunk is forwarded as numpy VIEWS, valid during the call
    only -- params [n, nchains, npars], status [n, nchains], models [n, nchains, width], the iteration first, t0 the
    chunk's first global iteration; ``modelper = 0`` then means one chunk holding the whole run -- and the function
    returns ``{"nbad": [3], "models": count}``.  Returning a true value from the sink stops the run
    (``"stopped": True``); an exception raised in it stops the run and is raised again here.  With ``sink=None``
    everything is collected (in chunks of at most 256 iterations where ``modelper`` is 0) and returned as ``{"params":
    [nchains, niter, npars], "status": [nchains, niter], "models": [nchains, niter, width], "nbad": [3]}``.

    Sharded engines as :func:`run_native`: with the library's communicator every rank makes this call in lockstep and
    every rank receives the same whole rows.

    Speed as measured (MEASUREMENTS.md row 22; one MI355X, headline grid of 100 layers x 1e4 wavenumbers, chunks of
    16 iterations, a sink that discards; in brackets the ratio to a bare loop of ``bartrt_step_batch_dev`` on the same
    row count, which draws, packs and hands over nothing).  Whole spectra as double: 61 254 models/s at 10 rows
    (0.71), 101 006 at 64 (0.70), 113 448 at 256 (0.705).  As float: 64 921 (0.75), 116 261 (0.80), 129 317 (0.80).
    Band fluxes: 69 974 (0.81), 134 437 (0.93), 152 424 (0.95).  The chunk copies run on the engine's one stream
    behind the kernels; a second stream for them is the follow-up that row names."""
    from . import transit_module as trm
    need_whole_grid_or_comm(worker, "run_grid")
    nch = int(cfg.nchains)
    total = max(1, int(np.ceil(cfg.numit / nch)))
    first = int(first)
    niter = total - first
    if niter < 1 or first < 0:
        raise ValueError("run_grid: first = %d leaves none of the grid's %d iterations" % (first, total))
    par, pmin, pmax, step = (np.ascontiguousarray(v, np.double) for v in (cfg.params, cfg.pmin, cfg.pmax, cfg.stepsize))
    if any(v.shape != par.shape for v in (pmin, pmax, step)):
        raise ValueError("run_grid: pmin, pmax and stepsize have one value per parameter")
    npars = len(par)
    width = int(worker.nwave if spectra else worker.nfilters)
    if chunk is None:
        chunk = max(0, int(cfg.modelper))
        if sink is None and chunk == 0:
            chunk = min(niter, 256)
    dtype = np.float32 if f32 else np.double
    kept, failure = [], []
    state = {"models": 0, "stopped": False}

    def view(addr, shape, dt):
        n = int(np.prod(shape))
        return np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(addr), dtype=dt).reshape(shape)

    def forward(k, t0, n, p_par, p_st, p_rows, _):
        try:
            a = (view(p_par, (n, nch, npars), np.double), view(p_st, (n, nch), np.int32),
                 view(p_rows, (n, nch, width), dtype))
            state["models"] += n * nch
            if sink is None:
                kept.append(tuple(v.copy() for v in a))
                return 0
            if sink(k, t0, *a):
                state["stopped"] = True
                return 1
            return 0
        except BaseException as err:          # (no exception crosses the C frames: kept, and raised after the call)
            failure.append(err)
            return 1

    cb = SINK(forward)
    opts = GridOpts(size=C.sizeof(GridOpts), seed=cfg.seed, chunk=chunk, first=first, spectra=int(bool(spectra)),
                    f32=int(bool(f32)), sink=C.cast(cb, C.c_void_p))
    nbad = (C.c_long * 4)()
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    rc = trm.lib().bartrt_grid_run(nch, npars, C.c_long(niter), ptr(par), ptr(pmin), ptr(pmax), ptr(step),
                                   C.cast(C.byref(opts), C.c_void_p), C.cast(nbad, C.c_void_p))
    if failure:
        raise failure[0]
    if not state["stopped"]:
        trm.check(rc)
    for k in (1, 2, 3):
        worker.nbad[k] += int(nbad[k])
    counts = [int(nbad[k]) for k in (1, 2, 3)]
    if sink is not None:
        return {"nbad": counts, "models": state["models"], "stopped": state["stopped"]}
    cat = lambda j: np.ascontiguousarray(np.concatenate([c[j] for c in kept], axis=0).swapaxes(0, 1))
    return {"params": cat(0), "status": cat(1), "models": cat(2), "nbad": counts}
