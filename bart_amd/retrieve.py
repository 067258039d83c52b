"""Run a retrieval: the batched sampler driving the GPU worker.

    python -m bart_amd.retrieve -c BART.cfg [--out DIR]
    python -m torch.distributed.run --nproc-per-node 8 -m bart_amd.retrieve -c BART.cfg
    python -m torch.distributed.run --nproc-per-node 8 -m bart_amd.retrieve -c BART.cfg --native-sharded

The second form shards the wavenumber axis over the node's GPUs (one process
per GPU; every rank runs the same seeded sampler, each computes its block of
every spectrum, one RCCL all-gather per step reassembles them).  By default
the sharded ranks run the Python sampler loop; ``--native-sharded`` attaches
the library's own communicator and runs the native loop on every rank in
lockstep (include/bartrt.h, bartrt_comm_init).  Reads the
reference's ``[MCMC]`` keys (examples/demo/BART_eclipse.cfg) and writes
``output.npy`` (posterior sample [nchains, nsteps, npars]), ``bestFit.txt`` and
``MCMC.log`` in the output directory.  ``--resident`` runs the sampler resident
on the GPU (sampler.run_resident) and also honours ``prior`` / ``priorlow`` /
``priorup``, negative (shared) stepsizes, ``thinning`` and ``savemodel`` (the band
fluxes of every kept sample, [nchains, ndata, nkept], written under that file's
name in the output directory).  ``leastsq = True`` in the configuration, or ``--leastsq``, runs a multi-start
least-squares fit first (fit.fit, ``--fit-starts N`` starts, default ``nchains``): the log gets every start's status and
chi-square and the optimum's uncertainties, ``bestFit.txt`` holds the optimum instead of the chain's best sample, and
the chain starts from it.  ``chisqscale = True`` (with ``leastsq`` only, as in MC3) then multiplies ``uncert`` by
sqrt(best chisq / (ndata - nfree)).

``--resident`` also honours ``grexit = True``: the Gelman-Rubin statistic is computed on the GPU between blocks of
iterations (every test is logged) and the run stops at the first test that finds every free parameter converged.  It
writes ``state.npz`` beside ``output.npy`` (iterations made, seed, nchains, thinning, walk, parameter count, accepted
proposals, rejected models, best sample); ``--resident --resume`` reads both, refuses a configuration whose seed,
nchains, thinning, walk or parameter count differ, continues the chain to ``numit`` with the draws an uninterrupted
run would have made -- ``grexit`` applies again, to the new rows alone: set ``grexit = False`` to run to the end --
and writes the concatenated ``output.npy``, the concatenated ``savemodel`` file and an appended ``MCMC.log``.
``--resident`` is also the loop that serves ``walk = mrw``; the other two refuse it.

``--resident --ess-target N`` computes, at every such test and on the GPU as well, the integrated autocorrelation time
of every chain and the effective sample size (ESS) of every free parameter (csrc/ess_core.hpp); ``MCMC.log`` gains,
next to each Gelman-Rubin line and at the end, the line of ESS per free parameter and the smallest one.  ``--ess-exit``
stops the run at the first test at which every free parameter has N effective samples; with ``grexit = True`` at the
first test where both hold.

``--resident --datasets FILE`` runs an ENSEMBLE (sampler.run_resident_groups; INTEGRATION.md, "Ensembles"): FILE is an
``.npz`` with ``data`` [G, ndata] and optionally ``uncert`` [G, ndata] (default: the configuration's) and ``seed`` [G]
(default: the configuration's seed + g); the G retrievals advance in one resident loop and are written to
``group_000/`` ... ``group_<G-1>/`` of the output directory, each as a run of its own writes its files.  Not with
``--resume``, ``leastsq``, ``chisqscale`` or ``walk = unif``.

``walk = unif`` makes a MODEL GRID instead of a chain (sampler.run_grid; INTEGRATION.md, "Model grids"): parameters
drawn uniformly in [pmin, pmax], no ``data`` / ``uncert`` needed, every model kept whole.  It writes ``output.npy``
(the parameters, [nchains, niter, npars]), ``status.npy`` ([nchains, niter]) and the models under the name of
``savemodel``: one file [nchains, width, niter] with ``modelper = 0``, else ``<stem>/<stem>_<k, five digits>.npy`` of
``modelper`` iterations each, written as the chunks arrive.  Whole spectra by default; ``--grid-bands`` keeps band
fluxes, ``--grid-f32`` writes float.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np

from . import BARTfunc, sampler


def least_squares(w, scfg, nstarts, log):
    """The fit before the chain: logs it, moves scfg.params to the optimum and, with chisqscale, rescales scfg.uncert.
    Returns fit.fit's dictionary."""
    from . import fit
    nfree, ndata = int((np.asarray(scfg.stepsize) > 0).sum()), len(scfg.data)
    if scfg.chisqscale and ndata <= nfree:
        raise ValueError("chisqscale needs more data points than free parameters (%d data, %d free): the reduced "
                         "chi-square is not defined" % (ndata, nfree))
    res = fit.fit(w, scfg, nstarts=nstarts or scfg.nchains, seed=scfg.seed)
    for s in range(len(res["chisq"])):
        log("fit start %d: %s after %d iterations, chisq %.6g" % (
            s, fit.STATUS[res["status"][s]], res["niter"][s], res["chisq"][s]))
    log("least-squares optimum: chisq %.6g at %s" % (res["best_chisq"], " ".join("%.8g" % p for p in res["bestp"])))
    try:
        sig = np.sqrt(np.diag(fit.covariance(w, scfg, res["bestp"])))
        log("best-fit uncertainties: " + " ".join("%.4g" % v for v in sig))
    except (RuntimeError, np.linalg.LinAlgError) as err:
        log("best-fit uncertainties: not available (%s)" % err)
    scfg.params = res["bestp"].copy()
    if scfg.chisqscale:
        if not res["best_chisq"] > 0:
            raise ValueError("chisqscale: the fit ends at a chi-square of zero, which would scale every uncertainty to "
                             "zero")
        factor = float(np.sqrt(res["best_chisq"] / (ndata - nfree)))
        scfg.uncert = np.asarray(scfg.uncert, float) * factor
        log("chisqscale: uncertainties multiplied by %.6g (reduced chisq %.6g)" % (factor, factor * factor))
    return res


def model_grid(w, scfg, a, out, rank, log):
    """`walk = unif`: the grid through sampler.run_grid and its files (the module's docstring has the layout).
    Returns run_grid's dictionary of the collected run, or its counts where the models went to chunk files."""
    stem = os.path.basename(scfg.savemodel)
    stem = stem[:-4] if stem.endswith(".npy") else stem
    kw = dict(spectra=not a.grid_bands, f32=a.grid_f32)
    t0 = time.perf_counter()
    if rank == 0:
        os.makedirs(out, exist_ok=True)
    if scfg.modelper > 0:
        pars, stats = [], []
        if rank == 0:
            os.makedirs(os.path.join(out, stem), exist_ok=True)

        def sink(k, t0_, params, status, models):
            pars.append(params.copy())
            stats.append(status.copy())
            if rank == 0:                # MC3's layout of a model file: [nchains, width, iterations]
                np.save(os.path.join(out, stem, "%s_%05d.npy" % (stem, k)),
                        np.ascontiguousarray(models.transpose(1, 2, 0)))
        res = sampler.run_grid(w, scfg, sink=sink, **kw)
        res["params"] = np.ascontiguousarray(np.concatenate(pars, axis=0).swapaxes(0, 1))
        res["status"] = np.ascontiguousarray(np.concatenate(stats, axis=0).swapaxes(0, 1))
    else:
        res = sampler.run_grid(w, scfg, **kw)
        if rank == 0:
            np.save(os.path.join(out, stem + ".npy"), np.ascontiguousarray(res["models"].transpose(0, 2, 1)))
    dt = time.perf_counter() - t0
    nmodel = res["status"].size
    log("%d models in %.2f s (%.0f models/s); %d of them rejected" % (nmodel, dt, nmodel / dt, sum(res["nbad"])))
    log("Bad iterations due to temperature %d, abundance %d, energy %d" % (w.nbad[1], w.nbad[2], w.nbad[3]))
    if rank == 0:
        np.save(os.path.join(out, "output.npy"), res["params"])
        np.save(os.path.join(out, "status.npy"), res["status"])
    return res


def ensemble(w, scfg, path, out, rank, log, lines):
    """`--resident --datasets FILE`: one retrieval per row of FILE's ``data`` in one resident loop
    (sampler.run_resident_groups), each written to ``group_<g, three digits>/`` as a run of its own writes its files.
    Returns the list of the groups' result dictionaries."""
    import copy
    with np.load(path) as f:
        data = np.asarray(f["data"], float)
        uncert = np.asarray(f["uncert"], float) if "uncert" in f.files else None
        seeds = np.asarray(f["seed"]) if "seed" in f.files else None
    if data.ndim != 2 or data.shape[1] != len(scfg.data):
        raise ValueError("--datasets: `data` is %r; it holds one row of %d values per retrieval" % (
            data.shape, len(scfg.data)))
    G = len(data)
    if uncert is not None and uncert.shape != data.shape:
        raise ValueError("--datasets: `uncert` is %r and `data` %r" % (uncert.shape, data.shape))
    if seeds is not None and seeds.shape != (G,):
        raise ValueError("--datasets: `seed` holds one value per retrieval")
    cfgs = []
    for g in range(G):
        cfg = copy.copy(scfg)
        cfg.data = data[g].copy()
        cfg.uncert = uncert[g].copy() if uncert is not None else np.asarray(scfg.uncert, float).copy()
        cfg.seed = int(seeds[g]) if seeds is not None else int(scfg.seed) + g
        cfgs.append(cfg)
    t0 = time.perf_counter()
    before = dict(w.nbad)
    results = sampler.run_resident_groups(w, cfgs, log=log)
    dt = time.perf_counter() - t0
    nmodel = G * scfg.nchains * results[0]["done"]
    log("%d models of %d groups in %.2f s (%.0f models/s)" % (nmodel, G, dt, nmodel / dt))
    log("Bad iterations due to temperature %d, abundance %d, energy %d" % tuple(w.nbad[k] - before[k] for k in (1, 2, 3)))
    if rank != 0:
        return results
    for g, (cfg, res) in enumerate(zip(cfgs, results)):
        d = os.path.join(out, "group_%03d" % g)
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "output.npy"), res["chain"])
        np.savez(os.path.join(d, "state.npz"), **dict(state_of(cfg), iterations=res["done"], naccept=res["accepted"],
                                                      nbad=np.array(res["nbad"]), best_chisq=res["best_chisq"],
                                                      bestp=res["bestp"]))
        with open(os.path.join(d, "bestFit.txt"), "w") as f:
            f.write("# best-fit parameters, chisq = %.6f\n" % res["best_chisq"])
            f.write(" ".join("%.8g" % p for p in res["bestp"]) + "\n")
        if cfg.savemodel:
            name = os.path.join(d, os.path.basename(cfg.savemodel))
            np.save(name if name.endswith(".npy") else name + ".npy", np.ascontiguousarray(res["models"].transpose(0, 2, 1)))
        with open(os.path.join(d, "MCMC.log"), "w") as f:      # the call's lines and this group's
            mine = [l for l in lines if not l.startswith("group ") or l.startswith("group %d:" % g)]
            f.write("\n".join(mine) + "\n")
    return results


STATE_KEYS = ("seed", "nchains", "thinning", "walk", "npars")     # what a resumed run must share with the run before


def state_of(scfg):
    return {"seed": int(scfg.seed), "nchains": int(scfg.nchains), "thinning": max(1, int(scfg.thinning)),
            "walk": str(scfg.walk), "npars": len(scfg.params)}


def load_state(out, scfg):
    """output.npy and state.npz of the run before; ValueError naming the first key of STATE_KEYS that differs."""
    try:
        chain = np.load(os.path.join(out, "output.npy"))
        with np.load(os.path.join(out, "state.npz")) as f:
            state = {k: f[k][()] for k in f.files}
    except OSError as err:
        raise ValueError("--resume: no run to resume in %s (%s)" % (out, err))
    now = state_of(scfg)
    for k in STATE_KEYS:
        if str(state[k]) != str(now[k]):
            raise ValueError("--resume: `%s` is %s in the configuration and %s in the run to resume (%s): a chain "
                             "continues under the settings it began with" % (k, now[k], state[k], out))
    kept = -(-int(state["iterations"]) // now["thinning"])
    if chain.shape != (now["nchains"], kept, now["npars"]) or int(state["iterations"]) % now["thinning"]:
        raise ValueError("--resume: output.npy %r does not hold the %d iterations state.npz speaks of, or they do not "
                         "end on a kept row" % (chain.shape, int(state["iterations"])))
    return chain, state


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config_file", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--numit", type=int, default=None)
    ap.add_argument("--python-loop", action="store_true",
                    help="run the sampler loop in Python (sampler.run) instead of the native one")
    ap.add_argument("--native-sharded", action="store_true",
                    help="with WORLD_SIZE > 1: attach the library's communicator and run the native loop on every "
                         "rank (one collective per step inside the library) instead of the Python loop")
    ap.add_argument("--resident", action="store_true",
                    help="run the sampler resident on the GPU (sampler.run_resident): reproducible draws, shared "
                         "parameters, priors, thinning and the `savemodel` array of the configuration")
    ap.add_argument("--resume", action="store_true",
                    help="with --resident: continue the run whose output.npy and state.npz lie in the output directory")
    ap.add_argument("--ess-target", type=float, default=0.0, metavar="N",
                    help="with --resident: compute the effective sample size of every free parameter on the GPU "
                         "wherever a Gelman-Rubin test runs, and write it to MCMC.log")
    ap.add_argument("--ess-exit", action="store_true",
                    help="with --ess-target N: stop at the first test at which every free parameter has N effective "
                         "samples (with grexit = True: at the first test where both hold)")
    ap.add_argument("--datasets", default=None, metavar="FILE",
                    help="with --resident: an .npz with data[G][ndata] (optional uncert[G][ndata], seed[G]): G "
                         "independent retrievals in one resident loop, written to group_000/ ... (INTEGRATION.md, "
                         "\"Ensembles\")")
    ap.add_argument("--leastsq", action="store_true",
                    help="run the multi-start least-squares fit before the chain (fit.fit), as `leastsq = True` in "
                         "the configuration does")
    ap.add_argument("--fit-starts", type=int, default=None, help="starts of that fit (default: nchains)")
    ap.add_argument("--grid-bands", action="store_true",
                    help="with walk = unif: keep the band fluxes of every model instead of its whole spectrum")
    ap.add_argument("--grid-f32", action="store_true", help="with walk = unif: write the models as float")
    ap.add_argument("--tp-envelopes", action="store_true",
                    help="after the run (after --resume: on the whole chain) write tp_envelopes.npz beside output.npy: "
                         "the median and the 1- and 2-sigma percentiles of T(p) over the rows past the burn-in "
                         "(bart_amd.posterior; not with walk = unif or --datasets)")
    ap.add_argument("--spectrum-envelopes", action="store_true",
                    help="after the run (after --resume: on the whole chain) write spectrum_envelopes.npz beside "
                         "output.npy: the median and the 1- and 2-sigma percentiles of the smoothed model spectrum (flux "
                         "ratio for an eclipse) and of the band fluxes over the rows past the burn-in, and the best fit's "
                         "curve and points (bart_amd.posterior.spectrum_envelopes; on one GPU; not with walk = unif or "
                         "--datasets)")
    ap.add_argument("--marginals", default=None, metavar="FILE.npz",
                    help="after the run (after --resume: on the whole chain) write the free parameters' 1-D and "
                         "pairwise histograms and their highest-density regions over the rows past the burn-in to "
                         "FILE.npz (a relative name: beside output.npy; bart_amd.posterior.marginals; not with walk = "
                         "unif or --datasets)")
    ap.add_argument("--marginals-bins", type=int, default=20, metavar="N",
                    help="with --marginals: bins per parameter (default 20, MC3's own)")
    ap.add_argument("--marginals-kde", action="store_true",
                    help="with --marginals: add every free parameter's Gaussian kernel density estimate and the credible "
                         "regions taken on it (kde_x, kde_pdf, kde_bw, mean, std, cr_*; bart_amd.posterior.marginals)")
    ap.add_argument("--marginals-kde-points", type=int, default=128, metavar="N",
                    help="with --marginals-kde: grid points per parameter (default 128; 1 .. 1024)")
    a = ap.parse_args(argv)
    if a.marginals_kde and not a.marginals:
        ap.error("--marginals-kde adds to the file --marginals writes: name it with --marginals FILE.npz")
    if a.marginals_kde and not 1 <= a.marginals_kde_points <= 1024:
        ap.error("--marginals-kde-points is a number of grid points: 1 .. 1024")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    wcfg = BARTfunc.WorkerConfig.from_cfg(a.config_file)
    scfg = sampler.SamplerConfig.from_cfg(a.config_file)
    if a.numit:
        scfg.numit = a.numit
    leastsq = a.leastsq or scfg.leastsq
    unif = scfg.walk == "unif"
    if a.datasets:
        if not a.resident:
            ap.error("--datasets runs an ensemble in the resident loop: add --resident")
        if a.resume:
            ap.error("--datasets with --resume: an ensemble is not resumed from the command line.")
        if scfg.chisqscale:
            ap.error("--datasets with chisqscale: the uncertainties are not rescaled per group.")
        if leastsq:
            ap.error("--datasets with leastsq: the fit before the chain is not run per group.")
        if unif:
            ap.error("--datasets with walk = unif: a model grid has no data to vary.")
    if unif:
        for on, what in ((leastsq, "leastsq"), (scfg.chisqscale, "chisqscale"), (scfg.grexit, "grexit"),
                         (a.resume, "--resume")):
            if on:
                ap.error("walk = unif makes a model grid, not a chain: %s does not apply" % what)
        if not scfg.savemodel:
            ap.error("walk = unif keeps every model: name their file with `savemodel`")
        if a.python_loop or (world > 1 and not a.native_sharded):
            ap.error("walk = unif runs the native way: not with --python-loop, and on several ranks only with "
                     "--native-sharded")
    elif a.grid_bands or a.grid_f32:
        ap.error("--grid-bands and --grid-f32 go with walk = unif")
    if a.tp_envelopes and (unif or a.datasets):
        ap.error("--tp-envelopes is the envelope of one retrieval's chain: not with walk = unif or --datasets")
    if a.spectrum_envelopes and (unif or a.datasets):
        ap.error("--spectrum-envelopes is the envelope of one retrieval's chain: not with walk = unif or --datasets")
    if a.spectrum_envelopes and world > 1:
        ap.error("--spectrum-envelopes needs whole spectra on one GPU: not on several ranks (run "
                 "bart_amd.posterior.spectrum_envelopes on the written output.npy)")
    if a.marginals and (unif or a.datasets):
        ap.error("--marginals is the histograms of one retrieval's chain: not with walk = unif or --datasets")
    if a.marginals and not 1 <= a.marginals_bins <= 1024:
        ap.error("--marginals-bins is a number of bins: 1 .. 1024")
    if a.ess_exit and not a.ess_target > 0:
        ap.error("--ess-exit stops at a target: name it with --ess-target N")
    if a.ess_target < 0:
        ap.error("--ess-target is a number of effective samples: > 0")
    if a.ess_target > 0 and (not a.resident or a.datasets or unif):
        ap.error("--ess-target is served by the resident loop of one retrieval: add --resident (not with --datasets "
                 "or walk = unif)")
    if scfg.walk == "mrw" and not a.resident:
        ap.error("walk = mrw is served by the resident loop: add --resident")
    if scfg.chisqscale and not leastsq:
        ap.error("chisqscale = True scales the uncertainties by the least-squares optimum's chi-square: it comes with "
                 "leastsq = True (or --leastsq)")
    w = BARTfunc.Worker(wcfg, shard=(rank, world) if world > 1 else None, device=local)
    out = a.out or os.path.dirname(os.path.abspath(a.config_file))
    lines = []

    def log(msg):
        lines.append(msg)
        if rank == 0:
            print(msg, flush=True)

    t0 = time.perf_counter()
    native = not a.python_loop and (world == 1 or a.native_sharded)
    if native and world > 1:
        from . import engine
        engine.comm_init()
    if unif:
        res = model_grid(w, scfg, a, out, rank, log)
        if rank == 0:
            with open(os.path.join(out, "MCMC.log"), "w") as f:
                f.write("\n".join(lines) + "\n")
        w.close()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        return res
    if a.resident and not native:
        ap.error("--resident runs the native way: not with --python-loop, and on several ranks only with --native-sharded")
    if a.resume and not a.resident:
        ap.error("--resume continues a --resident run")
    if a.datasets:
        try:
            res = ensemble(w, scfg, a.datasets, out, rank, log, lines)
        finally:
            w.close()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        return res
    before = None
    if a.resume:
        if scfg.chisqscale:
            ap.error("--resume: chisqscale rescales the uncertainties from a fit this run does not repeat")
        try:
            before = load_state(out, scfg)
        except ValueError as err:
            w.close()
            ap.error(str(err))
        log("resuming after %d iterations" % int(before[1]["iterations"]))
        leastsq = False                      # (the chain continues from its own rows, not from an optimum)
    fitted = None
    if leastsq:
        if not native:
            ap.error("leastsq / chisqscale run the native way: not with --python-loop, and on several ranks only with "
                     "--native-sharded")
        fitted = least_squares(w, scfg, a.fit_starts, log)
    ess = dict(esstarget=a.ess_target, essexit=a.ess_exit)
    if a.resident and before is not None:
        res = sampler.run_resident(w, scfg, log=log, first=int(before[1]["iterations"]), start=before[0][:, -1], **ess)
    elif a.resident:
        res = sampler.run_resident(w, scfg, log=log, **ess)
    else:
        res = sampler.run_native(w, scfg, log=log) if native else sampler.run(w.step, scfg, log=log)
    dt = time.perf_counter() - t0
    nmodel = scfg.nchains * res.get("done", max(1, int(np.ceil(scfg.numit / scfg.nchains))))   # (a thinned chain holds fewer rows)
    log("%d models in %.2f s (%.0f models/s); acceptance %.3f; best chisq %.4f" % (
        nmodel, dt, nmodel / dt, res["accept_rate"], res["best_chisq"]))
    if res["grstat"] is not None:
        log("Gelman-Rubin: " + " ".join("%.3f" % g for g in res["grstat"]))
    log("Bad iterations due to temperature %d, abundance %d, energy %d" % (
        w.nbad[1], w.nbad[2], w.nbad[3]))
    state = None
    if a.resident:
        state = dict(state_of(scfg), iterations=res["done"], naccept=res["accepted"],
                     nbad=np.array([w.nbad[1], w.nbad[2], w.nbad[3]]), best_chisq=res["best_chisq"], bestp=res["bestp"])
    if before is not None:
        # the whole run: the rows, counts and best sample of both calls
        old = before[1]
        res["chain"] = np.concatenate([before[0], res["chain"]], axis=1)
        state.update(iterations=int(old["iterations"]) + res["done"], naccept=int(old["naccept"]) + res["accepted"],
                     nbad=old["nbad"] + state["nbad"])
        if float(old["best_chisq"]) <= res["best_chisq"]:
            res["best_chisq"], res["bestp"] = float(old["best_chisq"]), old["bestp"]
            state.update(best_chisq=res["best_chisq"], bestp=res["bestp"])
    if rank == 0:
        os.makedirs(out, exist_ok=True)
        np.save(os.path.join(out, "output.npy"), res["chain"])
        if state is not None:
            np.savez(os.path.join(out, "state.npz"), **state)
        with open(os.path.join(out, "bestFit.txt"), "w") as f:
            top = fitted if fitted is not None else res    # the optimum, not the chain's best sample
            f.write("# best-fit parameters, chisq = %.6f\n" % top["best_chisq"])
            f.write(" ".join("%.8g" % p for p in top["bestp"]) + "\n")
        if a.resident and native and scfg.savemodel:
            # MC3's layout of `savemodel`: [nchains, ndata, nkept]
            name = os.path.join(out, os.path.basename(scfg.savemodel))
            if not name.endswith(".npy"):
                name += ".npy"               # (the name np.save gives it)
            models = np.ascontiguousarray(res["models"].transpose(0, 2, 1))
            if before is not None and os.path.exists(name):
                models = np.concatenate([np.load(name), models], axis=2)
            np.save(name, models)
        with open(os.path.join(out, "MCMC.log"), "a" if before is not None else "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.tp_envelopes:
        # the whole chain's rows past the burn-in (after --resume: both calls'), on the engine the run used; the T(p)
        # model needs no spectrum, so every rank computes the same curves and rank 0 writes them
        from . import cf, posterior
        thin = max(1, int(scfg.thinning)) if a.resident else 1
        rows = min(int(scfg.burnin) // thin, res["chain"].shape[1] - 1)
        samples = cf.posterior_samples(res["chain"], scfg.params, scfg.stepsize, rows, layout="retrieve")
        env = dict(posterior.envelopes_of_samples(samples), burnin=rows)
        if rank == 0:
            posterior.save(os.path.join(out, "tp_envelopes.npz"), env)
        res["tp_envelopes"] = env
    if a.spectrum_envelopes:
        # the same rows on the engine the run used, and the run's best fit as the figure's curve and points
        from . import cf, posterior
        thin = max(1, int(scfg.thinning)) if a.resident else 1
        rows = min(int(scfg.burnin) // thin, res["chain"].shape[1] - 1)
        samples = cf.posterior_samples(res["chain"], scfg.params, scfg.stepsize, rows, layout="retrieve")
        top = fitted if fitted is not None else res
        senv = dict(posterior.spectrum_envelopes_of_worker(w, samples, best=top["bestp"], data=scfg.data,
                                                           uncert=scfg.uncert), burnin=rows)
        if rank == 0:
            posterior.save(os.path.join(out, "spectrum_envelopes.npz"), senv)
        res["spectrum_envelopes"] = senv
    if a.marginals:
        # the same rows; counted on this rank's GPU (no engine call: every rank gets the same integers, rank 0 writes)
        from . import cf, posterior
        thin = max(1, int(scfg.thinning)) if a.resident else 1
        rows = min(int(scfg.burnin) // thin, res["chain"].shape[1] - 1)
        samples = cf.posterior_samples(res["chain"], scfg.params, scfg.stepsize, rows, layout="retrieve")
        free = np.nonzero(np.asarray(scfg.stepsize) > 0)[0]
        marg = dict(posterior.marginals_of_samples(samples, free, a.marginals_bins, kde=a.marginals_kde,
                                                   kde_points=a.marginals_kde_points), burnin=rows)
        if rank == 0:
            posterior.save(os.path.join(out, a.marginals), marg)
        res["marginals"] = marg
    if fitted is not None:
        res["fit"] = fitted
    w.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return res


if __name__ == "__main__":
    main()
