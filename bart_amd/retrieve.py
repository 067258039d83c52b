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
    ap.add_argument("--leastsq", action="store_true",
                    help="run the multi-start least-squares fit before the chain (fit.fit), as `leastsq = True` in "
                         "the configuration does")
    ap.add_argument("--fit-starts", type=int, default=None, help="starts of that fit (default: nchains)")
    a = ap.parse_args(argv)
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
    if a.resident and not native:
        ap.error("--resident runs the native way: not with --python-loop, and on several ranks only with --native-sharded")
    fitted = None
    if leastsq:
        if not native:
            ap.error("leastsq / chisqscale run the native way: not with --python-loop, and on several ranks only with "
                     "--native-sharded")
        fitted = least_squares(w, scfg, a.fit_starts, log)
    if a.resident:
        res = sampler.run_resident(w, scfg, log=log)
    else:
        res = sampler.run_native(w, scfg, log=log) if native else sampler.run(w.step, scfg, log=log)
    dt = time.perf_counter() - t0
    nmodel = scfg.nchains * max(1, int(np.ceil(scfg.numit / scfg.nchains)))   # (a thinned chain holds fewer rows)
    log("%d models in %.2f s (%.0f models/s); acceptance %.3f; best chisq %.4f" % (
        nmodel, dt, nmodel / dt, res["accept_rate"], res["best_chisq"]))
    if res["grstat"] is not None:
        log("Gelman-Rubin: " + " ".join("%.3f" % g for g in res["grstat"]))
    log("Bad iterations due to temperature %d, abundance %d, energy %d" % (
        w.nbad[1], w.nbad[2], w.nbad[3]))
    if rank == 0:
        os.makedirs(out, exist_ok=True)
        np.save(os.path.join(out, "output.npy"), res["chain"])
        with open(os.path.join(out, "bestFit.txt"), "w") as f:
            top = fitted if fitted is not None else res    # the optimum, not the chain's best sample
            f.write("# best-fit parameters, chisq = %.6f\n" % top["best_chisq"])
            f.write(" ".join("%.8g" % p for p in top["bestp"]) + "\n")
        if a.resident and native and scfg.savemodel:
            # MC3's layout of `savemodel`: [nchains, ndata, nkept]
            np.save(os.path.join(out, os.path.basename(scfg.savemodel)),
                    np.ascontiguousarray(res["models"].transpose(0, 2, 1)))
        with open(os.path.join(out, "MCMC.log"), "w") as f:
            f.write("\n".join(lines) + "\n")
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
