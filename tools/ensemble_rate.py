"""Models per second of an ENSEMBLE of G independent ten-chain retrievals on one engine, two ways:

    grouped       one call of sampler.run_resident_groups: G groups in one resident loop, one model batch of 10 G rows
                  per iteration
    consecutive   G calls of sampler.run_resident one after the other (what an ensemble cost before), timed on the
                  library --parent-lib names -- a build of the commit before the grouped call -- or, without it, on
                  this build's unchanged single call

    python tools/ensemble_rate.py [--shapes headline,wasp] [--groups 1,2,4,6,8] [--iterations 400] [--repeat 3]
                                  [--inner 3] [--parent-lib bart_amd/libbartrt_parent.so] [--out FILE]

Every timing runs in a child process that builds the engine once per shape, warms both sizes up and then times each G
`inner` times.  The driver ALTERNATES the two kinds of child (consecutive, grouped, consecutive, ...) `repeat` times,
so that a drift of the machine falls on both alike, and reports per shape and G the median, the lowest and the highest
rate of each way and the ratio of the medians.  snooker, 400 iterations, Gelman-Rubin tests off in both (they cost the
same per group either way).  Shapes as tools/retrieval_rate.py: headline = 100 layers x 1e4 samples, 4 molecules,
10 filters, energy balance; wasp = the WASP-12b grid (2424 samples, 4 molecules, 4 filters)."""
import argparse
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="headline,wasp")
ap.add_argument("--groups", default="1,2,4,6,8")
ap.add_argument("--iterations", type=int, default=400)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--child", choices=("grouped", "consecutive"), default=None, help=argparse.SUPPRESS)
a = ap.parse_args()
groups = [int(g) for g in a.groups.split(",")]
NCH = 10


def child():
    import numpy as np
    from bart_amd import BARTfunc, sampler, synthcfg, transit_module as trm
    mols = ("H2O", "CO", "CO2", "CH4")
    truth = np.array([-1.5, -0.8, -0.8, 0.5, 1.0, -0.3, 0.2, -0.5, 0.1])
    pmin, pmax = np.array([-5, -2, -2, 0, 0.55, -9, -9, -9, -9.0]), np.array([-1, 1, 1, 1, 1.2, 1.5, 1.5, 1.5, 1.5])
    step = np.array([0.01, 0.01, 0.01, 0.01, 0.001, 0.05, 0.05, 0.05, 0.05])
    kws = {"headline": dict(nwave=10000, wnlow=1000.0, opmol=mols, molfit=mols, params=tuple(truth), nfilters=10,
                            ebalance=True),
           "wasp": dict(nwave=2424, wnlow=910.0, opmol=mols, molfit=mols, params=tuple(truth), nfilters=4)}
    build_id = trm.lib().bartrt_build_id().decode()
    for shape in a.shapes.split(","):
        d = os.path.join(tempfile.gettempdir(), "bartrt_retrate_" + shape)
        case, cfg = synthcfg.make_worker_case(d, reuse=True, **kws[shape])
        w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
        data = w.step(truth)[0]
        rng = np.random.default_rng(1)
        base = sampler.SamplerConfig(params=truth + 0.02, pmin=pmin, pmax=pmax, stepsize=step, data=data,
                                     uncert=data * 0.01, nchains=NCH, numit=a.iterations * NCH, burnin=50,
                                     walk="snooker", seed=1, grtest=False)
        # noise realisations of one spectrum, a seed each
        cfgs = [dataclasses.replace(base, data=data * (1.0 + 0.01 * rng.standard_normal(len(data))), seed=1 + g)
                for g in range(max(groups))]
        if a.child == "grouped":
            fn = lambda G: sampler.run_resident_groups(w, cfgs[:G])
        else:
            fn = lambda G: [sampler.run_resident(w, c) for c in cfgs[:G]]
        fn(1)
        fn(max(groups))                                # warm-up: every batch size's buffers and kernels
        for G in groups:
            fn(G)
            for _ in range(a.inner):
                t0 = time.perf_counter()
                fn(G)
                dt = time.perf_counter() - t0
                print("RATE " + json.dumps({"shape": shape, "way": a.child, "groups": G, "seconds": round(dt, 5),
                                            "models_per_s": round(G * NCH * a.iterations / dt, 1),
                                            "build_id": build_id}), flush=True)
        w.close()


def driver():
    rows = []
    args = [sys.executable, os.path.abspath(__file__), "--shapes", a.shapes, "--groups", a.groups, "--iterations",
            str(a.iterations), "--inner", str(a.inner)]
    for rep in range(a.repeat):
        for way in ("consecutive", "grouped"):
            env = dict(os.environ)
            if way == "consecutive" and a.parent_lib:
                env["BARTRT_LIBPATH"] = os.path.abspath(a.parent_lib)
            r = subprocess.run(args + ["--child", way], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("child %s failed (%d)\n%s\n%s" % (way, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
            for line in r.stdout.splitlines():
                if line.startswith("RATE "):
                    rows.append(dict(json.loads(line[5:]), repetition=rep))
                    print(json.dumps(rows[-1]), flush=True)
    where = "the parent build (%s)" % a.parent_lib if a.parent_lib else "this build's single call"
    lines = ["consecutive calls timed on " + where,
             "| shape | G | consecutive models/s: median (low - high) | grouped models/s: median (low - high) | ratio |",
             "|---|---|---|---|---|"]
    for shape in a.shapes.split(","):
        for G in groups:
            cell = {}
            for way in ("consecutive", "grouped"):
                v = [r["models_per_s"] for r in rows if (r["shape"], r["way"], r["groups"]) == (shape, way, G)]
                cell[way] = (statistics.median(v), min(v), max(v))
            lines.append("| %s | %d | %.0f (%.0f - %.0f) | %.0f (%.0f - %.0f) | %.2f |" % (
                shape, G, *cell["consecutive"], *cell["grouped"], cell["grouped"][0] / cell["consecutive"][0]))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n" + "\n".join(lines) + "\n")


if a.child:
    child()
else:
    driver()
