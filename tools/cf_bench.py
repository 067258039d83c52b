"""Batched contribution functions / band transmittance (include/bartrt.h, bartrt_cf_batch_dev) on the
headline grid (100 layers x 1e4 wavenumbers, four table molecules, H2-H2 CIA, SURVEY.md 8d opacities),
ten filters, against the RT launch of the same batch under `toomuch 1e100` (every layer walked).

    python tools/cf_bench.py [walkers ...]        (default: 1 10 1000 10000)
    python tools/cf_bench.py --posterior [n]      (default: 1000 samples)

One JSON line per batch size: milliseconds per call (wall clock between device synchronisations, the
median of several calls) of the contribution functions, the transmittance, and the RT launch
(run_batch_dev, same profiles), and their ratio.

--posterior: n posterior samples, each with its own radius and cloud top, three ways in one session, interleaved
(one round = one call of each form; the median over the rounds and the rounds' spread per form):
  (a) batched_over   bartrt_cf_batch_over, one call for all samples;
  (b) host_loop      what there was before it: bartrt_set_radius / bartrt_set_cloudtop and bartrt_cf_batch on one
                     profile, per sample;
  (c) batched_wide   bartrt_cf_batch on the same profiles under one engine-wide radius and cloud top (the median of
                     the samples' own, so the layers walked agree on average): the floor -- (a) moves 24 bytes per
                     walker more;
and the device forms of (a) and (c) on resident tensors."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from bart_amd import cf, engine, synth, transit_module as trm  # noqa: E402


def filters(d, wn, n=10):
    """n filters of 300-1500 samples spread over the grid, two of them overlapping their neighbour."""
    rng = np.random.default_rng(5)
    out = []
    centres = np.linspace(wn[0] + 600, wn[-1] - 600, n)
    for j, c in enumerate(centres):
        half = rng.uniform(150, 750) * (2.0 if j in (3, 7) else 1.0)
        wl = np.linspace(1e4 / (c + half), 1e4 / (c - half), 60)
        p = os.path.join(d, "bench_f%02d.dat" % j)
        synth.write_filter(p, wl, np.sin(np.linspace(0, np.pi, wl.size)) ** 2)
        out.append(p)
    return out


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def posterior_leg(case, win, n, rounds=9):
    """The three forms on n samples (module docstring): one JSON line."""
    nf = engine.cf_setup(win)
    L = engine.nlayers()
    rng = np.random.default_rng(3)
    base = bench.make_profiles(case, 64, seed=11)
    prof = np.ascontiguousarray(base[np.arange(n) % len(base)])
    r0 = float(case.keys["refradius"])
    over = np.column_stack([r0 * rng.uniform(0.95, 1.05, n), rng.uniform(0.0, 1.0, n), np.full(n, np.nan)])
    wide = (float(np.median(over[:, 0])), float(np.median(over[:, 1])))
    band = np.zeros((n, nf, L))
    one = np.zeros((1, nf, L))
    lib, ptr = trm.lib(), trm._ptr
    d_prof, d_over = torch.from_numpy(prof).cuda(), torch.from_numpy(over).cuda()

    def batched_over():
        trm.check(lib.bartrt_cf_batch_over(ptr(prof), n, prof.shape[1], ptr(over), engine.CF_CONTRIB, ptr(band), None, None))

    def host_loop():
        for w in range(n):
            trm.set_radius(over[w, 0])
            trm.set_cloudtop(over[w, 1])
            trm.check(lib.bartrt_cf_batch(ptr(prof[w:w + 1]), 1, prof.shape[1], engine.CF_CONTRIB, ptr(one), None, None))

    def set_wide():
        trm.set_radius(wide[0])
        trm.set_cloudtop(wide[1])

    def batched_wide():
        trm.check(lib.bartrt_cf_batch(ptr(prof), n, prof.shape[1], engine.CF_CONTRIB, ptr(band), None, None))

    forms = {"batched_over": batched_over, "host_loop": host_loop, "batched_wide": batched_wide,
             "batched_over_dev": lambda: engine.contribution_dev(d_prof, over=d_over),
             "batched_wide_dev": lambda: engine.contribution_dev(d_prof)}
    times = {k: [] for k in forms}
    for r in range(rounds + 1):              # round 0 warms every form up
        for k, fn in forms.items():
            if k.startswith("batched_wide"):
                set_wide()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[k].append(1e3 * (time.perf_counter() - t0))
    out = {"workload": "posterior cf, 100 layers x 1e4 wavenumbers, %d filters, per-sample radius and cloud top" % nf,
           "samples": n, "rounds": rounds, "build_id": trm.lib().bartrt_build_id().decode()}
    for k, t in times.items():
        out[k + "_ms"] = round(float(np.median(t)), 3)
        out[k + "_spread_ms"] = [round(float(np.min(t)), 3), round(float(np.max(t)), 3)]
    out["over_vs_wide"] = round(out["batched_over_ms"] / out["batched_wide_ms"], 4)
    out["loop_vs_over"] = round(out["host_loop_ms"] / out["batched_over_ms"], 2)
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    posterior = "--posterior" in args
    if posterior:
        args.remove("--posterior")
    batches = [int(a) for a in args] or ([1000] if posterior else [1, 10, 1000, 10000])
    d = os.path.join(tempfile.gettempdir(), "bartrt_cfbench")
    case = synth.make_case(d, nlayers=100, nwave=10000, kappa_model="survey8d", reuse=True)
    keys = dict(case.keys)
    keys["toomuch"] = "1e100"
    cfg = os.path.join(d, "cf_tconfig.cfg")
    synth.write_tcfg(cfg, keys)
    files = filters(d, case.wn)
    win = cf.filter_windows(case.wn, files)
    engine.init(cfg)
    try:
        if posterior:
            for n in batches:
                posterior_leg(case, win, n)
            return
        nf = engine.cf_setup(win)
        base = bench.make_profiles(case, 64, seed=11)
        for n in batches:
            d_prof = torch.from_numpy(base[np.arange(n) % len(base)]).cuda().contiguous()
            spec = torch.empty((n, 10000), dtype=torch.float64, device="cuda")
            reps = 20 if n <= 10 else 5
            t_cf = timed(lambda: engine.contribution_dev(d_prof), reps)
            t_tr = timed(lambda: engine.transmittance_dev(d_prof), reps)
            t_rt = timed(lambda: engine.run_batch_dev(d_prof, spec), reps)
            print(json.dumps({"workload": "cf_batch, 100 layers x 1e4 wavenumbers, %d filters" % nf, "walkers": n,
                              "cf_ms": round(t_cf, 4), "transmit_ms": round(t_tr, 4),
                              "rt_toomuch_1e100_ms": round(t_rt, 4), "cf_over_rt": round(t_cf / t_rt, 3),
                              "build_id": trm.lib().bartrt_build_id().decode()}), flush=True)
    finally:
        trm.free_memory()


if __name__ == "__main__":
    main()
