"""Batched contribution functions / band transmittance (include/bartrt.h, bartrt_cf_batch_dev) on the
headline grid (100 layers x 1e4 wavenumbers, four table molecules, H2-H2 CIA, SURVEY.md 8d opacities),
ten filters, against the RT launch of the same batch under `toomuch 1e100` (every layer walked).

    python tools/cf_bench.py [walkers ...]        (default: 1 10 1000 10000)

One JSON line per batch size: milliseconds per call (wall clock between device synchronisations, the
median of several calls) of the contribution functions, the transmittance, and the RT launch
(run_batch_dev, same profiles), and their ratio."""
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


def main():
    batches = [int(a) for a in sys.argv[1:]] or [1, 10, 1000, 10000]
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
