#!/usr/bin/env python3
"""Times the posterior marginals on the GPU against the host loop they replace.

    python tools/marginals_bench.py [--rows 1000000 10000000] [--cols 9] [--bins 20] [--reps 3] [--no-numpy] [--slab N]

A synthetic posterior [rows, cols] of doubles, every column free.  The host loop is what MC3's `histogram` and `pairwise`
do: np.histogram per parameter and np.histogram2d per pair, with numpy's default ranges.  Timed against it, each with a
device synchronise inside the window:

    engine, host form      engine.marginals_range + engine.marginals on the numpy array (upload in chunks included)
    engine, device form    the same two calls on a CUDA tensor already in HBM, results copied back
    posterior, host/device posterior.marginals_of_samples (range, edges, counts, HPD regions)
    bin only / with pairs  engine.marginals on the CUDA tensor without and with pairs: the first is the binning kernel
                           alone, the difference the pair kernel and the bin indices written for it

Every count is compared with numpy's (equality).  Prints one JSON line.  --no-numpy leaves the host loop out (for a run
under a profiler)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def best(f, reps, sync):
    out = None
    times = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        out = f()
        sync()
        times.append(time.perf_counter() - t0)
    return round(1e3 * min(times), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--slab", type=int, default=0, help="rows per workgroup (0: the library's default)")
    a = ap.parse_args()
    import torch
    from bart_amd import engine, posterior, transit_module as trm
    sync = torch.cuda.synchronize
    engine.marginals_set_slab(a.slab)
    cols = np.arange(a.cols)
    shapes = []
    for n in a.rows:
        rng = np.random.default_rng(n)
        x = rng.normal(size=(n, a.cols)) * 10.0 ** rng.integers(-2, 3, a.cols) + rng.normal(size=a.cols)
        d_x = torch.from_numpy(x).cuda()

        def engine_form(m):
            lohi, _ = engine.marginals_range(m, cols)
            lohi = lohi if isinstance(lohi, np.ndarray) else lohi.cpu().numpy()
            edges = np.stack([np.linspace(lo, hi, a.bins + 1) for lo, hi in lohi])
            h1, out, h2 = engine.marginals(m, cols, edges)
            return (h1, h2) if isinstance(h1, np.ndarray) else (h1.cpu().numpy(), h2.cpu().numpy())

        engine_form(x), engine_form(d_x)           # (buffers grown, kernels loaded)
        row = {"rows": n, "cols": a.cols, "bins": a.bins, "pairs": a.cols * (a.cols - 1) // 2}
        row["engine_host_ms"], (h1, h2) = best(lambda: engine_form(x), a.reps, sync)
        row["engine_device_ms"], (d1, d2) = best(lambda: engine_form(d_x), a.reps, sync)
        row["posterior_host_ms"], m = best(lambda: posterior.marginals_of_samples(x, cols, a.bins), a.reps, sync)
        row["posterior_device_ms"], _ = best(lambda: posterior.marginals_of_samples(d_x, cols, a.bins), a.reps, sync)
        edges = m["edges"]
        row["bin_only_ms"], _ = best(lambda: engine.marginals(d_x, cols, edges, pairs=False), a.reps, sync)
        row["bin_and_pairs_ms"], _ = best(lambda: engine.marginals(d_x, cols, edges, pairs=True), a.reps, sync)
        row["pairs_ms"] = round(row["bin_and_pairs_ms"] - row["bin_only_ms"], 3)
        same = np.array_equal(h1, d1) and np.array_equal(h2, d2) and np.array_equal(m["hist"], h1.astype(np.int64))
        if not a.no_numpy:
            def numpy_loop():
                w1 = [np.histogram(x[:, c], bins=a.bins)[0] for c in cols]
                w2 = [np.histogram2d(x[:, i], x[:, j], bins=a.bins)[0] for i in cols for j in cols[i + 1:]]
                return np.array(w1), np.array(w2)
            row["numpy_ms"], (w1, w2) = best(numpy_loop, 1 if n > 2000000 else a.reps, sync)
            same = same and np.array_equal(h1, w1.astype(np.uint64)) and np.array_equal(h2, w2.astype(np.uint64))
            row["speedup_host_form"] = round(row["numpy_ms"] / row["engine_host_ms"], 2)
            row["speedup_device_form"] = round(row["numpy_ms"] / row["engine_device_ms"], 2)
        row["equal"] = bool(same)
        shapes.append(row)
        del d_x
    print(json.dumps({"build_id": trm.lib().bartrt_build_id().decode(), "slab": engine.marginals_slab(), "shapes": shapes}), flush=True)


if __name__ == "__main__":
    main()
