#!/usr/bin/env python3
"""Times the posterior kernel density estimates on the GPU against the host loop they replace.

    python tools/kde_bench.py [--rows 1000000 10000000] [--cols 9] [--points 128] [--reps 3] [--no-scipy]

A synthetic posterior [rows, cols] of doubles, every column free, each column's grid np.linspace over its range.  The
host loop is scipy.stats.gaussian_kde(col, 'scott')(grid) per parameter, on one core.  Timed against it, each with a
device synchronise inside the window:

    engine, host form        engine.kde on the numpy array (two uploads in chunks included)
    engine, device form      engine.kde on a CUDA tensor already in HBM, results copied back
    posterior without / with kde    posterior.marginals_of_samples on the CUDA tensor and on the numpy array: the first is
                             what `retrieve --marginals` cost before, the second what --marginals-kde adds to it

scipy is timed on every column up to 2e6 rows and on `--scipy-cols` columns (default 1) above, where the figure for all
columns is that time scaled by cols / scipy-cols and is marked as scaled.  The densities are compared with scipy's on
the columns it ran (largest absolute difference over the largest density).  Prints one JSON line."""
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
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--scipy-cols", type=int, default=1, help="columns scipy is timed on above 2e6 rows")
    a = ap.parse_args()
    import torch
    from bart_amd import engine, posterior, transit_module as trm
    sync = torch.cuda.synchronize
    cols = np.arange(a.cols)
    shapes = []
    for n in a.rows:
        rng = np.random.default_rng(n)
        x = rng.normal(size=(n, a.cols)) * 10.0 ** rng.integers(-2, 3, a.cols) + rng.normal(size=a.cols)
        grid = np.stack([np.linspace(x[:, c].min(), x[:, c].max(), a.points) for c in cols])
        d_x = torch.from_numpy(x).cuda()

        def engine_form(m):
            pdf, stat, _ = engine.kde(m, cols, grid, "scott")
            return (pdf, stat) if isinstance(pdf, np.ndarray) else (pdf.cpu().numpy(), stat.cpu().numpy())

        engine_form(x), engine_form(d_x)           # (buffers grown, kernels loaded)
        posterior.marginals_of_samples(d_x, cols, kde=True, kde_points=a.points)
        row = {"rows": n, "cols": a.cols, "points": a.points, "exponentials": n * a.cols * a.points}
        row["engine_host_ms"], (pdf, stat) = best(lambda: engine_form(x), a.reps, sync)
        row["engine_device_ms"], (d_pdf, d_stat) = best(lambda: engine_form(d_x), a.reps, sync)
        row["exponentials_per_s_device_form"] = round(row["exponentials"] / (1e-3 * row["engine_device_ms"]), -6)
        for name, m in (("device", d_x), ("host", x)):
            row["posterior_%s_ms" % name], _ = best(lambda: posterior.marginals_of_samples(m, cols), a.reps, sync)
            row["posterior_%s_kde_ms" % name], _ = best(
                lambda: posterior.marginals_of_samples(m, cols, kde=True, kde_points=a.points), a.reps, sync)
        row["same_bits_host_and_device_form"] = bool(pdf.tobytes() == d_pdf.tobytes() and stat.tobytes() == d_stat.tobytes())
        if not a.no_scipy:
            from scipy.stats import gaussian_kde
            timed = a.cols if n <= 2000000 else min(a.cols, max(1, a.scipy_cols))
            t0 = time.perf_counter()
            want = np.stack([gaussian_kde(x[:, c], bw_method="scott")(grid[c]) for c in cols[:timed]])
            row["scipy_cols_timed"] = timed
            row["scipy_ms"] = round(1e3 * (time.perf_counter() - t0) * a.cols / timed, 1)
            row["scipy_ms_is_scaled"] = timed != a.cols
            row["max_diff_over_max_pdf"] = float(np.max(np.abs(pdf[:timed] - want) / want.max(axis=1, keepdims=True)))
            row["speedup_host_form"] = round(row["scipy_ms"] / row["engine_host_ms"], 1)
            row["speedup_device_form"] = round(row["scipy_ms"] / row["engine_device_ms"], 1)
        shapes.append(row)
        del d_x
    print(json.dumps({"build_id": trm.lib().bartrt_build_id().decode(), "tile": engine.kde_tile(), "shapes": shapes}),
          flush=True)


if __name__ == "__main__":
    main()
