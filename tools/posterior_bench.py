#!/usr/bin/env python3
"""Times the percentile envelope of a synthetic posterior on the GPU against the host route.

    python tools/posterior_bench.py [--rows 200000 1000000] [--cols 100] [--reps 3]

The matrix [rows, cols] of doubles (temperature-like values) lies in HBM.  Device route: engine.percentiles_dev, the five
percentiles of bart_amd.posterior (ten order statistics in one selection call) and their interpolation.  Host route,
what the tree offered before: the same matrix copied to the host and passed to np.percentile / np.median, copy included.
Prints one JSON line per shape; the two results are compared (2 ulp of the larger neighbour)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[200000, 1000000])
    ap.add_argument("--cols", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import tempfile
    import torch
    from bart_amd import engine, synth, transit_module as trm
    from bart_amd.posterior import LEVELS
    q = list(LEVELS.values())
    with tempfile.TemporaryDirectory() as d:
        case = synth.make_case(d, nlayers=20, nwave=64)       # (any engine: the selection needs its stream and scratch)
        engine.init(case.tcfg)
        try:
            for n in a.rows:
                g = torch.Generator(device="cuda").manual_seed(n)
                x = 1500.0 + 300.0 * torch.randn((n, a.cols), dtype=torch.float64, device="cuda", generator=g)
                engine.percentiles_dev(x, q)                   # (buffers grown, kernels loaded)
                torch.cuda.synchronize()
                dev, host = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    vals, _, _ = engine.percentiles_dev(x, q)
                    dev.append(time.perf_counter() - t0)
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    h = x.cpu().numpy()
                    t1 = time.perf_counter()
                    want = np.percentile(h, q, axis=0)
                    host.append((time.perf_counter() - t0, t1 - t0))
                spacing = np.spacing(np.abs(want))
                print(json.dumps({"rows": n, "cols": a.cols, "percentiles": len(q),
                                  "device_ms": round(1e3 * min(dev), 3),
                                  "host_ms": round(1e3 * min(h[0] for h in host), 1),
                                  "host_copy_ms": round(1e3 * min(h[1] for h in host), 1),
                                  "worst_ulp": float(np.max(np.abs(vals - want) / spacing))}), flush=True)
                del x
        finally:
            trm.free_memory()


if __name__ == "__main__":
    main()
