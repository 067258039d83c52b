#!/usr/bin/env python3
"""Times the percentile envelope of a synthetic posterior on the GPU against the host route.

    python tools/posterior_bench.py [--rows 200000 1000000] [--cols 100] [--reps 3]

The matrix [rows, cols] of doubles (temperature-like values) lies in HBM.  Device route: engine.percentiles_dev, the five
percentiles of bart_amd.posterior (ten order statistics in one selection call) and their interpolation.  Host route,
what the tree offered before: the same matrix copied to the host and passed to np.percentile / np.median, copy included.
Prints one JSON line per shape; the two results are compared (2 ulp of the larger neighbour).

    python tools/posterior_bench.py --spectrum [--samples 10000 100000] [--strides 1 4] [--reps 5]

The posterior spectrum envelope (bart_amd.posterior.spectrum_envelopes) on the demo eclipse configuration
(synthcfg.make_worker_case's defaults: 2501 samples, CH4, 10 filters), piece by piece, each timed by device events around
the call on the current stream, the median of --reps after a warm-up: per chunk of 4096 samples the step's launch
(engine.step_batch_dev with spectra) and the display kernel after it (engine.spectrum_display_dev, per stride), the
kernel's byte count 8 n W (1 + 1 / stride) over its time against the 8 TB/s the rooflines of this project use; per
sample count the two selection calls at the end (ten ranks over [n, Wk] and over [n, F]) and the whole
engine.posterior_spectrum call on the wall clock; and the host route this replaces on the smallest sample count: the
spectra copied back, spectrum / sflux * rprs**2, scipy's gaussian_filter1d and np.percentile."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


PEAK_HBM_GBS = 8000.0      # (tools/bench_configs.py)
CHUNK = 4096


def device_ms(fn, reps):
    """The median over reps of the device time of fn() between two events on the current stream, after a warm-up."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def spectrum_main(a):
    import tempfile
    import torch
    from scipy.ndimage import gaussian_filter1d
    from bart_amd import BARTfunc, engine, posterior, synthcfg, transit_module as trm
    q = list(posterior.LEVELS.values())
    half = posterior.gauss_half(2.0)
    pmin = np.array([-2.6, -0.6, 0.5, 0.0, 0.80, -2.0])      # (a box without rejected rows around BART_eclipse.cfg:80)
    pmax = np.array([-1.6, 0.6, 1.2, 1.0, 1.20, 1.0])
    with tempfile.TemporaryDirectory() as d:
        case, cfg = synthcfg.make_worker_case(d)
        w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg), carry=False)
        try:
            W, F = w.nwave, w.nfilters
            sflux = posterior.stellar_flux(w)
            d_sflux = torch.from_numpy(sflux).cuda()
            rng = np.random.default_rng(1)
            draw = lambda n: np.ascontiguousarray(pmin + (pmax - pmin) * rng.random((n, pmin.size)))
            d_par = torch.from_numpy(draw(CHUNK)).cuda()
            out = {"build_id": trm.lib().bartrt_build_id().decode(), "nwave": W, "nfilters": F, "chunk": CHUNK,
                   "radius": int(half.size - 1), "reps": a.reps}
            band, st, spec = engine.step_batch_dev(d_par, F, want_spec=True)
            torch.cuda.synchronize()
            out["chunk_accepted"] = int((st == 0).sum().item())
            out["step_batch_ms"] = device_ms(lambda: engine.step_batch_dev(d_par, F, want_spec=True), a.reps)
            for s in a.strides:
                ms = device_ms(lambda: engine.spectrum_display_dev(spec, half, d_sflux, w.rprs, s), a.reps)
                nbytes = 8.0 * CHUNK * W * (1.0 + 1.0 / s)
                out["display_ms_stride%d" % s] = ms
                out["display_share_of_step_stride%d" % s] = ms[0] / out["step_batch_ms"][0]
                out["display_gbs_stride%d" % s] = nbytes / (1e-3 * ms[0]) / 1e9
                out["display_frac_of_hbm_stride%d" % s] = nbytes / (1e-3 * ms[0]) / 1e9 / PEAK_HBM_GBS
            print(json.dumps(out), flush=True)
            disp = engine.spectrum_display_dev(spec, half, d_sflux, w.rprs, 1)
            for n in a.samples:
                # the matrices a posterior of n samples leaves: the chunk's rows repeated, jittered so that no two are equal
                g = torch.Generator(device="cuda").manual_seed(n)
                idx = torch.arange(n, device="cuda") % CHUNK
                jit = 1.0 + 1e-3 * torch.rand((n, 1), dtype=torch.float64, device="cuda", generator=g)
                M, B = disp[idx] * jit, band[idx] * jit
                lohi = [engine.percentile_rule(n, v) for v in q]
                ranks = np.array([k for lo, hi, _ in lohi for k in (lo, hi)], np.int64)
                row = {"samples": n, "matrix_bytes": int(n) * W * 8,
                       "colselect_spec_ms": device_ms(lambda: engine.colselect(M, ranks), a.reps),
                       "colselect_band_ms": device_ms(lambda: engine.colselect(B, ranks), a.reps)}
                del M, B
                params = draw(n)
                engine.posterior_spectrum(params[:CHUNK], q, sflux, half, 1)
                ts = []
                for _ in range(max(1, a.reps // 2)):
                    t0 = time.perf_counter()
                    env = engine.posterior_spectrum(params, q, sflux, half, 1)
                    ts.append(1e3 * (time.perf_counter() - t0))
                row["posterior_spectrum_wall_ms"] = [float(np.median(ts)), float(min(ts)), float(max(ts))]
                row["ngood"] = int(env[3])
                if n == min(a.samples):
                    # the host route: every chunk's spectra copied back, the display quantity and the percentiles in numpy
                    t0 = time.perf_counter()
                    rows = []
                    for off in range(0, n, CHUNK):
                        _, _, sp = engine.step_batch_dev(torch.from_numpy(params[off:off + CHUNK]).cuda(), F, want_spec=True)
                        rows.append(sp.cpu().numpy())
                    t1 = time.perf_counter()
                    y = gaussian_filter1d(np.concatenate(rows) / sflux * w.rprs * w.rprs, 2, axis=1)
                    t2 = time.perf_counter()
                    want = np.percentile(y, q, axis=0)
                    t3 = time.perf_counter()
                    row.update(host_total_ms=1e3 * (t3 - t0), host_step_and_copy_ms=1e3 * (t1 - t0),
                               host_filter_ms=1e3 * (t2 - t1), host_percentile_ms=1e3 * (t3 - t2),
                               worst_rel_diff=float(np.max(np.abs(env[0] - want) / np.abs(want))))
                print(json.dumps(row), flush=True)
        finally:
            w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectrum", action="store_true", help="time the posterior spectrum envelope's pieces instead")
    ap.add_argument("--samples", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--strides", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rows", type=int, nargs="+", default=[200000, 1000000])
    ap.add_argument("--cols", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.spectrum:
        return spectrum_main(a)
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
