"""`python bench.py --gpus N` must launch itself: with N > 1
and no RANK in the environment the script starts torch.distributed.run on itself
as a child process, the ranks run the sharded step loop, and exactly ONE JSON
line comes back on stdout.  Run here with --dry-gloo: a stub engine on CPU
tensors over gloo, whose reassembled spectra are checked sample for sample
inside bench.py; the GPU engine takes the same code path with nccl."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=e,
                          capture_output=True, text=True, timeout=600)


def test_gpus2_self_launch_one_json_line():
    r = _bench("--gpus", "2", "--full", "--dry-gloo", "--steps", "11", "--warmup", "3", "--walkers", "3",
               "--nwave", "2501", "--gather-steps", "4", "--sweep", "")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout            # the contract: ONE line on stdout
    j = json.loads(lines[0])
    assert j["dry"] is True and j["value"] is None      # a dry run is never a measurement
    assert j["n_gpus"] == 2 and j["steps"] == 11 and j["warmup"] == 3
    assert j["scaling"] == "weak" and j["config"]["walkers_per_step"] == 6   # walkers scale with N
    assert j["ms_per_step"] > 0
    # the N > 1 line explains itself: per-rank window and kernel times, the
    # bucket's bytes, the final drain, the skew between the ranks
    d = j["scaling_diag"]
    assert d["mode"] == "shard" and len(d["per_rank_window_s"]) == 2 and len(d["per_rank_rt_kernel_ms"]) == 2
    assert d["steps_per_bucket"] == 4 and d["rank_skew_ms"] >= 0 and len(d["per_rank_final_drain_ms"]) == 2
    wmax = 2501 - 2501 // 2
    assert d["allgather_send_bytes_per_rank_per_bucket"] == 4 * 6 * wmax * 8
    assert d["allgather_recv_bytes_per_rank_per_bucket"] == 2 * 4 * 6 * wmax * 8


def test_gpus8_uneven_grid_dry_run():
    """A node's worth of ranks on a grid that does not divide (2 501 samples over 8): the blocks' padding in the
    bucketed all-gather, the reassembly checked sample for sample inside bench.py, and the keys the first real
    8-GPU record will be read by (what an N = 8 line should look like)."""
    r = _bench("--gpus", "8", "--full", "--dry-gloo", "--steps", "9", "--warmup", "2", "--walkers", "2",
               "--nwave", "2501", "--gather-steps", "4", "--sweep", "")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 8 and j["config"]["walkers_per_step"] == 16 and j["scaling"] == "weak"
    d = j["scaling_diag"]
    for key in ("mode", "per_rank_window_s", "rank_skew_ms", "per_rank_rt_kernel_ms", "per_rank_final_drain_ms",
                "steps_per_bucket", "allgather_send_bytes_per_rank_per_bucket",
                "allgather_recv_bytes_per_rank_per_bucket", "ms_per_step_minus_rt_kernel"):
        assert key in d, key
    assert len(d["per_rank_window_s"]) == 8 and len(d["per_rank_final_drain_ms"]) == 8
    wmax = max(2501 * (k + 1) // 8 - 2501 * k // 8 for k in range(8))
    assert wmax == 313 and d["allgather_send_bytes_per_rank_per_bucket"] == 4 * 16 * wmax * 8


def test_gpus2_replicas_mode_has_no_collective():
    """--mode replicas: SURVEY 8e's baseline -- every rank the whole grid and its own walkers."""
    r = _bench("--gpus", "2", "--full", "--dry-gloo", "--mode", "replicas", "--steps", "5", "--warmup", "1", "--walkers", "3",
               "--nwave", "700", "--sweep", "")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["config"]["walkers_per_step"] == 6
    assert "replicas x2" in j["config"]["parallelism"]
    assert j["scaling_diag"]["mode"] == "replicas" and "steps_per_bucket" not in j["scaling_diag"]


def test_child_failure_becomes_the_exit_code():
    # an impossible shard (more ranks than samples) fails in the ranks; the
    # launcher must pass the failure on, not print a line
    r = _bench("--gpus", "2", "--dry-gloo", "--steps", "1", "--warmup", "0", "--walkers", "1",
               "--nwave", "1", "--sweep", "")
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_single_rank_needs_no_launcher():
    r = _bench("--dry-gloo", "--steps", "3", "--warmup", "1", "--walkers", "2", "--nwave", "700", "--sweep", "")
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(r.stdout.strip())
    assert j["n_gpus"] == 1 and j["dry"] is True


def test_launch_byte_model_counts_shared_rows_once(tmp_path):
    """bench.py's per-launch byte model: identical walkers share every
    row (unique bytes of one walker + the per-walker records and spectra), walkers in
    disjoint temperature brackets share none, and a launch that stops half way down
    moves half the table bytes; the effective bytes follow SURVEY 8d's per-spectrum
    figure restricted to the walked layers."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from bart_amd import synth
    L, W, nw = 40, 640, 4
    case = synth.make_case(str(tmp_path), nlayers=L, nwave=W)          # 4 molecules, H2-H2 CIA, 27 planes
    prof = case.profiles(temp=np.full(L, 1010.0)).ravel()
    same = np.tile(prof, (nw, 1))
    walked = np.full((nw, W // 64), L, np.int32)
    m = bench.launch_byte_model(case, same, walked, 64, W)
    table = 2 * L * 4 * W * 8                     # two planes, four molecules
    cia = 2 * W * 8                               # one pair of CIA planes, shared by every layer
    fixed = nw * L * (4 + 2 * 4 + 2 + 2) * 8 + nw * W * 8 + W * 8
    assert m["unique_bytes"] == table + cia + fixed and m["layers_walked_frac"] == 1.0
    assert m["effective_bytes"] == nw * (2 * L * W * 4 * 8 + 2 * L * W * 8) + fixed
    apart = np.array([case.profiles(temp=np.full(L, t)).ravel() for t in (450.0, 1010.0, 1650.0, 2950.0)])
    m2 = bench.launch_byte_model(case, apart, walked, 64, W)
    assert m2["unique_bytes"] - fixed == nw * table + 4 * cia          # nothing shared (CIA grid: 200 K steps)
    half = bench.launch_byte_model(case, same, walked // 2, 64, W)
    assert half["unique_bytes"] - fixed == table // 2 + cia and half["layers_walked_frac"] == 0.5


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "parity", "detail")
ROOFLINE_KEYS = ("bound", "achieved", "peak", "unit", "frac", "frac_cold", "frac_survey8d_letter", "traffic",
                 "traffic_source", "kernel", "avg_launch_ms", "unique_bytes_per_launch", "launches")


def _full_size_result(n_gpus):
    """A result as large as any run has produced: round 5's 20 kB record (profiles/r05_bench.json -- every side leg,
    every note) with the profiler-derived fields filled in and, for N > 1, per-rank diagnostics and a replicas leg."""
    res = json.load(open(os.path.join(ROOT, "profiles", "r05_bench.json")))
    res["n_gpus"] = n_gpus
    res["roofline"].update(traffic=353.1e6, traffic_source="profiles/r06_w10_pmc.json",
                           bound_measured={"source": "profiles/r06_w10_sq.json",
                                           "10": {"bound": "issue/latency", "fp64_pipe_busy_fraction": 0.51,
                                                  "resident_waves_per_simd": 1.5, "wave_time": {"busy": 0.5}},
                                           "256": {"bound": "fp64_valu", "fp64_pipe_busy_fraction": 0.83,
                                                   "resident_waves_per_simd": 4, "wave_time": {"busy": 0.8}}},
                           fp64={"frac": 0.31234567, "note": "x" * 400})
    if n_gpus > 1:
        per_rank = [0.0123456789 + 1e-4 * r for r in range(n_gpus)]
        res["scaling_diag"] = {"mode": "shard", "per_rank_window_s": per_rank, "rank_skew_ms": 0.7,
                               "per_rank_rt_kernel_ms": per_rank, "per_rank_final_drain_ms": per_rank,
                               "exposed_gather_note": "y" * 300, "steps_per_bucket": 4,
                               "allgather_send_bytes_per_rank_per_bucket": 4 * 80 * 1250 * 8,
                               "allgather_recv_bytes_per_rank_per_bucket": 8 * 4 * 80 * 1250 * 8,
                               "ms_per_step_minus_rt_kernel": 0.031}
        res["replicas"] = {"value": 7.1e5, "unit": "spectra/s", "ms_per_step": 0.11, "walkers_per_rank": 10,
                           "note": "z" * 300, "diag": dict(res["scaling_diag"])}
        res["config"]["parallelism"] = "wavenumber-block shard x%d + all-gather" % n_gpus
    return res


def test_contract_line_is_short_and_complete():
    """the last stdout line is the contract's line and nothing else -- at most 4 kB whatever the
    run produced (the driver keeps 8 kB of stdout: round 5's 20 kB line did not parse), valid JSON, every key the
    judge reads; the rest goes to the detail file."""
    sys.path.insert(0, ROOT)
    import bench
    for n in (1, 8, 64):
        res = _full_size_result(n)
        assert len(json.dumps(res)) > 15000                      # the input really is the large record
        text = bench.contract_line(res)
        assert "\n" not in text and len(text) <= 4096, len(text)
        j = json.loads(text)
        for k in CONTRACT_KEYS:
            assert k in j, k
        for k in ROOFLINE_KEYS:
            assert k in j["roofline"], k
        assert j["roofline"]["traffic"] == 353.1e6 and j["roofline"]["bound_measured"]["256"] == "fp64_valu"
        assert set(j["config"]) >= {"workload", "walkers_per_step", "nlayers", "nwave", "integ", "cut", "cia_interp"}
        assert len(j["config"]["workload"]) <= 300
        assert set(j["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"}
        assert set(j["parity"]) >= {"max_rel_err", "n_samples", "bit_equal_to_plain_launch", "ok"}
        assert j["value"] == float("%.6g" % res["value"]) and j["n_gpus"] == n
        for leg in ("configs", "batch_sweep", "integ_sweep", "cut_sweep", "forest_workload", "with_prefetch"):
            assert leg not in j                                  # side legs live in the detail file
        if n > 1:
            assert j["scaling_diag"]["mode"] == "shard" and j["replicas"]["value"] == 7.1e5
            assert "exposed_gather_note" not in j["scaling_diag"]
        if n == 8:
            assert len(j["scaling_diag"]["per_rank_window_s"]) == 8


def test_detail_file_carries_the_rest(tmp_path):
    """The dry --full run writes the full record where --detail says and names it in the line."""
    detail = tmp_path / "detail.json"
    r = _bench("--gpus", "2", "--full", "--dry-gloo", "--steps", "5", "--warmup", "1", "--walkers", "2", "--nwave", "700",
               "--sweep", "", "--detail", str(detail))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and len(lines[0]) <= 4096
    full = json.load(open(detail))
    assert "exposed_gather_note" in full["scaling_diag"]         # the notes are there, not in the line
    assert json.loads(lines[0])["scaling_diag"]["mode"] == "shard"


def _dry_last_step(nwalk, nwave, steps, world):
    """The stub spectra of the last timed step of a dry run: batch (steps - 1) mod nsets of the seeded walkers,
    every rank's block reassembled."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from bart_amd import synth
    case = synth.make_case("unused", nlayers=100, nwave=nwave, kappa_model="survey8d", write=False)
    nsets = max(1, min(16, 4096 // nwalk))
    profs = bench.make_profiles(case, nwalk * nsets, seed=20260103).reshape(nsets, nwalk, -1)
    return bench.StubEngine.expected(torch.from_numpy(profs[(steps - 1) % nsets]), 0, nwave).numpy()


def test_plain_run_times_the_window_and_dumps_its_last_step(tmp_path):
    """A plain run (no --full) prints the contract's line and nothing of the full record: no detail file, no
    scaling_diag.  --dump-outputs writes the spectra of the last timed step, the same on every run."""
    import numpy as np
    dumps = []
    for k in range(2):
        detail, out = tmp_path / ("detail%d.json" % k), tmp_path / ("out%d" % k)
        r = _bench("--gpus", "2", "--dry-gloo", "--steps", "7", "--warmup", "2", "--walkers", "3", "--nwave", "701",
                   "--detail", str(detail), "--dump-outputs", str(out))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        j = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in j, key
        assert j["steps"] == 7 and j["warmup"] == 2 and j["ms_per_step"] > 0 and j["detail"] is None
        assert "scaling_diag" not in j and "parity" not in j and not detail.exists()
        assert sorted(os.listdir(out)) == ["spectra.npy"]
        dumps.append(np.load(out / "spectra.npy"))
    assert dumps[0].dtype == np.float64 and dumps[0].shape == (6, 701)
    assert np.array_equal(dumps[0], dumps[1])
    assert np.array_equal(dumps[0], _dry_last_step(6, 701, 7, 2))


def test_dump_outputs_samples_rows_above_the_limit(tmp_path, monkeypatch):
    """Above the size limit --dump-outputs keeps evenly spaced walkers, the same ones on every run."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    spec = torch.arange(50 * 40, dtype=torch.float64).reshape(50, 40)
    bench.dump_outputs(str(tmp_path / "all"), spec)
    assert np.array_equal(np.load(tmp_path / "all" / "spectra.npy"), spec.numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT", 10 * 40 * 8)
    bench.dump_outputs(str(tmp_path / "some"), spec)
    got = np.load(tmp_path / "some" / "spectra.npy")
    assert got.nbytes <= 10 * 40 * 8 and got.shape == (10, 40)
    assert np.array_equal(got, spec.numpy()[np.linspace(0, 49, 10).round().astype(int)])


@pytest.mark.gpu
def test_plain_gpu_run_dumps_the_last_timed_step(tmp_path):
    """A plain run on the GPU: the contract's line without the --full record, and DIR/spectra.npy = the spectra of
    the last timed step, held to the CPU oracle on the same walkers as the --full line's `parity` holds them."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from bart_amd import synth
    steps = 7
    r = _bench("--steps", str(steps), "--warmup", "2", "--nwave", "2501", "--workdir", str(tmp_path / "w"),
               "--detail", str(tmp_path / "detail.json"), "--dump-outputs", str(tmp_path / "out"))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["steps"] == steps and j["value"] > 0 and j["ms_per_step"] > 0 and j["n_gpus"] == 1
    assert j["roofline"] is None and j["cpu_baseline"] is None and "parity" not in j
    assert not (tmp_path / "detail.json").exists()
    spec = np.load(tmp_path / "out" / "spectra.npy")
    assert spec.dtype == np.float64 and spec.shape == (10, 2501)
    case = synth.make_case(str(tmp_path / "w_survey8d"), nlayers=100, nwave=2501, kappa_model="survey8d", write=False)
    profs = bench.make_profiles(case, 10 * 16, seed=20260103).reshape(16, 10, -1)[(steps - 1) % 16]
    conv = {k: j["config"][k] for k in ("integ", "cut", "cia_interp")}
    rec = bench.parity_record(case, conv, profs, spec, True, "the dumped last step")
    assert rec["ok"], rec
