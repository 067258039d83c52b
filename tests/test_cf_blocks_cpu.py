"""CPU: the arithmetic behind contribution functions on wavenumber-sharded engines (include/bartrt.h,
bartrt_cf_setup_block / _partials_dev / _combine_dev), restated in numpy and held to np.trapz.

A filter window is stated on the full grid; each rank integrates the part of it that lies in its block [lo, hi).
The restatement below is what contrib.hip's cf_setup builds for a block: the response at every sample of the clipped
window, halved at the window's TRUE first and last sample only, 1 where a block cuts the window.  The blocks' weighted
sums, added and divided by the whole window's trapz(resp), must be filter_cf's band average of the whole window.
Also here: the new entry points are exported with the declared signatures and refuse to run without an engine, the
block split of the restatement is the engine's (engine.block_sizes restates Engine::setup; the GPU tests hold
bartrt_get_local_range to the same split), and the host half of cf.posterior is untouched by the sharding arguments."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
trapz = getattr(np, "trapezoid", None) or np.trapz      # (np.trapz under its newer name where numpy has one)

SIGNATURES = {
    "bartrt_cf_setup_block": "int, const int *, const int *, const double *",
    "bartrt_cf_partials_dev": "const double *, int, int, const double *, double *, double *, unsigned char *, void *",
    "bartrt_cf_combine_dev": "const double *, int, int, const unsigned char *, double *, void *",
}


def starts(total, n):
    """Engine::setup's split: block r = [total r // n, total (r + 1) // n)."""
    return [total * r // n for r in range(n + 1)]


def block_weights(idx0, npts, resp, lo, hi):
    """-> (first sample, weights) of the window [idx0, idx0 + npts) clipped to [lo, hi); empty if they do not meet."""
    a, b = max(idx0, lo), min(idx0 + npts, hi)
    if a >= b:
        return a, np.zeros(0)
    i = np.arange(a, b)
    half = (i == idx0) | (i == idx0 + npts - 1)
    return a, np.where(half, 0.5, 1.0) * resp[a - idx0:b - idx0]


def block_sum(x, idx0, npts, resp, lo, hi):
    a, w = block_weights(idx0, npts, resp, lo, hi)
    return float(np.sum(x[a:a + w.size] * w))


def whole(x, idx0, npts, resp):
    return trapz(x[idx0:idx0 + npts] * resp) / trapz(resp)


def test_a_window_cut_at_every_position_adds_up_to_the_whole_windows_trapezoid():
    rng = np.random.default_rng(1)
    total, idx0, npts = 97, 11, 40
    x, resp = rng.uniform(0.5, 2.0, total), rng.uniform(0.2, 1.0, npts)
    ref = whole(x, idx0, npts, resp)
    for cut in range(0, total + 1):                      # two blocks, the edge anywhere (outside the window too)
        s = block_sum(x, idx0, npts, resp, 0, cut) + block_sum(x, idx0, npts, resp, cut, total)
        assert abs(s / trapz(resp) - ref) <= 4 * npts * 2.0 ** -53 * ref, cut
    for c1 in range(idx0, idx0 + npts + 1):              # three blocks, both edges anywhere in the window
        for c2 in range(c1, idx0 + npts + 1):
            s = sum(block_sum(x, idx0, npts, resp, lo, hi) for lo, hi in ((0, c1), (c1, c2), (c2, total)))
            assert abs(s / trapz(resp) - ref) <= 4 * npts * 2.0 ** -53 * ref, (c1, c2)


def test_the_engines_split_of_an_odd_grid_adds_up_for_every_rank_count():
    rng = np.random.default_rng(2)
    total = 1777
    x = rng.uniform(0.0, 3.0, total)
    for n in (1, 2, 3, 5, 8):
        s = starts(total, n)
        for idx0, npts in ((s[n // 2] + 2, 41), (total // 20, total - 2 * (total // 20)), (s[1] - 1 if n > 1 else 888, 2),
                           (0, 25), (total - 30, 30)):
            resp = rng.uniform(0.2, 1.0, npts)
            parts = [block_sum(x, idx0, npts, resp, s[r], s[r + 1]) for r in range(n)]
            got = sum(parts) / trapz(resp)
            ref = whole(x, idx0, npts, resp)
            assert abs(got - ref) <= 4 * npts * 2.0 ** -53 * ref, (n, idx0, npts)
            # a rank without a sample of the window contributes exactly 0
            for r in range(n):
                if s[r + 1] <= idx0 or s[r] >= idx0 + npts:
                    assert parts[r] == 0.0


def test_the_end_halves_land_on_the_true_ends_only():
    resp = np.linspace(1.0, 2.0, 10)
    idx0, npts = 20, 10
    _, w0 = block_weights(idx0, npts, resp, 0, 24)       # holds the first sample, cut after four
    _, w1 = block_weights(idx0, npts, resp, 24, 27)      # the middle: both edges are cuts
    _, w2 = block_weights(idx0, npts, resp, 27, 64)      # holds the last sample
    assert np.array_equal(w0, resp[:4] * [0.5, 1, 1, 1])
    assert np.array_equal(w1, resp[4:7])
    assert np.array_equal(w2, resp[7:] * [1, 1, 0.5])
    # uncut: np.trapz's own weights
    _, w = block_weights(idx0, npts, resp, 0, 64)
    assert np.array_equal(w, resp * ([0.5] + [1] * 8 + [0.5]))
    # a block that starts at the window's first sample / ends on its last still halves it
    assert block_weights(idx0, npts, resp, 20, 21)[1][0] == 0.5 * resp[0]
    assert block_weights(idx0, npts, resp, 29, 30)[1][0] == 0.5 * resp[-1]


def test_a_two_sample_window_split_one_and_one():
    x = np.array([0.0, 3.0, 5.0, 0.0])
    resp = np.array([0.4, 0.8])
    a = block_sum(x, 1, 2, resp, 0, 2)
    b = block_sum(x, 1, 2, resp, 2, 4)
    assert a == 0.5 * 3.0 * 0.4 and b == 0.5 * 5.0 * 0.8
    assert (a + b) / trapz(resp) == pytest.approx(whole(x, 1, 2, resp), rel=1e-15)


def test_the_split_is_the_engines():
    """engine.block_sizes restates Engine::setup's W r / n (what bartrt_get_local_range reports and bartrt_comm_init
    checks; tests/test_gpu_cf_blocks.py holds the library to it on an engine)."""
    from bart_amd import engine
    for total, n in ((1777, 1), (1777, 2), (1777, 3), (1777, 5), (2424, 8), (10, 4)):
        s = starts(total, n)
        assert [s[r + 1] - s[r] for r in range(n)] == engine.block_sizes(total, n)
        assert s[0] == 0 and s[-1] == total
    assert starts(1777, 2) == [0, 888, 1777]
    assert all(s % 64 for n in (2, 3, 5) for s in starts(1777, n)[1:-1])


@pytest.fixture(scope="module")
def lib():
    from bart_amd import build, transit_module as trm
    build.build()
    return trm.lib()


def test_the_three_symbols_have_the_declared_signatures(lib, tmp_path):
    tu = tmp_path / "sig.c"
    lines = ['#include "bartrt.h"']
    lines += ["int (*p_%s)(%s) = %s;" % (n, args, n) for n, args in SIGNATURES.items()]
    lines.append("int main(void) { return p_bartrt_cf_combine_dev == 0; }")
    tu.write_text("\n".join(lines) + "\n")
    libdir = os.path.join(ROOT, "bart_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tu),
                           "-L" + libdir, "-lbartrt", "-Wl,-rpath," + libdir, "-o", str(tmp_path / "sig")])
    for n, args in SIGNATURES.items():
        fn = getattr(lib, n)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args.split(",")), n


def test_without_an_engine_the_calls_fail_and_do_not_crash(lib):
    from bart_amd import transit_module as trm
    trm.free_memory()
    p = trm._ptr
    idx0, npts, resp = np.zeros(1, np.int32), np.full(1, 2, np.int32), np.ones(2)
    x, part = np.zeros((2, 8)), np.zeros((2, 1, 10))
    assert lib.bartrt_cf_setup_block(1, p(idx0), p(npts), p(resp)) == EINVAL
    assert b"not initialised" in lib.bartrt_last_error()
    assert lib.bartrt_cf_partials_dev(p(x), 2, 0, None, p(part), None, None, None) == EINVAL
    assert lib.bartrt_cf_combine_dev(p(part), 1, 2, None, p(part), None) == EINVAL


def test_the_header_no_longer_calls_sharded_engines_unsupported():
    import re
    text = re.sub(r"\s*\n\s*\*\s*", " ", open(os.path.join(ROOT, "include", "bartrt.h")).read())
    assert "bartrt_cf_setup_block" in text and "Contribution functions stay unsupported" not in text


def test_posterior_samples_is_unchanged_and_posterior_passes_the_sharding_on(tmp_path, monkeypatch):
    from bart_amd import cf
    rng = np.random.default_rng(4)
    params = np.array([1.0, 2.0, 3.0, 4.0])
    stepsize = np.array([0.1, 0.0, 0.2, 0.0])
    data = rng.normal(size=(3, 2, 50))                   # MC3: [nchains, nfree, niter]
    got = cf.posterior_samples(data, params, stepsize, burnin=10, thinning=4)
    kept = data[:, :, 10::4]
    want = np.tile(params, (3 * kept.shape[2], 1))
    want[:, [0, 2]] = kept.transpose(0, 2, 1).reshape(-1, 2)
    assert np.array_equal(got, want) and got.shape == (30, 4)
    own = rng.normal(size=(2, 20, 4))                    # bart_amd.retrieve: [nchains, nsteps, npars]
    got = cf.posterior_samples(own, params, stepsize, burnin=5)
    want = own[:, 5:, :].reshape(-1, 4).copy()
    want[:, [1, 3]] = params[[1, 3]]
    assert np.array_equal(got, want)

    cfg = tmp_path / "run.cfg"
    cfg.write_text("[MCMC]\nparams = 1.0 2.0 3.0 4.0\nstepsize = 0.1 0.0 0.2 0.0\n")
    seen = []

    def stub(cfg_path, samples, filters, kind, chunk, **kw):
        seen.append(kw)
        return np.ones((len(samples), 1, 3)), np.zeros(len(samples), np.int32), "contribution"

    monkeypatch.setattr(cf, "_run_samples", stub)
    monkeypatch.delenv("BARTRT_GPUS", raising=False)
    cf.posterior(data, str(cfg), ["f.dat"], burnin=10)
    cf.posterior(data, str(cfg), ["f.dat"], burnin=10, shard=(1, 2), device=0)
    assert seen == [{}, {"shard": (1, 2), "device": 0, "group": None}]
    monkeypatch.setenv("BARTRT_GPUS", "2")               # ... needs a process group of two ranks
    with pytest.raises(ValueError, match="BARTRT_GPUS"):
        cf.posterior(data, str(cfg), ["f.dat"], burnin=10)
