"""CPU: the resident sampler's arithmetic (bart_amd/csrc/mcmc_core.hpp) through a stand-alone host program
(tests/mcmc_core_host.cpp, its own main, built here with g++ and the address / undefined-behaviour sanitizers) that
drives the very propose / finish functions the device kernel runs, over an analytic model band = A p.  Held against
tests/mcmc_restate.py, a restatement in plain Python that carries its own Philox."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcmc_restate as mr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mcmc_core") / "mcmc_core_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "mcmc_core_host.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        return r.stdout
    run.exe = exe
    return run


KAT = [([0, 0, 0, 0], (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ([mr.MASK] * 4, (mr.MASK, mr.MASK), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0),
        "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers(prog):
    lines = prog("philox").split("\n")
    for (ctr, key, want), got in zip(KAT, lines):
        assert got == want
        assert " ".join("%08x" % w for w in mr.philox(ctr, key)) == want     # the restatement's own generator


def test_uniforms_strictly_inside_the_unit_interval_and_draw_tables(prog):
    lo, hi = (float.fromhex(v) for v in prog("edges").split())
    assert lo == 2.0 ** -54 and hi == 1.0 - 2.0 ** -53 and 0.0 < lo and hi < 1.0
    assert (mr.uniform53(0, 0), mr.uniform53(mr.MASK, mr.MASK)) == (lo, hi)
    worst = 0.0
    for seed, t, nch, npars in ((0, 0, 1, 1), (7, 3, 2, 5), (2 ** 64 - 1, 10, 3, 4), (0x123456789ABCDEF, 2 ** 40 + 5, 11, 7),
                                (5, mr.START_T + 2, 64, 6)):
        rows = [[float.fromhex(v) for v in line.split()] for line in prog("draws", seed, t, nch, npars).strip().split("\n")]
        assert len(rows) == nch
        for i, row in enumerate(rows):
            want = mr.draws_row(seed, t, nch, i, npars)
            assert row[:5] == want[:5] and row[6:9] == want[6:9], (seed, t, i)            # uniforms, partners: exact
            assert all(0.0 < u < 1.0 for u in row[:5])
            if nch > 3:
                assert len({i, int(row[6]), int(row[7]), int(row[8])}) == 4                # distinct partners
            np.testing.assert_allclose(row[5:6] + row[9:], want[5:6] + want[9:], rtol=1e-13, atol=1e-15)
            worst = max(worst, max(abs(a - b) for a, b in zip(row[9:], want[9:])))
    print("draw tables: largest difference of a normal against the restatement %.3g" % worst)


A = np.array([[1.0, 0.0, 0.5, 0.25], [1.0, 0.3, 0.5, -0.5], [1.0, 0.6, 0.5, 1.0], [1.0, 1.0, 0.5, 0.1], [1.0, 1.5, 0.5, 0.7]])
TRUTH = np.array([1.0, 2.0, 7.0, 2.0])


def _problem(nch, snooker, seed=11):
    """Four parameters: free, free and carrying a two-sided prior, fixed (outside its box), shared with the second."""
    data = A @ TRUTH
    return mr.Problem(params=[0.8, 1.9, 7.0, 0.0], pmin=[-5, -5, 0, -5], pmax=[5, 5, 5, 5], stepsize=[0.1, 0.1, 0.0, -2],
                      data=data, uncert=np.full(len(data), 0.05), nch=nch, snooker=snooker, seed=seed,
                      prior=[0.0, 2.05, 0.0, 0.0], priorlow=[0.0, 0.04, 0.0, 0.0], priorup=[0.0, 0.08, 0.0, 0.0])


def _write_problem(path, P, nsteps, thin, A, reject_par, reject_above):
    z = [0.0] * P.npars
    prior = P.prior if P.prior is not None else (z, z, z)
    rows = [[P.nch, P.npars, len(P.data), nsteps, int(P.snooker), P.seed, thin, reject_par, repr(float(reject_above))],
            P.params, P.pmin, P.pmax, P.stepsize, *prior, P.data, P.uncert, *np.asarray(A, float).tolist()]
    with open(path, "w") as f:
        for r in rows:
            f.write(" ".join(v if isinstance(v, str) else repr(v) for v in r) + "\n")


def _read_result(path, nch, npars, ndata, nsteps, thin):
    v = np.fromfile(path)
    assert v[-1] == 1.0
    nk = -(-nsteps // thin)
    sizes = [nch * nk * npars, nch * nk, nch * nk * ndata, nsteps * nch, nch * 4]
    assert v.size == sum(sizes) + 1
    parts = np.split(v[:-1], np.cumsum(sizes)[:-1])
    return (parts[0].reshape(nch, nk, npars), parts[1].reshape(nch, nk), parts[2].reshape(nch, nk, ndata),
            parts[3].reshape(nsteps, nch), parts[4].reshape(nch, 4))


def _linear_model(A, reject_par, reject_above):
    def model(rows):
        rows = np.asarray(rows, float)
        status = (rows[:, reject_par] > reject_above).astype(int) if reject_par >= 0 else np.zeros(len(rows), int)
        band = [[-1.0] * len(A) if status[i] else [sum(a * p for a, p in zip(Af, rows[i].tolist()))
                                                   for Af in A.tolist()] for i in range(len(rows))]
        return band, status
    return model


@pytest.mark.parametrize("snooker", [0, 1])
@pytest.mark.parametrize("nch", [1, 2, 3, 4, 11])
def test_draw_for_draw_against_the_restatement(prog, tmp_path, nch, snooker):
    """200 iterations: the program's chain is the restatement's, every accept decision included."""
    nsteps, P = 200, _problem(nch, snooker)
    # (the model rejects the first parameter above 1.02: some in-box proposals come back as -1 rows)
    _write_problem(tmp_path / "p.txt", P, nsteps, 1, A, 0, 1.02)
    prog("run", tmp_path / "p.txt", tmp_path / "o.bin")
    chain, chisq, models, acc, counts = _read_result(tmp_path / "o.bin", nch, 4, len(A), nsteps, 1)
    rc, rq, rm, ra, rn = P.loop(_linear_model(A, 0, 1.02), nsteps)
    assert np.array_equal(acc, ra)
    assert np.array_equal(counts, rn) and counts[:, 0].sum() > 0
    assert nch < 3 or counts[:, 1].sum() > 0       # (one or two chains move by their jitter alone: too little to get there)
    np.testing.assert_allclose(chain, rc, rtol=1e-13, atol=0)
    np.testing.assert_allclose(chisq, rq, rtol=1e-13, atol=0)
    np.testing.assert_allclose(models, rm, rtol=1e-13, atol=0)
    assert np.all(chain[:, :, 2] == 7.0)                            # fixed, outside its box: kept, no veto
    assert np.array_equal(chain[:, :, 3], chain[:, :, 1])           # shared: a copy of the second parameter
    assert np.ptp(chain[:, :, 0]) > 0 and chain[:, :, 0].max() <= 1.02


def test_thinning_writes_every_nth_row_and_the_last(prog, tmp_path):
    P = _problem(5, 1)
    _write_problem(tmp_path / "a.txt", P, 41, 1, A, -1, 0.0)
    _write_problem(tmp_path / "b.txt", P, 41, 3, A, -1, 0.0)
    prog("run", tmp_path / "a.txt", tmp_path / "a.bin")
    prog("run", tmp_path / "b.txt", tmp_path / "b.bin")
    full = _read_result(tmp_path / "a.bin", 5, 4, len(A), 41, 1)
    thin = _read_result(tmp_path / "b.bin", 5, 4, len(A), 41, 3)
    rows = list(range(2, 41, 3)) + [40]
    assert thin[0].shape == (5, 14, 4) and rows[-2] == 38
    for k in range(3):
        assert np.array_equal(thin[k], full[k][:, rows])
    assert np.array_equal(thin[3], full[3]) and np.array_equal(thin[4], full[4])


@pytest.mark.parametrize("snooker", [0, 1])
def test_recovers_a_gaussian_posterior(prog, tmp_path, snooker):
    """The case and the bounds of tests/test_sampler.py::test_recovers_a_gaussian_posterior, same chain length."""
    x = np.linspace(0, 1, 12)
    A3 = np.stack([np.ones(12), x, np.zeros(12)], axis=1)
    data = A3 @ np.array([1.0, 2.0, 7.0])
    P = mr.Problem(params=[0.5, 1.0, 7.0], pmin=[-5.0, -5.0, 0.0], pmax=[5.0, 5.0, 10.0], stepsize=[0.1, 0.1, 0.0],
                   data=data, uncert=np.full(12, 0.05), nch=8, snooker=snooker, seed=3)
    nsteps = 16000 // 8
    _write_problem(tmp_path / "p.txt", P, nsteps, 1, A3, 1, 4.5)
    prog("run", tmp_path / "p.txt", tmp_path / "o.bin")
    chain, chisq, models, acc, counts = _read_result(tmp_path / "o.bin", 8, 3, 12, nsteps, 1)
    post = chain[:, 500:, :].reshape(-1, 3)
    assert np.all(post[:, 2] == 7.0)
    print("mean %r std %r" % (post.mean(axis=0).tolist(), post.std(axis=0).tolist()))
    assert abs(post[:, 0].mean() - 1.0) < 0.02 and abs(post[:, 1].mean() - 2.0) < 0.04
    cov = np.linalg.inv(np.array([[12, x.sum()], [x.sum(), (x ** 2).sum()]]) / 0.05 ** 2)
    assert abs(post[:, 0].std() / np.sqrt(cov[0, 0]) - 1) < 0.25
    assert abs(post[:, 1].std() / np.sqrt(cov[1, 1]) - 1) < 0.25
    rate = counts[:, 0].sum() / (nsteps * 8)
    assert 0.05 < rate < 0.7 and chisq.min() < 1e-2
    assert np.all(post[:, 1] <= 4.5)


def test_shared_parameter_validation(prog):
    assert prog("check", 3, 0.1, -1, 0.0).strip() == "0"         # shared with a free parameter
    assert prog("check", 3, 0.1, 0.0, -2).strip() == "0"         # shared with a fixed one
    assert prog("check", 3, 0.1, -3, -1).strip() == "2"          # shared with a shared one
    assert prog("check", 3, 0.1, 0.2, -4).strip() == "3"         # k > npars
    assert prog("check", 3, -0.5, 0.2, 0.1).strip() == "1"       # k = 0 (and not an integer)
    assert prog("check", 2, 0.1, -1.5).strip() == "2"            # not an integer
    assert prog("check", 1, -1).strip() == "1"                   # shared with itself
