"""CPU: MC3's other two walks.  `mrw` (bart_amd/csrc/mcmc_core.hpp, State::walk = kWalkMrw) and the samples of a
`unif` model grid (bart_amd/csrc/grid_core.hpp) through a stand-alone host program (tests/walks_core_host.cpp, its own
main, built here with g++ and the address / undefined-behaviour sanitizers) that drives the functions the device
kernels run; held against tests/walks_restate.py.  And the Python side: the configuration of a grid, and the refusal
of both walks by the two loops that used to run DEMC in their place."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcmc_restate as mr  # noqa: E402
import walks_restate as wr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
WALK_MRW = 2


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walks_core") / "walks_core_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "walks_core_host.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        return r.stdout
    return run


A4 = np.array([[1.0, 0.0, 0.5, 0.25], [1.0, 0.3, 0.5, -0.5], [1.0, 0.6, 0.5, 1.0], [1.0, 1.0, 0.5, 0.1], [1.0, 1.5, 0.5, 0.7]])
A5 = np.hstack([A4, np.array([[0.2], [-0.1], [0.4], [0.3], [-0.6]])])


def problem(npars, nch, seed=11, **over):
    """Four parameters: free, free and carrying a two-sided prior, fixed (outside its box), shared with the second.
    Five: a free one more, so that the last normal of the third pair goes unused."""
    A = A4 if npars == 4 else A5
    five = npars == 5
    data = A @ np.array([1.0, 2.0, 7.0, 2.0] + [0.5] * five)
    kw = dict(params=[0.8, 1.9, 7.0, 0.0] + [0.4] * five, pmin=[-5, -5, 0, -5] + [-5] * five, pmax=[5, 5, 5, 5] + [5] * five,
              stepsize=[0.1, 0.1, 0.0, -2] + [0.1] * five, data=data, uncert=np.full(len(data), 0.05), nch=nch, seed=seed,
              prior=[0.0, 2.05, 0.0, 0.0] + [0.0] * five, priorlow=[0.0, 0.04, 0.0, 0.0] + [0.0] * five,
              priorup=[0.0, 0.08, 0.0, 0.0] + [0.0] * five)
    kw.update(over)
    return wr.MrwProblem(**kw), A


def write_problem(path, P, nsteps, thin, A, reject_par, reject_above):
    z = [0.0] * P.npars
    prior = P.prior if P.prior is not None else (z, z, z)
    rows = [[P.nch, P.npars, len(P.data), nsteps, WALK_MRW, P.seed, thin, reject_par, repr(float(reject_above)),
             int(P.prior is not None)],
            P.params, P.pmin, P.pmax, P.stepsize, *prior, P.data, P.uncert, *np.asarray(A, float).tolist()]
    with open(path, "w") as f:
        for r in rows:
            f.write(" ".join(v if isinstance(v, str) else repr(v) for v in r) + "\n")


def read_result(path, nch, npars, ndata, nsteps, thin):
    v = np.fromfile(path)
    assert v[-1] == 1.0
    nk = -(-nsteps // thin)
    sizes = [nch * nk * npars, nch * nk, nch * nk * ndata, nsteps * nch, nch * 4]
    assert v.size == sum(sizes) + 1
    parts = np.split(v[:-1], np.cumsum(sizes)[:-1])
    return (parts[0].reshape(nch, nk, npars), parts[1].reshape(nch, nk), parts[2].reshape(nch, nk, ndata),
            parts[3].reshape(nsteps, nch), parts[4].reshape(nch, 4))


def linear_model(A, reject_par, reject_above):
    def model(rows):
        rows = np.asarray(rows, float)
        status = (rows[:, reject_par] > reject_above).astype(int) if reject_par >= 0 else np.zeros(len(rows), int)
        band = [[-1.0] * len(A) if status[i] else [sum(a * p for a, p in zip(Af, rows[i].tolist()))
                                                   for Af in A.tolist()] for i in range(len(rows))]
        return band, status
    return model


def table(prog, seed, t, nch, npars):
    return np.array([[float.fromhex(v) for v in line.split()] for line in prog("draws", seed, t, nch, npars).strip().split("\n")])


@pytest.mark.parametrize("npars", [4, 5])
@pytest.mark.parametrize("nch", [1, 2, 5])
def test_mrw_draw_for_draw_against_the_restatement(prog, tmp_path, nch, npars):
    """60 iterations, thin 3, a model that rejects the first parameter above 0.95: every accept decision and counter
    exact, values to the tolerances tests/test_mcmc_core_cpu.py holds demc to."""
    nsteps, thin = 60, 3
    P, A = problem(npars, nch)
    write_problem(tmp_path / "p.txt", P, nsteps, thin, A, 0, 0.95)
    prog("run", tmp_path / "p.txt", tmp_path / "o.bin")
    chain, chisq, models, acc, counts = read_result(tmp_path / "o.bin", nch, npars, len(A), nsteps, thin)
    rc, rq, rm, ra, rn = P.loop(linear_model(A, 0, 0.95), nsteps, thin)
    assert np.array_equal(acc, ra)
    assert np.array_equal(counts, rn) and counts[:, 0].sum() > 0
    assert counts[:, 1].sum() > 0 and (acc == 0).any()              # rejected models and refused proposals both occur
    np.testing.assert_allclose(chain, rc, rtol=1e-13, atol=0)
    np.testing.assert_allclose(chisq, rq, rtol=1e-13, atol=0)
    np.testing.assert_allclose(models, rm, rtol=1e-13, atol=0)
    assert chain.shape == (nch, 20, npars)
    assert np.all(chain[:, :, 2] == 7.0)                            # fixed, outside its box: kept, no veto
    assert np.array_equal(chain[:, :, 3], chain[:, :, 1])           # shared: a copy of the second parameter
    assert np.ptp(chain[:, :, 0]) > 0 and chain[:, :, 0].max() <= 0.95


@pytest.mark.parametrize("npars", [4, 5])
@pytest.mark.parametrize("nch", [1, 2, 5])
def test_mrw_known_answer_from_the_draw_table(prog, tmp_path, nch, npars):
    """Uncertainties of 1e30, a box of +-1e6, no priors: every proposal is accepted, so every state is the one before
    plus stepsize_j n_j(t), n_j(t) read from the program's own draw table -- no restatement of the walk involved."""
    nsteps, seed = 12, 5
    big = [1e6] * npars
    P, A = problem(npars, nch, seed=seed, uncert=np.full(5, 1e30), pmin=[-v for v in big], pmax=big, prior=None)
    assert P.prior is None
    write_problem(tmp_path / "p.txt", P, nsteps, 1, A, -1, 0.0)
    prog("run", tmp_path / "p.txt", tmp_path / "o.bin")
    chain, chisq, models, acc, counts = read_result(tmp_path / "o.bin", nch, npars, len(A), nsteps, 1)
    assert counts[:, 0].sum() == nsteps * nch and np.all(acc == 1) and np.all(counts[:, 1:] == 0)
    step = np.array(P.stepsize)
    free = step > 0
    start = np.tile(np.array(P.params), (nch, 1))
    n0 = table(prog, seed, mr.START_T, nch, npars)[:, 9:]
    start[1:, free] = (np.array(P.params) + step * n0)[1:, free]    # the jittered start of every chain but the first
    start[:, 3] = start[:, 1]
    prev = start
    for t in range(nsteps):
        n = table(prog, seed, t, nch, npars)[:, 9:]
        want = prev.copy()
        want[:, free] = (prev + step * n)[:, free]
        want[:, 3] = want[:, 1]
        assert np.array_equal(chain[:, t], want), t
        prev = chain[:, t]
    assert np.all(chain[:, :, 2] == 7.0)


BOX = {1: ([0.3], [-2.0], [1.5], [0.1]),
       4: ([0.8, 1.9, 7.0, 0.0], [-5.0, 1.0, 0.0, -5.0], [5.0, 1.0 + 2.0 ** -40, 5.0, 5.0], [0.1, 0.1, 0.0, -2.0]),
       5: ([0.8, 1.9, 7.0, 0.0, 0.4], [-5.0, -1e-3, 0.0, -5.0, 10.0], [5.0, 3e7, 5.0, 5.0, 10.0], [0.1, 0.1, 0.0, -2.0, 0.3])}


@pytest.mark.parametrize("npars", [1, 4, 5])
def test_unif_samples(prog, npars):
    """The samples of (seed, t, i): the restatement's bits, inside the box, and independent of the number of rows."""
    par, lo, hi, step = BOX[npars]
    got = {}
    for seed, t in ((0, 0), (17, 6), (2 ** 64 - 1, 2 ** 40 + 3)):
        for nrows in (1, 3, 65):
            out = prog("grid", seed, t, nrows, npars, *[repr(v) for v in par + lo + hi + step])
            rows = np.array([[float.fromhex(v) for v in line.split()] for line in out.strip().split("\n")])
            assert rows.shape == (nrows, npars)
            want = np.array(wr.grid_samples(seed, t, nrows, par, lo, hi, step))
            assert rows.tobytes() == want.tobytes(), (seed, t, nrows)
            for j in range(npars):
                if step[j] > 0:
                    assert np.all(rows[:, j] >= lo[j]) and np.all(rows[:, j] <= hi[j])
                elif step[j] == 0:
                    assert np.all(rows[:, j] == par[j])
                else:
                    assert np.array_equal(rows[:, j], rows[:, int(-step[j]) - 1])
            got[seed, t, nrows] = rows
        assert np.array_equal(got[seed, t, 3][2], got[seed, t, 65][2])
        assert np.array_equal(got[seed, t, 1][0], got[seed, t, 65][0])
        free = [j for j in range(npars) if step[j] > 0 and hi[j] > lo[j]]
        assert all(np.ptp(got[seed, t, 65][:, j]) > 0 for j in free)
    assert not np.array_equal(got[0, 0, 65], got[17, 6, 65])


GRID_CFG = """[MCMC]
params = -2.0 0.0 1.0
pmin = -5 -2 -2
pmax = -1 1 1
stepsize = 0.01 0.0 0.01
nchains = 5
numit = 35
walk = unif
modelper = 3
savemodel = grid.npy
"""


def test_a_grid_configuration_needs_no_data(tmp_path):
    from bart_amd import sampler
    (tmp_path / "g.cfg").write_text(GRID_CFG)
    cfg = sampler.SamplerConfig.from_cfg(str(tmp_path / "g.cfg"))
    assert (cfg.walk, cfg.modelper, cfg.nchains, cfg.numit, cfg.savemodel) == ("unif", 3, 5, 35, "grid.npy")
    assert len(cfg.data) == 0 and len(cfg.uncert) == 0
    (tmp_path / "c.cfg").write_text(GRID_CFG.replace("walk = unif", "walk = demc"))
    with pytest.raises(KeyError):                  # a chain still needs its data
        sampler.SamplerConfig.from_cfg(str(tmp_path / "c.cfg"))
    (tmp_path / "d.cfg").write_text(GRID_CFG.replace("modelper = 3\n", "") + "data = 1 2\nuncert = 1 1\n")
    cfg = sampler.SamplerConfig.from_cfg(str(tmp_path / "d.cfg"))
    assert cfg.modelper == 0 and cfg.data.tolist() == [1.0, 2.0]


class NoWorker:
    """A stand-in whose every use fails: the refusal comes before a model or the library is touched."""

    def __getattr__(self, name):
        raise AssertionError("the worker was touched: %s" % name)

    def __call__(self, *a, **k):
        raise AssertionError("the model was called")


@pytest.mark.parametrize("walk", ["mrw", "unif"])
def test_the_host_loops_refuse_the_walks_they_do_not_serve(walk, monkeypatch):
    from bart_amd import sampler, transit_module as trm
    monkeypatch.setattr(trm, "lib", NoWorker())
    cfg = sampler.SamplerConfig(params=np.zeros(2), pmin=-np.ones(2), pmax=np.ones(2), stepsize=np.full(2, 0.1),
                                data=np.zeros(3), uncert=np.ones(3), nchains=4, numit=40, walk=walk)
    with pytest.raises(ValueError, match="run_resident.*run_grid"):
        sampler.run(NoWorker(), cfg)
    with pytest.raises(ValueError, match="run_resident.*run_grid"):
        sampler.run_native(NoWorker(), cfg)
    assert sampler.McmcOpts._fields_[-1] == ("walk", sampler.C.c_int)
