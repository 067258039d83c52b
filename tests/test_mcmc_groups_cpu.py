"""CPU: the grouped resident sampler's host-buildable parts -- mcmc::group_state and start_groups of
bart_amd/csrc/mcmc_core.hpp, check_groups of bart_amd/csrc/retrieval_check.hpp -- through a stand-alone host program
(tests/mcmc_groups_host.cpp, its own main, built here with g++ and the address / undefined-behaviour sanitizers).  The
program lays the groups out in common arrays and evaluates the model once per iteration over all of their rows, as the
device loop does; every group's output must be the BYTES of tests/mcmc_core_host.cpp's solo loop on that group's seed,
data and box."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcmc_restate as mr  # noqa: E402
import test_mcmc_core_cpu as solo  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mcmc_groups")
    exes = {}
    for name in ("mcmc_groups_host", "mcmc_core_host"):
        exes[name] = str(d / name)
        subprocess.check_call(FLAGS + [os.path.join(HERE, name + ".cpp"), "-o", exes[name]])

    def run(name, *args):
        r = subprocess.run([exes[name], *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        return r.stdout
    return run


def _groups(nch, snooker):
    """Three groups of four parameters: other seeds, other data (the truth moved), other boxes; a prior on the second
    group alone; the third shares its last parameter with the first one instead of the second and fixes none."""
    out = []
    for g, (seed, shift) in enumerate(((11, 0.0), (12, 0.15), (2 ** 63 + 5, -0.1))):
        data = solo.A @ (solo.TRUTH + shift * np.array([1.0, -1.0, 0.0, 0.0]))
        z = [0.0] * 4
        prior = ([0.0, 2.05, 0.0, 0.0], [0.0, 0.04, 0.0, 0.0], [0.0, 0.08, 0.0, 0.0]) if g == 1 else (z, z, z)
        out.append(mr.Problem(params=[0.8 + shift, 1.9 - shift, 7.0, 0.0], pmin=[-5 + g, -5, 0, -5],
                              pmax=[5, 5 - 0.5 * g, 5, 5], stepsize=[0.1, 0.1, 0.0, -2] if g < 2 else [0.1, 0.05, 0.2, -1],
                              data=data, uncert=np.full(len(data), 0.05 + 0.01 * g), nch=nch, snooker=snooker, seed=seed,
                              prior=prior[0], priorlow=prior[1], priorup=prior[2]))
    return out


def _write_groups(path, groups, nsteps, thin, A, reject_par, reject_above):
    P0 = groups[0]
    rows = [[len(groups), P0.nch, P0.npars, len(P0.data), nsteps, int(P0.snooker), thin, reject_par,
             repr(float(reject_above))]]
    for P in groups:
        rows += [[P.seed], P.params, P.pmin, P.pmax, P.stepsize, *P.prior, P.data, P.uncert]
    rows += np.asarray(A, float).tolist()
    with open(path, "w") as f:
        for r in rows:
            f.write(" ".join(v if isinstance(v, str) else repr(v) for v in r) + "\n")


@pytest.mark.parametrize("snooker,thin", [(0, 1), (1, 1), (1, 3)])
def test_every_group_is_the_bytes_of_its_solo_loop(progs, tmp_path, snooker, thin):
    """3 groups x 5 chains, 41 iterations; the model rejects the first parameter above 1.02, so some groups re-draw
    start points and meet -1 rows.  Byte for byte: chain, chisq, models, every accept decision and the counters."""
    nsteps, groups = 41, _groups(5, snooker)
    _write_groups(tmp_path / "g.txt", groups, nsteps, thin, solo.A, 0, 1.02)
    progs("mcmc_groups_host", "run", tmp_path / "g.txt", tmp_path / "out")
    seen = []
    for g, P in enumerate(groups):
        solo._write_problem(tmp_path / ("p%d.txt" % g), P, nsteps, thin, solo.A, 0, 1.02)
        progs("mcmc_core_host", "run", tmp_path / ("p%d.txt" % g), tmp_path / ("solo.%d" % g))
        got, want = (open(tmp_path / (stem + ".%d" % g), "rb").read() for stem in ("out", "solo"))
        assert got == want, "group %d differs from its solo loop" % g
        chain, chisq, models, acc, counts = solo._read_result(tmp_path / ("out.%d" % g), 5, 4, len(solo.A), nsteps, thin)
        assert counts[:, 0].sum() > 0 and acc.sum() == counts[:, 0].sum()
        seen.append(chain)
    # the groups are different runs (a slicing that handed every group the first one's rows would pass the above
    # only if the solo runs agreed too)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert np.array_equal(seen[2][:, :, 3], seen[2][:, :, 0]) and np.ptp(seen[2][:, :, 2]) > 0


def test_one_group_is_the_solo_loop(progs, tmp_path):
    P = _groups(4, 1)[1]
    _write_groups(tmp_path / "g.txt", [P], 30, 1, solo.A, -1, 0.0)
    solo._write_problem(tmp_path / "p.txt", P, 30, 1, solo.A, -1, 0.0)
    progs("mcmc_groups_host", "run", tmp_path / "g.txt", tmp_path / "out")
    progs("mcmc_core_host", "run", tmp_path / "p.txt", tmp_path / "solo")
    assert open(tmp_path / "out.0", "rb").read() == open(tmp_path / "solo", "rb").read()


def test_check_names_the_offending_group(progs):
    assert progs("mcmc_groups_host", "check", 3, 5, -1).strip() == "ok 3 groups, 3 free"
    msg = progs("mcmc_groups_host", "check", 3, 5, 2).strip()
    assert msg.startswith("mcmc_groups_host: group 2: stepsize[6] = -7"), msg
    assert "shared" in msg
    assert progs("mcmc_groups_host", "check", 3, 5, 0).startswith("mcmc_groups_host: group 0: stepsize[6]")


def test_limits_of_a_grouped_call(progs):
    ok = lambda G, nch: progs("mcmc_groups_host", "check", G, nch, -1).startswith("ok")
    assert ok(1, 1024) and ok(1024, 1) and ok(4, 256) and ok(102, 10)
    for G, nch in ((5, 205), (1, 1025), (1025, 1), (103, 10), (2 ** 20, 2 ** 20)):        # 1025 rows; past 2^31 rows
        msg = progs("mcmc_groups_host", "check", G, nch, -1).strip()
        assert msg.startswith("mcmc_groups_host: ") and "1024 chains in all" in msg, msg
    for G in (0, -3):
        assert "at least one group" in progs("mcmc_groups_host", "check", G, 5, -1)
    assert "1024" in progs("mcmc_groups_host", "check", 2, 0, -1)
