"""GPU: `retrieve --resident --datasets FILE` (bart_amd/retrieve.py: ensemble): one retrieval per row of the file's
`data` in one resident loop, each written to its own group_<g>/ directory as a run of its own writes its files.  The
runs are made in a child process with a time limit of its own, under BARTRT_KERNEL=generic so that the two-group
launch and the solo launch take the same RT kernel (tests/test_gpu_mcmc_groups.py, test_group_against_solo_run, says
why that pin is enough)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_mcmc_resident as T  # noqa: E402

pytestmark = pytest.mark.gpu

NCH = 5


def write_cfg(root, name, data, **over):
    """The case of tests/test_gpu_mcmc_resident.py as a configuration file with its [MCMC] section."""
    from bart_amd import synthcfg
    sc = T.scfg(np.asarray(data, float), NCH, "snooker")
    line = lambda v: " ".join(repr(float(x)) for x in v)
    case, cfg = synthcfg.make_worker_case(os.path.join(root, name), **T.CASE)
    head, tail = open(cfg).read().split("[MCMC]", 1)
    kw = dict(params=line(sc.params), pmin=line(sc.pmin), pmax=line(sc.pmax), stepsize=line(sc.stepsize),
              data=line(sc.data), uncert=line(sc.uncert), nchains=str(NCH), numit=str(NCH * T.NSTEPS), burnin="8",
              walk="snooker", grtest="True", grcheck="8", seed="9", savemodel="band.npy")
    kw.update(over)
    keep = [l for l in tail.split("\n") if l.split("=")[0].strip() not in kw]
    with open(cfg, "w") as f:
        f.write(head + "[MCMC]\n" + "\n".join("%s = %s" % kv for kv in kw.items()) + "\n" + "\n".join(keep))
    return cfg


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import test_retrieve_datasets as V
import test_gpu_mcmc_resident as T
from bart_amd import BARTfunc, retrieve, synthcfg
tmp = %(tmp)r
case, cfg = synthcfg.make_worker_case(os.path.join(tmp, "probe"), **T.CASE)
w = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
data = w.step(np.array(T.P0))[0].copy()
w.close()
sets = np.stack([data * 1.003, data * 0.996])
np.savez(os.path.join(tmp, "sets.npz"), data=sets, seed=np.array([9, 44]))
res = retrieve.main(["-c", V.write_cfg(tmp, "both", data), "--resident", "--datasets", os.path.join(tmp, "sets.npz"),
                     "--out", os.path.join(tmp, "o_both")])
assert len(res) == 2 and res[1]["chain"].shape == (V.NCH, T.NSTEPS, 7)
# the uncertainties of a solo run on the second data set: the configuration's own, as --datasets keeps them
line = lambda v: " ".join(repr(float(x)) for x in v)
solo_cfg = V.write_cfg(tmp, "solo", sets[1], uncert=line(0.01 * np.abs(data)), seed="44")
retrieve.main(["-c", solo_cfg, "--resident", "--out", os.path.join(tmp, "o_solo")])
print("ok")
"""


def test_two_datasets_write_two_runs(tmp_path):
    env = dict(os.environ, BARTRT_KERNEL="generic")
    code = CHILD % {"root": T.ROOT, "tmp": str(tmp_path)}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout.splitlines(), "exit %d\n%s\n%s" % (r.returncode, r.stdout[-1500:],
                                                                                      r.stderr[-3000:])
    both, solo = str(tmp_path / "o_both"), str(tmp_path / "o_solo")
    for g in (0, 1):
        d = os.path.join(both, "group_%03d" % g)
        assert sorted(os.listdir(d)) == ["MCMC.log", "band.npy", "bestFit.txt", "output.npy", "state.npz"], os.listdir(d)
        assert np.load(os.path.join(d, "output.npy")).shape == (NCH, T.NSTEPS, 7)
        assert np.load(os.path.join(d, "band.npy")).shape == (NCH, 3, T.NSTEPS)
        state = np.load(os.path.join(d, "state.npz"))
        assert (int(state["iterations"]), int(state["seed"]), int(state["nchains"])) == (T.NSTEPS, (9, 44)[g], NCH)
        log = open(os.path.join(d, "MCMC.log")).read()
        assert "group %d: Gelman-Rubin after 16 iterations" % g in log and "group %d:" % (1 - g) not in log
        assert "models of 2 groups" in log and "models/s" in log
    a, b = (np.load(os.path.join(both, "group_%03d" % g, "output.npy")) for g in (0, 1))
    assert not np.array_equal(a, b)
    d = os.path.join(both, "group_001")
    for name in ("output.npy", "band.npy"):
        got, want = np.load(os.path.join(d, name)), np.load(os.path.join(solo, name))
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert open(os.path.join(d, "bestFit.txt")).read() == open(os.path.join(solo, "bestFit.txt")).read()
    s1, s2 = np.load(os.path.join(d, "state.npz")), np.load(os.path.join(solo, "state.npz"))
    assert int(s1["naccept"]) == int(s2["naccept"]) > 0 and s1["nbad"].tolist() == s2["nbad"].tolist()


@pytest.mark.parametrize("extra,over,sentence", [
    (["--resume"], {}, "--datasets with --resume: an ensemble is not resumed from the command line."),
    (["--leastsq"], {}, "--datasets with leastsq: the fit before the chain is not run per group."),
    ([], dict(leastsq="True"), "--datasets with leastsq: the fit before the chain is not run per group."),
    ([], dict(leastsq="True", chisqscale="True"), "--datasets with chisqscale: the uncertainties are not rescaled per group."),
    ([], dict(walk="unif"), "--datasets with walk = unif: a model grid has no data to vary."),
])
def test_what_does_not_go_with_datasets(tmp_path, capsys, extra, over, sentence):
    """Refused before any engine is made: --resume, leastsq, chisqscale and walk = unif."""
    from bart_amd import retrieve
    np.savez(tmp_path / "sets.npz", data=np.ones((2, 3)))
    cfg = write_cfg(str(tmp_path), "case", np.ones(3), **over)
    with pytest.raises(SystemExit) as err:
        retrieve.main(["-c", cfg, "--resident", "--datasets", str(tmp_path / "sets.npz"), "--out", str(tmp_path / "o")]
                      + extra)
    assert err.value.code != 0 and sentence in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "o")
