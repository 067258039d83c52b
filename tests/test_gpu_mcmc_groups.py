"""GPU: several independent retrievals in one resident loop (bartrt_mcmc_run_resident_groups, csrc/mcmc.hip:
mcmc_advance_groups; sampler.run_resident_groups).  A group must be a run of its own: held to the existing single call
byte for byte where the model's launch has the same batch size (G = 1) or the kernel is pinned (a child process under
BARTRT_KERNEL=generic), to itself under changes of the OTHER groups, and to the single-step replay of
tests/test_gpu_mcmc_resident.py group by group.  Case, configuration helper, run, problem and replay are that module's;
every run here makes NSTEPS = 41 iterations in blocks of 8, so blocks hand over and the last one is partial."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_mcmc_resident as T  # noqa: E402
import walks_restate as wr  # noqa: E402
from test_gpu_mcmc_resident import W  # noqa: E402,F401  (the module-scoped worker fixture)

pytestmark = pytest.mark.gpu

N, BLOCK, SENTINEL, EINVAL = T.NSTEPS, 8, -777.0, -1
KEYS = ("chain", "chisq", "models")
MRW_STEP = np.array([0.005, 0.0, 0.0, 0.0, 0.0005, 0.02, -6.0])     # (the stepsizes tests/test_gpu_walks.py walks with)


def three(data, nch=5, walk="snooker", seeds=(9, 31, 57), changed=False, **over):
    """Three groups on one engine: other seeds and other data (noise realisations of the case's spectrum).  `changed`
    alters groups 1 and 2 alone: their data, their boxes, a prior on group 1, a shared parameter in group 2, their
    seeds."""
    rng = np.random.default_rng(5)
    noise = 1.0 + 0.004 * rng.standard_normal((3, len(data)))
    cfgs = [T.scfg(data * noise[g], nch, walk, seed=seeds[g], **over) for g in range(3)]
    if changed:
        z = np.zeros(7)
        prior, lo, up = z.copy(), z.copy(), z.copy()
        prior[5], lo[5], up[5] = -0.48, 0.03, 0.06
        cfgs[1] = T.scfg(data * noise[1] * 1.002, nch, walk, seed=seeds[1] + 100, prior=prior, priorlow=lo, priorup=up,
                         pmin=np.array([-4.0, -2.0, -2.0, 0.0, 0.6, -8.0, -9.0]), **over)
        cfgs[2] = T.scfg(data * noise[2] * 0.998, nch, walk, seed=seeds[2] + 100,
                         stepsize=np.array([0.01, 0.0, 0.0, 0.0, 0.001, 0.05, -6.0]),
                         pmax=np.array([-1.0, 1.0, 1.0, 1.0, 1.15, 1.0, 1.5]), **over)
    return cfgs


def run_groups(W, cfgs, **kw):
    from bart_amd import sampler
    kw.setdefault("block", BLOCK)
    return sampler.run_resident_groups(W.worker, cfgs, **kw)


def same(a, b, keys=KEYS + ("accepted", "nbad")):
    for k in keys:
        x, y = a[k], b[k]
        assert (x.tobytes() == y.tobytes() and x.shape == y.shape) if isinstance(x, np.ndarray) else x == y, k


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["demc", "snooker", "mrw"])
def test_one_group_is_the_existing_call(W, walk):
    """The same batch size, so the same RT kernel serves both: every byte and both counters."""
    for nch in (5, 12):
        over = dict(stepsize=MRW_STEP) if walk == "mrw" else {}
        cfg = T.scfg(W.data, nch, walk, seed=21, **over)
        want = T.run(W, cfg, block=BLOCK)
        got = run_groups(W, [cfg])
        assert len(got) == 1 and got[0]["chain"].shape == (nch, N, 7) and want["accepted"] > 0
        same(got[0], want)


# ---- 2 ----------------------------------------------------------------------------------------------------------------
def test_no_cross_talk(W):
    """15 rows, so the groups straddle a wave's lanes in the model batch: group 0 does not see what the others are."""
    a, b = run_groups(W, three(W.data)), run_groups(W, three(W.data, changed=True))
    same(a[0], b[0])
    assert a[0]["accepted"] > 0
    for g in (1, 2):
        assert not np.array_equal(a[g]["chain"], b[g]["chain"]) and b[g]["accepted"] > 0
    assert np.array_equal(b[2]["chain"][:, :, 6], b[2]["chain"][:, :, 5]) and np.ptp(b[2]["chain"][:, :, 6]) > 0
    assert not np.array_equal(a[0]["chain"], a[1]["chain"]) and not np.array_equal(a[1]["chain"], a[2]["chain"])


# ---- 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["demc", "snooker"])
def test_every_group_replays(W, walk):
    cfgs = three(W.data, walk=walk, changed=True)
    res = run_groups(W, cfgs)
    for cfg, r in zip(cfgs, res):
        assert T.replay(W, cfg, r)["accepted"] > 0


def models_of_all(chains):
    """The band fluxes of every group's chains at every kept row, each row of the result from one model call on the
    rows of ALL groups: the loop's own batch size."""
    from bart_amd import engine
    G, nch, nk, npars = chains.shape
    out = [engine.step_batch(np.ascontiguousarray(chains[:, :, k].reshape(G * nch, npars)), 3)[0] for k in range(nk)]
    return np.stack(out, axis=1).reshape(G, nch, nk, 3)


def test_thinned_groups_with_models(W):
    full = run_groups(W, three(W.data))
    thin = run_groups(W, three(W.data, thinning=3))
    rows = list(range(2, N, 3)) + [N - 1]
    for f, t in zip(full, thin):
        assert t["chain"].shape == (5, 14, 7) and rows[-2:] == [38, 40]
        for key in KEYS:
            assert np.array_equal(t[key], f[key][:, rows]), key
        assert t["accepted"] == f["accepted"] > 0
    want = models_of_all(np.stack([t["chain"] for t in thin]))
    assert np.array_equal(np.stack([t["models"] for t in thin]), want)


def test_one_lane_per_workgroup_mrw_replays(W, monkeypatch):
    """mrw with one chain per group, four groups: every workgroup has one live lane."""
    monkeypatch.setattr(T, "problem", lambda cfg: wr.MrwProblem(cfg.params, cfg.pmin, cfg.pmax, cfg.stepsize, cfg.data,
                                                                cfg.uncert, cfg.nchains, cfg.seed, cfg.prior,
                                                                cfg.priorlow, cfg.priorup))
    cfgs = [T.scfg(W.data * (1.0 + 0.002 * g), 1, "mrw", seed=40 + g, stepsize=MRW_STEP) for g in range(4)]
    res = run_groups(W, cfgs)
    for cfg, r in zip(cfgs, res):
        assert r["chain"].shape == (1, N, 7)
        assert T.replay(W, cfg, r)["accepted"] > 0
    assert not np.array_equal(res[0]["chain"], res[1]["chain"])


# ---- 4 ----------------------------------------------------------------------------------------------------------------
CHILD_SOLO = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import test_gpu_mcmc_groups as V
import test_gpu_mcmc_resident as T
from bart_amd import BARTfunc, synthcfg
case, cfg = synthcfg.make_worker_case(%(tmp)r, **T.CASE)
T.Shared.worker = BARTfunc.Worker(BARTfunc.WorkerConfig.from_cfg(cfg))
data = T.Shared.worker.step(np.array(T.P0))[0].copy()
for walk, thin in (("snooker", 1), ("demc", 3)):
    cfgs = V.three(data, walk=walk, changed=True, thinning=thin)
    res = V.run_groups(T.Shared, cfgs)
    for g, c in enumerate(cfgs):
        solo = T.run(T.Shared, c, block=V.BLOCK)
        V.same(res[g], solo)
        assert solo["accepted"] > 0
T.Shared.worker.close()
print("ok")
"""


def test_group_against_solo_run(tmp_path):
    """Each group's arrays are the bytes of run_resident on that group's configuration alone.  A child process under
    BARTRT_KERNEL=generic, so that the 5-row and the 15-row model launch take the same RT kernel.  Nothing else in the
    launch path reads the batch size under that setting: launch_rt (csrc/kernels.hip) goes straight to the generic
    kernel without consulting the tuned table, and launch_rt_folded -- the preparation fold of one to four walkers,
    BARTRT_FOLD -- returns unfolded when the mode is generic, so it needs no pin of its own."""
    env = dict(os.environ, BARTRT_KERNEL="generic")
    code = CHILD_SOLO % {"root": T.ROOT, "tmp": str(tmp_path / "case")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout.splitlines(), "exit %d\n%s\n%s" % (r.returncode, r.stdout[-1500:],
                                                                                      r.stderr[-3000:])


# ---- the C call itself ------------------------------------------------------------------------------------------------
def call(cfgs, nsteps, thin=1, block=BLOCK, start=None, ngroups=None, nch=None, edit=None, **o):
    """bartrt_mcmc_run_resident_groups on arrays filled with SENTINEL.  Returns the full arrays and every output;
    rc < 0: the refusal, with its message.  ngroups / nch override what is passed; edit(groups) alters the structs."""
    from bart_amd import sampler, transit_module as trm
    G, n = len(cfgs), cfgs[0].nchains
    arrays = [sampler.problem_arrays(c, "test") for c in cfgs]
    groups = (sampler.McmcGroup * max(G, 1))()
    for g, (c, a) in enumerate(zip(cfgs, arrays)):
        groups[g] = sampler.McmcGroup(size=C.sizeof(sampler.McmcGroup), params=a[0].ctypes.data, pmin=a[1].ctypes.data,
                                      pmax=a[2].ctypes.data, stepsize=a[3].ctypes.data, data=a[4].ctypes.data,
                                      uncert=a[5].ctypes.data, seed=c.seed)
        if a[6] is not None:
            groups[g].prior, groups[g].priorlow, groups[g].priorup = (v.ctypes.data for v in a[6])
    if start is not None:
        start = np.ascontiguousarray(start, float)
        for g in range(G):
            groups[g].start = start[g].ctypes.data
    if edit:
        edit(groups)
    nk, ngr = -(-nsteps // thin), 16
    out = dict(chain=np.full((G, n, nk, 7), SENTINEL), chisq=np.full((G, n, nk), SENTINEL),
               models=np.full((G, n, nk, 3), SENTINEL), grstat=np.zeros((ngr, G, 7)), grwhen=np.zeros(ngr, np.int64))
    made, done = C.c_int(-1), C.c_long(-1)
    nacc, nbad, conv = np.full(G, -5, np.int64), np.full((G, 4), -5, np.int64), np.full(G, -5, np.intc)
    opts = sampler.McmcOpts(size=C.sizeof(sampler.McmcOpts), snooker=int(cfgs[0].walk == "snooker"), thin=thin,
                            block=block, ngr=ngr, grstat=out["grstat"].ctypes.data, grwhen=out["grwhen"].ctypes.data,
                            ngr_out=C.addressof(made), done=C.addressof(done))
    for k, v in o.items():
        setattr(opts, k, v)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    lib = trm.lib()
    rc = lib.bartrt_mcmc_run_resident_groups(G if ngroups is None else ngroups, C.cast(groups, C.c_void_p),
                                             n if nch is None else nch, 7, C.c_long(nsteps), 3,
                                             C.cast(C.byref(opts), C.c_void_p), p(out["chain"]), p(out["chisq"]),
                                             p(out["models"]), p(nacc), p(nbad), p(conv))
    out.update(rc=rc, err=lib.bartrt_last_error().decode() if rc < 0 else "", done=done.value, ngr=made.value,
               naccept=nacc.tolist(), nbad=nbad[:, 1:].tolist(), converged_at=conv.tolist(),
               stepsize=[a[3] for a in arrays])
    return out


# ---- 5 ----------------------------------------------------------------------------------------------------------------
SEEDS = ((9, 31, 57), (3, 4, 5), (101, 202, 303), (7, 77, 777))     # the first triple whose history separates the groups


def separating_threshold(h):
    """From a history without exit: (threshold, first test below it per group, first test at which all are), the
    groups' first tests not all the same and the common one not the last test made; None where no recorded value gives
    that."""
    G = h["grstat"].shape[1]
    tops = np.stack([h["grstat"][:h["ngr"], g][:, h["stepsize"][g] > 0].max(axis=1) for g in range(G)], axis=1)
    tops = np.where(np.isfinite(tops), tops, np.inf)                  # [ntests, G]
    for v in sorted(set(tops[np.isfinite(tops)].tolist())):
        thr = (1 + 1e-6) * v
        below = tops < thr
        if not below.any(axis=0).all() or not below.all(axis=1).any():
            continue
        first, common = below.argmax(axis=0).tolist(), int(below.all(axis=1).argmax())
        if len(set(first)) > 1 and common < h["ngr"] - 1:
            return thr, first, common
    return None


def test_convergence_records_and_exit(W):
    from bart_amd import sampler
    for seeds in SEEDS:
        cfgs = three(W.data, seeds=seeds)
        h = call(cfgs, N, burnin=8, grcheck=8)
        # after 8 iterations no row lies past the burn-in; then every 8, and after the last iteration
        assert h["rc"] == 0 and h["done"] == N and h["ngr"] == 5, (h["err"], h["done"], h["ngr"])
        assert h["grwhen"][:5].tolist() == [16, 24, 32, 40, 41] and not h["grwhen"][5:].any()
        found = separating_threshold(h)
        if found:
            break
    else:
        pytest.fail("no seed triple of SEEDS separates the groups' first converged tests: add one that does")
    # every record is the probe's statistic of that group's rows, bit for bit
    for k in range(h["ngr"]):
        for g in range(3):
            want = sampler.gelman_rubin_dev(h["chain"][g], h["stepsize"][g], 8, int(h["grwhen"][k]))[0]
            assert h["grstat"][k, g].tobytes() == want.tobytes(), (k, g)
    assert not h["grstat"][h["ngr"]:].any()
    thr, first, common = found
    stop = int(h["grwhen"][common])
    print("seeds %r: threshold %.9g; first converged tests %r; all at test %d (%d iterations)" % (seeds, thr, first,
                                                                                             common, stop))
    loose = call(cfgs, N, burnin=8, grcheck=8, grthreshold=thr)       # no exit: the same run, converged_at reported
    assert loose["done"] == N and loose["converged_at"] == first
    assert all(loose[k].tobytes() == h[k].tobytes() for k in KEYS)
    e = call(cfgs, N, burnin=8, grcheck=8, grexit=1, grthreshold=thr)
    assert e["rc"] == 0 and e["done"] == stop and e["converged_at"] == first and e["ngr"] == common + 1
    for k in KEYS:
        assert e[k][:, :, :stop].tobytes() == h[k][:, :, :stop].tobytes(), k
        assert (e[k][:, :, stop:] == SENTINEL).all(), k
    plain = call(cfgs, stop)
    assert (e["naccept"], e["nbad"]) == (plain["naccept"], plain["nbad"]) and min(e["naccept"]) > 0
    never = call(cfgs, N, burnin=8, grcheck=8, grexit=1, grthreshold=1.0)
    assert never["done"] == N and never["converged_at"] == [-1, -1, -1]
    assert never["chain"].tobytes() == h["chain"].tobytes()


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_resume(W):
    cfgs = three(W.data, changed=True)[1:]
    whole = call(cfgs, N)
    head = call(cfgs, 24)
    tail = call(cfgs, N - 24, first=24, start=head["chain"][:, :, -1])
    assert whole["rc"] == head["rc"] == tail["rc"] == 0, (whole["err"], head["err"], tail["err"])
    for k in KEYS:
        assert np.concatenate([head[k], tail[k]], axis=2).tobytes() == whole[k].tobytes(), k
    assert not (whole["chain"] == SENTINEL).any() and min(whole["naccept"]) > 0
    assert [a + b for a, b in zip(head["naccept"], tail["naccept"])] == whole["naccept"]
    assert (np.array(head["nbad"]) + np.array(tail["nbad"])).tolist() == whole["nbad"]
    # first and start come together, in every group
    for kw in (dict(first=24), dict(start=head["chain"][:, :, -1])):
        r = call(cfgs, N - 24, **kw)
        assert r["rc"] == EINVAL and "start" in r["err"], r["err"]


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_refusals(W):
    cfgs = three(W.data)
    z = np.zeros(7)

    def size0(groups):
        groups[1].size = 0

    def lone_prior(groups):
        groups[2].prior = z.ctypes.data

    many = [T.scfg(W.data, 205, "demc", seed=g) for g in range(5)]                   # 1025 rows
    cases = (("no group", dict(ngroups=0), "at least one group"),
             ("1025 rows", dict(cfgs=many), "1024 chains in all"),
             ("opts seed", dict(seed=7), "opts->seed"),
             ("size 0", dict(edit=size0), "group 1: set size"),
             ("lone prior", dict(edit=lone_prior), "group 2: prior, priorlow and priorup come together"),
             ("unif", dict(walk=3), "bartrt_grid_run"))
    for name, kw, word in cases:
        r = call(kw.pop("cfgs", cfgs), 3, **kw)
        assert r["rc"] == EINVAL, (name, r["rc"], r["err"])
        assert r["err"].startswith("mcmc_run_resident_groups: ") and word in r["err"], (name, r["err"])
        assert (r["chain"] == SENTINEL).all(), name
    bad = three(W.data)
    bad[2].stepsize = np.array([0.01, 0.0, 0.0, 0.0, 0.001, 0.05, -7.0])
    r = call(bad, 3)
    assert r["rc"] == EINVAL and r["err"].startswith("mcmc_run_resident_groups: group 2: stepsize[6] = -7"), r["err"]
    with pytest.raises(ValueError, match="`thinning`"):
        run_groups(W, [cfgs[0], T.scfg(W.data, 5, "snooker", thinning=2)])
    ok = call(cfgs, 3)
    assert ok["rc"] == 0 and not (ok["chain"] == SENTINEL).any()
