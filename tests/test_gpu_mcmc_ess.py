"""GPU: the effective sample size of the resident sampler (csrc/mcmc.hip: mcmc_ess_lags, mcmc_ess_finish;
bartrt_mcmc_ess; bartrt_mcmc_run_resident with esstarget / essexit / maxlag / essstat / esstau).

The statistic is held to the host build of csrc/ess_core.hpp (tests/ess_core_host.cpp), byte for byte but for the sign
of a NaN (ess_restate.same), on the smallest shapes at which the kernel's sliding window can go wrong: fewer rows than
one window, one row past a window, 255 / 256 / 257 lags across the lane-block edge, the lag count clamped to n - 1,
one chain.  The loop is held to the probe on its own chain, to the plain-Python restatement for where it stops, and to
itself for a resumed run.  The case and the configuration helper are those of tests/test_gpu_mcmc_resident.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ess_restate as er  # noqa: E402
import gr_restate as gr  # noqa: E402
import test_gpu_mcmc_resident as T  # noqa: E402

pytestmark = pytest.mark.gpu

N, BLOCK, BURNIN = 1024, 256, 128
NGR = 8
SENTINEL = -777.0
SEED = 9


@pytest.fixture(scope="module")
def W(tmp_path_factory):
    from bart_amd import BARTfunc, synthcfg
    case, cfg = synthcfg.make_worker_case(str(tmp_path_factory.mktemp("ess")), **T.CASE)
    T.Shared.wcfg = BARTfunc.WorkerConfig.from_cfg(cfg)
    T.Shared.worker = BARTfunc.Worker(T.Shared.wcfg)
    T.Shared.data = T.Shared.worker.step(np.array(T.P0))[0].copy()
    yield T.Shared
    if T.Shared.worker is not None:
        T.Shared.worker.close()
    T.Shared.worker = None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return er.build_host(tmp_path_factory.mktemp("ess_core"))


def problem(data, nch, walk, seed):
    from bart_amd import sampler
    return sampler.problem_arrays(T.scfg(data, nch, walk, seed=seed), "test")


def call(data, nsteps, walk="snooker", seed=SEED, nch=5, **o):
    """bartrt_mcmc_run_resident itself, on arrays filled with SENTINEL, block 256, grcheck 256 and burnin 128 unless
    told otherwise.  rc < 0: the call's refusal, with its message."""
    from bart_amd import sampler, transit_module as trm
    par, pmin, pmax, step, dat, unc, _ = problem(data, nch, walk, seed)
    out = dict(chain=np.full((nch, nsteps, 7), SENTINEL), chisq=np.full((nch, nsteps), SENTINEL),
               grstat=np.full((NGR, 7), SENTINEL), grwhen=np.zeros(NGR, np.int64),
               essstat=np.full((NGR, 7), SENTINEL), esstau=np.full((NGR, nch, 7), SENTINEL))
    made, done, nacc, nbad = C.c_int(-1), C.c_long(-1), C.c_long(-1), (C.c_long * 4)()
    opts = sampler.McmcOptsEss(size=C.sizeof(sampler.McmcOptsEss), snooker=int(walk == "snooker"), seed=seed, thin=1,
                               block=BLOCK, burnin=BURNIN, grcheck=BLOCK, ngr=NGR, grstat=out["grstat"].ctypes.data,
                               grwhen=out["grwhen"].ctypes.data, ngr_out=C.addressof(made), done=C.addressof(done),
                               walk=sampler.WALK_MRW if walk == "mrw" else 0, essstat=out["essstat"].ctypes.data,
                               esstau=out["esstau"].ctypes.data)
    start = o.pop("start", None)
    if start is not None:
        start = np.ascontiguousarray(start, float)
        opts.start = start.ctypes.data
    for k, v in o.items():
        setattr(opts, k, v)
    if not opts.esstarget > 0:
        opts.essstat = opts.esstau = None
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    lib = trm.lib()
    rc = lib.bartrt_mcmc_run_resident(nch, 7, C.c_long(nsteps), p(par), p(pmin), p(pmax), p(step), 3, p(dat), p(unc),
                                      C.cast(C.byref(opts), C.c_void_p), p(out["chain"]), p(out["chisq"]), None,
                                      C.cast(C.byref(nacc), C.c_void_p), C.cast(nbad, C.c_void_p))
    out.update(rc=rc, err=lib.bartrt_last_error().decode() if rc < 0 else "", done=done.value, ngr=made.value,
               naccept=nacc.value, stepsize=step)
    return out


@pytest.mark.parametrize("c", er.CASES, ids=lambda c: c["id"])
def test_probe_is_the_host_build(host, c):
    """bartrt_mcmc_ess on the shared cases (no engine): tau, ess, truncated, the lagged sums and reached are the host
    program's."""
    from bart_amd import sampler
    chain, step, r0, r1, maxlag = er.case(c)
    tau, ess, trunc, acf, reached = sampler.ess(chain, step, r0, r1, maxlag, 10.0)
    h = er.reference(host, c)
    assert acf.shape == h["acf"].shape
    assert er.same(acf, h["acf"]), "lagged sums: %d of %d differ" % (int((acf != h["acf"]).sum()), acf.size)
    assert er.same(tau, h["tau"]) and er.same(ess, h["ess"])
    assert er.same(trunc, h["truncated"]) and reached == bool(h["reached"])


def test_probe_edges():
    from bart_amd import sampler, transit_module as trm
    chain, step, r0, r1, _ = er.case(er.CASES[0])
    tau, ess, trunc, acf, reached = sampler.ess(chain, step, r0, r0 + 3, 2, 0.0)          # fewer than four rows
    assert not tau.any() and not ess.any() and not trunc.any() and not acf.any() and not reached
    with pytest.raises(trm.TransitError, match="maxlag"):
        sampler.ess(chain, step, r0, r1, 4097, 0.0)
    with pytest.raises(trm.TransitError, match="bartrt_mcmc_ess"):
        sampler.ess(chain, step, 0, chain.shape[1] + 1, 0, 0.0)


@pytest.fixture(scope="module")
def history(W):
    """1 024 iterations of five snooker chains with ESS tests and no exit, and the restatements of its four tests:
    (reached-relevant) ess, truncated of ess_restate and R of gr_restate on rows [burnin, grwhen[k])."""
    h = call(W.data, N, esstarget=1.0)
    assert h["rc"] == 0, h["err"]
    free = h["stepsize"] > 0
    h["restated"] = []
    for k in range(h["ngr"]):
        r1 = int(h["grwhen"][k])
        _, ess, trunc, _, _, _ = er.statistic(h["chain"], h["stepsize"], BURNIN, r1, 0, 0.0)
        psrf = gr.statistic(h["chain"], h["stepsize"], BURNIN, r1)[0]
        ok = bool(np.all(np.isfinite(ess[free])) and not trunc[:, free].any())
        h["restated"].append(dict(ess=ess, low=float(ess[free].min()) if ok else -np.inf, top=float(psrf[free].max())))
        print("test %d after %d: ess %s truncated %d R %s" % (k, r1, ess[free].tolist(), int(trunc[:, free].sum()),
                                                               psrf[free].tolist()))
    return h


def reached_at(h, k, target):
    return h["restated"][k]["low"] >= target


def converged_at(h, k, thr):
    top = h["restated"][k]["top"]
    return bool(np.isfinite(top) and top < thr)


def test_records_are_the_probe(W, history):
    from bart_amd import sampler
    h = history
    assert h["done"] == N and h["ngr"] == 4 and h["grwhen"][:4].tolist() == [256, 512, 768, 1024]
    assert not (h["chain"] == SENTINEL).any()
    plain = call(W.data, N)                                           # no ESS work: the same chain
    assert plain["rc"] == 0 and plain["ngr"] == 4 and plain["chain"].tobytes() == h["chain"].tobytes()
    assert plain["grstat"].tobytes() == h["grstat"].tobytes() and (plain["essstat"] == SENTINEL).all()
    free = h["stepsize"] > 0
    for k in range(4):
        tau, ess, trunc, _, _ = sampler.ess(h["chain"], h["stepsize"], BURNIN, int(h["grwhen"][k]), 0, 1.0)
        assert er.same(h["essstat"][k], ess) and er.same(h["esstau"][k], tau), k
        assert er.same(ess, h["restated"][k]["ess"]), k
        assert np.all(h["essstat"][k][~free] == 0.0) and np.all(h["esstau"][k][:, ~free] == 0.0)
    assert (h["essstat"][4:] == SENTINEL).all() and (h["esstau"][4:] == SENTINEL).all()


def test_essexit_stops_at_the_second_test(W, history):
    h = history
    a, b = h["restated"][0]["low"], h["restated"][1]["low"]
    target = max(0.5 * (a + b), 0.5 * b) if np.isfinite(a) else 0.5 * b
    assert reached_at(h, 1, target) and not reached_at(h, 0, target), \
        "seed %d: no target separates the first two tests (%r, %r); take another seed" % (SEED, a, b)
    e = call(W.data, N, esstarget=target, essexit=1)
    stop = int(h["grwhen"][1])
    assert e["rc"] == 0 and e["done"] == stop == 512 and e["ngr"] == 2
    for k in ("chain", "chisq"):
        assert e[k][:, :stop].tobytes() == h[k][:, :stop].tobytes(), k
        assert (e[k][:, stop:] == SENTINEL).all(), k
    assert e["essstat"][:2].tobytes() == h["essstat"][:2].tobytes() and (e["essstat"][2:] == SENTINEL).all()
    assert e["naccept"] == call(W.data, stop)["naccept"]
    never = call(W.data, N, esstarget=1e9, essexit=1)
    assert never["done"] == N and never["chain"].tobytes() == h["chain"].tobytes()


def test_essexit_with_grexit_needs_both(W, history):
    """A threshold the restatement finds met from some test on and a target met from another: the call stops at the
    first test where the restatement finds both, which is neither exit's own first where they differ."""
    h = history
    lows = [r["low"] for r in h["restated"]]
    tops = [r["top"] if np.isfinite(r["top"]) else np.inf for r in h["restated"]]
    # the target the second test reaches, the threshold the third test meets (each as the restatement has them)
    target, thr = 0.5 * lows[1], (1 + 1e-6) * tops[2]
    both = [k for k in range(4) if reached_at(h, k, target) and converged_at(h, k, thr)]
    assert both, "seed %d: no test has both; take another seed" % SEED
    first_ess = min(k for k in range(4) if reached_at(h, k, target))
    first_gr = min(k for k in range(4) if converged_at(h, k, thr))
    print("both exits: ess first reached at test %d, R first met at test %d, both at test %d" % (first_ess, first_gr, both[0]))
    e = call(W.data, N, esstarget=target, essexit=1, grexit=1, grthreshold=thr)
    assert e["rc"] == 0 and e["done"] == int(h["grwhen"][both[0]]) and e["ngr"] == both[0] + 1
    assert e["chain"][:, :e["done"]].tobytes() == h["chain"][:, :e["done"]].tobytes()
    assert (e["chain"][:, e["done"]:] == SENTINEL).all()
    # each exit alone stops at its own first
    assert call(W.data, N, esstarget=target, essexit=1)["done"] == int(h["grwhen"][first_ess])
    assert call(W.data, N, esstarget=target, grexit=1, grthreshold=thr)["done"] == int(h["grwhen"][first_gr])


def test_one_mrw_chain_is_tested(W):
    """One chain: no Gelman-Rubin test is possible, the ESS tests are made all the same."""
    from bart_amd import sampler
    r = call(W.data, N, walk="mrw", nch=1, esstarget=1.0)
    assert r["rc"] == 0 and r["done"] == N and r["ngr"] == 4 and r["grwhen"][:4].tolist() == [256, 512, 768, 1024]
    assert not r["grstat"][:4].any()
    free = r["stepsize"] > 0
    for k in range(4):
        tau, ess, _, _, _ = sampler.ess(r["chain"], r["stepsize"], BURNIN, int(r["grwhen"][k]), 0, 1.0)
        assert er.same(r["essstat"][k], ess) and er.same(r["esstau"][k], tau), k
    assert np.all(r["essstat"][3][free] != 0.0)
    none = call(W.data, N, walk="mrw", nch=1)                        # without esstarget: no test at all, as before
    assert none["rc"] == 0 and none["ngr"] == 0 and none["chain"].tobytes() == r["chain"].tobytes()


def test_resumed_run(W, history):
    from bart_amd import sampler
    h, cut = history, 512
    a = call(W.data, cut, esstarget=1.0)
    b = call(W.data, N - cut, esstarget=1.0, first=cut, start=a["chain"][:, -1])
    assert a["rc"] == b["rc"] == 0 and (a["done"], b["done"]) == (cut, N - cut)
    for k in ("chain", "chisq"):
        assert np.concatenate([a[k], b[k]], axis=1).tobytes() == h[k].tobytes(), k
    assert a["essstat"][:2].tobytes() == h["essstat"][:2].tobytes()
    # the resumed call's tests see its own rows alone
    assert b["ngr"] == 2 and b["grwhen"][:2].tolist() == [768, 1024]
    for k in range(2):
        tau, ess, _, _, _ = sampler.ess(h["chain"], h["stepsize"], cut, int(b["grwhen"][k]), 0, 1.0)
        assert er.same(b["essstat"][k], ess) and er.same(b["esstau"][k], tau), k


def test_refusals_name_the_field(W):
    from bart_amd import sampler, transit_module as trm
    for kw, word in ((dict(esstarget=10.0, grcheck=0), "esstarget"), (dict(esstarget=10.0, maxlag=4097), "maxlag")):
        r = call(W.data, BLOCK, **kw)
        assert r["rc"] == -1 and "mcmc_run_resident" in r["err"] and word in r["err"], r["err"]      # BARTRT_EINVAL
        assert (r["chain"] == SENTINEL).all()
    # the groups call does not serve the fields
    par, pmin, pmax, step, dat, unc, _ = problem(W.data, 5, "snooker", SEED)
    group = sampler.McmcGroup(size=C.sizeof(sampler.McmcGroup), params=par.ctypes.data, pmin=pmin.ctypes.data,
                              pmax=pmax.ctypes.data, stepsize=step.ctypes.data, data=dat.ctypes.data,
                              uncert=unc.ctypes.data, seed=SEED)
    chain, chisq = np.full((1, 5, BLOCK, 7), SENTINEL), np.full((1, 5, BLOCK), SENTINEL)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    lib = trm.lib()
    for kw in (dict(esstarget=10.0, grcheck=BLOCK), dict(maxlag=64), dict(essexit=1)):
        opts = sampler.McmcOptsEss(size=C.sizeof(sampler.McmcOptsEss), thin=1, block=BLOCK, **kw)
        rc = lib.bartrt_mcmc_run_resident_groups(1, C.cast(C.byref(group), C.c_void_p), 5, 7, C.c_long(BLOCK), 3,
                                                 C.cast(C.byref(opts), C.c_void_p), p(chain), p(chisq), None, None,
                                                 None, None)
        err = lib.bartrt_last_error().decode()
        assert rc == -1 and "mcmc_run_resident_groups" in err and "esstarget" in err and "maxlag" in err, err
        assert (chain == SENTINEL).all()
    good = call(W.data, BLOCK, esstarget=10.0)
    assert good["rc"] == 0 and good["ngr"] == 1


def test_run_resident_reports_and_stops(W):
    """sampler.run_resident: essstat / esstau beside grhistory, the ESS line next to every R line and at the end, and
    the stop under essexit (five effective samples: the first test has them)."""
    from bart_amd import sampler
    cfg = T.scfg(W.data, 5, "snooker", seed=SEED, numit=5 * N, burnin=BURNIN, grtest=True, grcheck=BLOCK)
    lines = []
    res = sampler.run_resident(W.worker, cfg, log=lines.append, esstarget=5.0)
    when, psrf = res["grhistory"]
    assert res["done"] == N and when.tolist() == [256, 512, 768, 1024]
    assert res["essstat"].shape == (4, 7) and res["esstau"].shape == (4, 5, 7)
    tau, ess, _, _, _ = sampler.ess(res["chain"], cfg.stepsize, BURNIN, 512, 0, 5.0)
    assert er.same(res["essstat"][1], ess) and er.same(res["esstau"][1], tau)
    free = np.asarray(cfg.stepsize) > 0
    for k, T_k in enumerate(when):
        at = [i for i, l in enumerate(lines) if l.startswith("Gelman-Rubin after %d iterations" % T_k)]
        assert len(at) == 1
        follow = [l for l in lines[at[0] + 1:at[0] + 3] if l.startswith("Effective sample size after %d iterations" % T_k)]
        assert len(follow) == 1 and "smallest: %.1f" % res["essstat"][k][free].min() in follow[0]
    assert lines[-1].startswith("At the end: Effective sample size after 1024 iterations")
    lines = []
    cut = sampler.run_resident(W.worker, cfg, log=lines.append, esstarget=5.0, essexit=True)
    assert cut["done"] == 256 and cut["chain"].tobytes() == res["chain"][:, :256].tobytes()
    assert any(l == "essexit: stopped after 256 of 1024 iterations" for l in lines)
    off = sampler.run_resident(W.worker, cfg)
    assert off["essstat"] is None and off["chain"].tobytes() == res["chain"].tobytes()
    with pytest.raises(ValueError, match="esstarget"):
        sampler.run_resident(W.worker, cfg, essexit=True)


def test_retrieve_ess_target_and_exit(W, tmp_path, capsys):
    """`retrieve --resident --ess-target 5 --ess-exit`: the run stops at the first test and MCMC.log carries the ESS
    lines.  LAST in this module: retrieve.main makes a worker of its own, after which the module's worker is rebuilt."""
    from bart_amd import BARTfunc, retrieve, synthcfg
    sc = T.scfg(W.data, 5, "snooker", seed=SEED)
    line = lambda v: " ".join(repr(float(x)) for x in v)
    case, cfg = synthcfg.make_worker_case(str(tmp_path / "case"), **T.CASE)
    head, tail = open(cfg).read().split("[MCMC]", 1)
    kw = dict(params=line(sc.params), pmin=line(sc.pmin), pmax=line(sc.pmax), stepsize=line(sc.stepsize),
              data=line(sc.data), uncert=line(sc.uncert), nchains="5", numit=str(5 * N), burnin=str(BURNIN),
              walk="snooker", grtest="True", grexit="False", grcheck=str(BLOCK), seed=str(SEED))
    keep = [l for l in tail.split("\n") if l.split("=")[0].strip() not in kw]
    with open(cfg, "w") as f:
        f.write(head + "[MCMC]\n" + "\n".join("%s = %s" % kv for kv in kw.items()) + "\n" + "\n".join(keep))
    W.worker.close()
    W.worker = None
    try:
        out = str(tmp_path / "out")
        os.makedirs(out)
        res = retrieve.main(["-c", cfg, "--resident", "--ess-target", "5", "--ess-exit", "--out", out])
        assert res["done"] == 256 and res["essstat"].shape == (1, 7)
        log = open(os.path.join(out, "MCMC.log")).read()
        assert "Effective sample size after 256 iterations:" in log and "smallest:" in log
        assert "essexit: stopped after 256 of 1024 iterations" in log
        assert "At the end: Effective sample size after 256 iterations:" in log
        for bad in (["--ess-exit"], ["--ess-target", "5"]):                  # (no target; not the resident loop)
            with pytest.raises(SystemExit):
                retrieve.main(["-c", cfg, "--out", out] + bad)
            assert "--ess-target" in capsys.readouterr().err
    finally:
        W.worker = BARTfunc.Worker(W.wcfg)
