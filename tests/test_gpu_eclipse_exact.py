"""Every forced form of the eclipse RT kernels against the exact restatement of the column (tests/eclipse_restate.py:
mpmath at 50 digits, fed the doubles the kernels themselves read -- the walker's layer records, the table values at
their offsets, the rays' 1 / mu, weights and thresholds as the engine holds them) within that module's DERIVED running
error bound, on the checked columns of walker 1; and the ray flags of rule 1's `cut slant` kernel (alive_flags) against
the comparison they stand for.  The oracle stays the reference on all columns (tests/test_gpu_kernel_matrix.py and its
siblings); here the exact value is asserted, |got - exact| <= bound per column, the worst ratio printed per test
(pytest -s; MEASUREMENTS.md has the figures).

The cases come from tests/eclipse_cases.py, which tests/test_eclipse_restate_cpu.py holds to the conditions that make
these tests able to fail.  A column whose cut is undecided (an exact tau within its bound of a ray's threshold) is
compared under both outcomes and must match one.

BARTRT_KERNEL is read once per process: each forced form runs in a child (the one of tests/test_gpu_kernel_matrix.py)
under its own time limit; the records, the rays and the restatement are read and computed once per (case, deck) and
shared by the module.  A child that fails ends its test with the child's output.

Held here: the flux F of every forced form (a), the default choice at 1, 2, 10 and 26 walkers on the clear, jump and
forest walkers (b), the tau / `last` / I_a read-backs (c), the `toomuch` sweep (d), zero extinction (e), the shortest
columns (f), alive_flags.

The whole file takes about 55 s on an MI355X (pytest durations: the first form 14 s with the records' child and the
restatement of 96 (case, deck) pairs, the first form of the other rules 11 s, the read-backs and the sweep 3 - 6 s each,
the rest 0.5 - 3.5 s, nearly all of it mpmath in the parent), measured on this build."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import eclipse_cases as ec
import eclipse_restate as er
import test_gpu_kernel_matrix as km
from test_gpu_parity import forced_kernel

pytestmark = pytest.mark.gpu

ROOT = km.ROOT
CHILD_LIMIT = 300

# the records and rays of every (case, deck): one launch of two walkers with the preparation as a launch of its own
# (BARTRT_FOLD=0: a folded preparation keeps the records in LDS), whatever kernel takes it -- the records do not depend
# on the rule, the cut or the form
REC_CHILD = r"""
import json, pickle, sys
import numpy as np
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
from bart_amd import engine, transit_module as trm
out = []
for case in job["cases"]:
    engine.init(case["tcfg"])
    p = np.load(case["profs"])
    res = {"rays": engine.ray_args(), "wn": trm.get_waveno_arr(trm.get_no_samples()), "rec": []}
    for deck in (0, 1):
        if deck:
            trm.set_cloudtop(case["cloudtop"])
        engine.run_batch(p)
        recs = {}
        for w in case["walkers"]:
            coef, idx, kstop, ok = engine.prep_records(w)
            recs[w] = {"coef": coef, "idx": idx, "kstop": kstop, "ok": ok}
        res["rec"].append(recs)
    trm.free_memory()
    out.append(res)
pickle.dump(out, open(job["out"], "wb"))
"""

# launches of chosen walkers and the read-backs, under the process's own kernel choice: per case and deck, `launches`
# [(rule, cut, [walkers of the batch])] and `reads` [(rule, cut, walker)]
PATH_CHILD = r"""
import json, pickle, sys
import numpy as np
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
from bart_amd import engine, transit_module as trm
out = []
for case in job["cases"]:
    engine.init(case["tcfg"])
    p = np.load(case["profs"])
    A, nw = trm.lib().bartrt_get_nangles(), trm.get_no_samples()
    res = {"launches": [], "reads": []}
    for deck in (0, 1):
        if deck:
            trm.set_cloudtop(case["cloudtop"])
        for rule, cut, batch in case["launches"]:
            trm.set_integ(rule); trm.set_cut(cut)
            engine.walked_begin(); s = engine.run_batch(p[batch]); name = engine.walked_end()[2]
            res["launches"].append({"deck": deck, "rule": rule, "cut": cut, "batch": batch, "spec": s, "name": name,
                                    "restarts": np.array(engine.walked_restarts())})
        for rule, cut, w in case["reads"]:
            trm.set_integ(rule); trm.set_cut(cut)
            engine.run_batch(p)
            engine.walked_begin(); tau, last = engine.get_tau(walker=w); kt = engine.walked_end()[2]
            inten = np.zeros((A, nw))
            engine.walked_begin(); trm.check(trm.lib().bartrt_get_intensity_of(w, trm._ptr(inten), A, nw)); ki = engine.walked_end()[2]
            res["reads"].append({"deck": deck, "rule": rule, "cut": cut, "walker": w, "tau": tau, "last": last, "intens": inten,
                                 "ktau": kt, "kintens": ki})
    trm.free_memory()
    out.append(res)
pickle.dump({"res": out, "rtc": trm.get_rtc_stats()}, open(job["out"], "wb"))
"""


def _child(code, job, tmp, tag, **env):
    jfile = os.path.join(tmp, tag + ".json")
    json.dump(job, open(jfile, "w"))
    r = subprocess.run([sys.executable, "-c", code, jfile], env=km.child_env(**env), capture_output=True, text=True,
                       timeout=CHILD_LIMIT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def _jobcases(cases, **more):
    return [dict(tcfg=c.tcfg, profs=os.path.join(c.dir, "p.npy"), cloudtop=c.cloudtop, walkers=list(getattr(c, "walkers", (1,))),
                 **more) for c in cases]


class Exact:
    """The exact columns of a set of cases: records read once, solutions cached per (case, deck, rule, cut)."""

    def __init__(self, cases, tmp, tag):
        from oracle import rt_oracle as orc
        self.cases = cases
        out = os.path.join(tmp, tag + "_rec.pkl")
        _child(REC_CHILD, {"root": ROOT, "cases": _jobcases(cases), "out": out}, tmp, tag + "_rec", BARTRT_FOLD="0")
        self.cols, self.sol = {}, {}
        for k, (c, res) in enumerate(zip(cases, pickle.load(open(out, "rb")))):
            o = orc.OracleEngine(c.tcfg)
            rays = er.Rays.from_engine(res["rays"])
            assert rays.sq == ((0, 3) if c.grid == 0 else None), (c.dir, res["rays"])
            for deck in (0, 1):
                for w in getattr(c, "walkers", (1,)):
                    rec = dict(res["rec"][deck][w], wn=res["wn"])
                    assert rec["ok"] == 1
                    self.cols[k, deck, w] = ec.device_columns(c, o, rec, rays)

    def outcomes(self, k, deck, rule, cut, w=1):
        key = (k, deck, rule, cut, w)
        if key not in self.sol:
            self.sol[key] = [er.outcomes(self.cols[k, deck, w], n, rule, cut) for n in range(len(self.cases[k].checked))]
        return self.sol[key]

    def check(self, k, deck, rule, cut, spec, worst, what, w=1):
        """spec[W]: the walker's spectrum of the launch; every checked column within its bound of the exact flux."""
        sol = self.outcomes(k, deck, rule, cut, w)
        for n, i in enumerate(self.cases[k].checked):
            ratios = []
            for r in sol[n]:
                d = float(er.absdev(spec[i], r["F"]))
                ratios.append(d / r["dF"] if r["dF"] > 0 else (0.0 if d == 0 else np.inf))
            worst[0] = max(worst[0], min(ratios))
            assert min(ratios) <= 1.0, (what, "column %d" % i, ratios, float(sol[n][0]["F"]), float(spec[i]))

    def check_reads(self, k, rd, worst, what):
        """One read-back (PATH_CHILD): tau against its own bound up to `last` and repeated below it, `last` exactly on
        decided columns, every ray's intensity against ITS OWN bound (a grazing ray does not hide behind its weight).
        `last` under `cut slant`: the deepest layer a ray of the sample reaches."""
        sol = self.outcomes(k, rd["deck"], rd["rule"], rd["cut"], rd["walker"])
        for n, i in enumerate(self.cases[k].checked):
            fits = []
            for r in sol[n]:
                last = max(r["last"])
                ok = int(rd["last"][i]) == last
                rt = 0.0
                for kk in range(last + 1):
                    d = float(er.absdev(rd["tau"][i, kk], r["tau"][kk]))
                    rt = max(rt, d / r["dtau"][kk] if r["dtau"][kk] > 0 else (0.0 if d == 0 else np.inf))
                ri = 0.0
                for a in range(len(r["I"])):
                    d = float(er.absdev(rd["intens"][a, i], r["I"][a]))
                    ri = max(ri, d / r["dI"][a] if r["dI"][a] > 0 else (0.0 if d == 0 else np.inf))
                fits.append((ok and rt <= 1.0 and ri <= 1.0, rt, ri, last))
            best = [f for f in fits if f[0]]
            assert best, (what, "column %d" % i, fits, int(rd["last"][i]))
            worst["tau"], worst["I"] = max(worst["tau"], best[0][1]), max(worst["I"], best[0][2])
            assert np.all(rd["tau"][i, best[0][3]:] == rd["tau"][i, best[0][3]]), (what, i)


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    return {"root": str(tmp_path_factory.mktemp("eclipse_exact")), "sets": {}}


def _set(shared, name, make):
    """-> (cases, Exact, the stand-in for tests/test_gpu_kernel_matrix.py's `matrix`) of a named case set."""
    if name not in shared["sets"]:
        cases = make(os.path.join(shared["root"], name))
        d = os.path.join(shared["root"], name + "_out")
        os.makedirs(d, exist_ok=True)
        shared["sets"][name] = (cases, Exact(cases, d, name), {"cases": cases, "runs": {}, "dir": d})
    return shared["sets"][name]


def _forms(shared, name, make, mode, combos=None):
    """The child of BARTRT_KERNEL=mode (None: the default choice) over a case set, every launch named and checked."""
    cases, exact, matrix = _set(shared, name, make)
    if mode is not None and combos is None:
        got, names = km._run(matrix, mode, False)
        combos = km.FORMS[mode]
    else:
        tag = "%s_%s" % (name, mode or "default")
        job = {"root": ROOT, "combos": combos, "out": os.path.join(matrix["dir"], tag + ".npy"), "cases": _jobcases(cases)}
        out = _child(km.CHILD, job, matrix["dir"], tag, **({"BARTRT_KERNEL": mode} if mode else {}))
        res = json.loads([l for l in out.splitlines() if l.startswith("RESULT")][0][6:])
        assert res["rtc"]["compiled"] == 0 and res["rtc"]["from_disk"] == 0, (mode, res["rtc"])
        got, names = np.load(job["out"]), res["names"]
    worst = [0.0]
    for k, c in enumerate(cases):
        for deck in (0, 1):
            for i, (rule, cut) in enumerate(combos):
                kname = names[k][deck * len(combos) + i]
                what = "%s M, C = %s, grid %d, rule %d, cut %s, deck %d: %s" % (os.path.basename(c.dir), c.mc, c.grid, rule, cut, deck, kname)
                if mode is not None:
                    assert kname.split(" [")[0] == forced_kernel(mode, rule, cut), what
                assert "[instantiated at run time]" not in kname, what
                assert np.all(np.isfinite(got[k, i, deck])), what
                exact.check(k, deck, rule, cut, got[k, i, deck][1], worst, what)
    return worst[0], got, cases


@pytest.mark.parametrize("mode", list(km.FORMS))
def test_every_form_within_the_bound_of_the_exact_flux(shared, mode):
    """a. BARTRT_KERNEL=mode x every (rule, cut) it serves x the 48 cases x without / with a deck."""
    worst, _, _ = _forms(shared, "matrix", ec.matrix_cases, mode)
    print("%s: worst |F - exact| / bound = %.3f" % (mode, worst))


@pytest.mark.parametrize("mode", ["mono_ilp", "adj8"])
def test_zero_extinction(shared, mode):
    """e. Exactly zero extinction in the top band, in a middle band, everywhere, 30 layers: the exact value under the
    degenerate-panel rule; everywhere, without a deck: exactly 0.0.  mono_ilp takes the non-finite fallback, adj8 the in-line selects."""
    combos = [(1, "slant")] if mode == "adj8" else [(1, "slant"), (1, "vertical")]
    worst, got, cases = _forms(shared, "zero", ec.zero_cases, mode, combos=combos)
    for k, c in enumerate(cases):
        if c.tag == "all":        # (with a deck the column ends on its surface term, B sum_a w_a: held by the bound above)
            assert np.all(got[k][:, 0] == 0.0), np.abs(got[k][:, 0]).max()
    print("zero extinction, %s: worst |F - exact| / bound = %.3f" % (mode, worst))


def test_shortest_columns(shared):
    """f. 2 .. 13 and 29 .. 33 layers on one cell, rule 1 with `cut slant`, the default kernel choice."""
    worst, _, _ = _forms(shared, "lengths", ec.length_cases, None, combos=[(1, "slant")])
    print("lengths 2 .. 13, 29 .. 33: worst |F - exact| / bound = %.3f" % worst)


THR = [1e-9, 1e-6, 1e-4, 3e-3, 0.05, 0.3, 0.7, 1.0, 2.0, 5.0, 10.0, 40.0, 300.0, 1e30]


def test_alive_flags_are_the_comparison():
    """alive_flags (csrc/rt_eclipse_s1s.hpp): the flag is exactly tm <= thr for every threshold above 2^-500 and every
    optical depth below 2^400; a threshold that overflows the scaling (1e200) is alive."""
    from bart_amd import engine
    tm, thr = [], []
    for t in THR + [np.nextafter(2.0 ** -500, 1.0), 2.0 ** -499]:
        for m in (t, np.nextafter(t, 0.0), np.nextafter(t, np.inf), 0.0, 2.0 ** 399, t * (1 + 2.0 ** -52), t * (1 - 2.0 ** -52)):
            tm.append(m); thr.append(t)
    tm, thr = np.array(tm), np.array(thr)
    got = engine.alive_flags(tm, thr)
    want = (tm <= thr).astype(float)
    assert np.array_equal(got, want), list(zip(tm[got != want], thr[got != want], got[got != want]))
    # (optical depths inside the stated domain: from 2^424 on the scaled depth overflows too, inf - inf, and the flag is 0)
    over = np.array([0.0, 1.0, 1e100, 2.0 ** 399, np.nextafter(2.0 ** 400, 0.0)])
    assert np.all(engine.alive_flags(over, np.full(5, 1e200)) == 1.0)
    # the selector's argument checks
    from bart_amd import transit_module as trm
    x, out = np.ones(3), np.zeros(3)
    assert trm.lib().bartrt_rt_math(engine.RT_MATH["alive_flags"], trm._ptr(x), trm._ptr(out), 3) == -1
    x, out = np.array([1.0, -1.0]), np.zeros(2)
    assert trm.lib().bartrt_rt_math(engine.RT_MATH["alive_flags"], trm._ptr(x), trm._ptr(out), 2) == -1


# ---- b, c: the default choice across walker counts; the read-backs ----------------------------------------------------
def _path_run(shared, name, make, launches, reads, **env):
    cases, exact, matrix = _set(shared, name, make)
    tag = name + "_path" + "_".join(env.values())
    job = {"root": ROOT, "out": os.path.join(matrix["dir"], tag + ".pkl"), "cases": _jobcases(cases, launches=launches, reads=reads)}
    _child(PATH_CHILD, job, matrix["dir"], tag, **env)
    out = pickle.load(open(job["out"], "rb"))
    return cases, exact, out


@pytest.mark.parametrize("mode", [None, "mono_ilp"])
def test_default_choice_across_walker_counts(shared, mode):
    """b. (The measured table gives these 3 .. 78 columns to the adjacent-rows kernel at every count, so the same
    launches run once more under BARTRT_KERNEL=mono_ilp, the single-wave slant kernel itself, where the jump walker's
    waves must walk twice.)  No BARTRT_KERNEL: 1, 2, 10 and 26 walkers of the clear / jump / forest columns (31 layers x 130 samples) on
    four cells, rule 1 with `cut slant`, without and with the deck: whatever kernel the table names, every walker of
    every batch within the bound -- the single-wave kernel's optimistic, restart and flagged walks among them."""
    launches = [(1, "slant", b) for n in ec.WALKER_COUNTS for b in ec.batch_of(n)]
    cases, exact, out = _path_run(shared, "paths", ec.path_cases, launches, [], **({"BARTRT_KERNEL": mode} if mode else {}))
    assert out["rtc"]["compiled"] == 0 and out["rtc"]["from_disk"] == 0, out["rtc"]
    worst, kernels, restarts = [0.0], set(), 0
    for k, (c, res) in enumerate(zip(cases, out["res"])):
        for ln in res["launches"]:
            what = "%s deck %d, %d walkers: %s" % (os.path.basename(c.dir), ln["deck"], len(ln["batch"]), ln["name"])
            kernels.add((len(ln["batch"]), ln["name"].split("<")[0].split(" [")[0]))
            restarts += int(np.sum(ln["restarts"]))
            assert np.all(np.isfinite(ln["spec"])), what
            for j, w in enumerate(ln["batch"]):
                exact.check(k, ln["deck"], 1, "slant", ln["spec"][j], worst, what + " walker %d (%d)" % (j, w), w=w)
    if mode:
        assert restarts > 0 and {k for _, k in kernels} == {forced_kernel(mode, 1, "slant").split("<")[0]}, (restarts, kernels)
    print("%s: worst |F - exact| / bound = %.3f; second walks %d; kernels %s" % (mode or "default choice", worst[0], restarts, sorted(kernels)))


@pytest.mark.parametrize("name", ["paths", "four"])
def test_optical_depth_last_and_ray_intensities(shared, name):
    """c. engine.get_tau(walker=) and bartrt_get_intensity_of on the four cells: the three path walkers under rule 1 and
    both cuts, and walker 1 of the matrix's cases (both ray orders) under every rule and cut; without and with a deck."""
    if name == "paths":
        make, reads = ec.path_cases, [(1, cut, w) for cut in ("slant", "vertical") for w in (0, 1, 2)]
    else:
        make, reads = (lambda root: ec.matrix_cases(root, cells=ec.FOUR_CELLS)), [(rule, cut, 1) for rule, cut in ec.RULES_CUTS]
    cases, exact, out = _path_run(shared, name, make, [], reads)
    worst, served = {"tau": 0.0, "I": 0.0}, set()
    for k, (c, res) in enumerate(zip(cases, out["res"])):
        for rd in res["reads"]:
            what = "%s deck %d rule %d cut %s walker %d: %s | %s" % (os.path.basename(c.dir), rd["deck"], rd["rule"], rd["cut"], rd["walker"], rd["ktau"], rd["kintens"])
            served.add((rd["rule"], rd["cut"], rd["ktau"].split("<")[0], rd["kintens"].split("<")[0]))
            exact.check_reads(k, rd, worst, what)
    print("%s: worst |tau - exact| / bound = %.3f, |I_a - exact| / bound = %.3f; served by %s" % (name, worst["tau"], worst["I"], sorted(served)))


# ---- d: the toomuch sweep ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mono_ilp", "quad", "adj8"])
def test_toomuch_sweep(shared, mode):
    """d. Thirteen values of toomuch on one 43-layer case, rule 1, both cuts (adj8 serves `cut slant` alone): F within
    the bound; `last` of the read-back (the output launch; a forced form serves none) exactly the exact one on decided
    columns, once per module."""
    combos = [(1, "slant")] if mode == "adj8" else [(1, "slant"), (1, "vertical")]
    worst, _, cases = _forms(shared, "sweep", ec.sweep_cases, mode, combos=combos)
    print("toomuch sweep, %s: worst |F - exact| / bound = %.3f" % (mode, worst))
    if "sweep_last" not in shared:
        cases, exact, out = _path_run(shared, "sweep", ec.sweep_cases, [], [(1, "slant", 1), (1, "vertical", 1)])
        w2 = {"tau": 0.0, "I": 0.0}
        lasts = set()
        for k, (c, res) in enumerate(zip(cases, out["res"])):
            for rd in res["reads"]:
                exact.check_reads(k, rd, w2, "%s deck %d cut %s" % (c.tag, rd["deck"], rd["cut"]))
                lasts |= set(int(x) for x in rd["last"][c.checked])
        shared["sweep_last"] = w2
        assert len(lasts) >= 10, sorted(lasts)
        print("toomuch sweep read-backs: worst tau %.3f, I_a %.3f; distinct `last` %d" % (w2["tau"], w2["I"], len(lasts)))
