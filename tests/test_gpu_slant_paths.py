"""Every build of rule 1's single-wave `cut slant` kernel (csrc/rt_eclipse_s1s.hpp) on every path of its optimistic loop,
with the path each wave must take PREDICTED on the CPU from the oracle's optical depths.

tests/test_gpu_slant_optimistic.py holds the loop's paths on one instantiation, <5, 4, 2, SQ, SCHED 1> at 64 lanes.  The
same template is compiled into many code objects, each with its own register allocation, spills and record read-ahead;
here every one of them walks the same three columns:

  walker 0  "clear"   table molecules at 1e-10: every whole block runs optimistically
  walker 1  "jump"    the table molecules' abundances jump from 1e-10 to 3e-3 on layer 9, position 3 of block 1: a ray
                      dies INSIDE an optimistic block and the wave walks its column a second time
  walker 2  "forest"  a line forest (a tenth of the usual abundances) whose rays die in mid-column, lane by lane on
                      other layers

on 31 layers (five whole six-layer blocks and a masked one) and 130 wavenumbers (three waves, the last partial).

The predictor (predict, below) restates the kernel's rules on the oracle's tau -- block b covers layers 6 b .. 6 b + 5,
block 0 is flagged; a block is entered while 6 b + 5 <= kcut and every lane of the wave has tm <= thr_min * guard; it
fails when some lane has tm > thr_min at its end -- and gives, per walker, the waves that walk twice, and per wave the
optimistic blocks and whether the guard failed before the column's end without a restart (the hand-over).  Every launch's
engine.walked_restarts() must EQUAL the prediction: a guard that is never met, or a restart that comes too often, fails
where bit equality with the guard-off spectra alone would pass.  A prediction is as sharp as tau: sharp() asserts, on the
oracle's numbers alone, that no lane's tm at a block boundary lies within a relative 1e-6 of thr_min or of a guard.

What the predictor confirmed for the cases (on the oracle's numbers, before any launch ran; asserted again in every
test through claims(): optimistic blocks on every walker and in every wave of the clear one, a restart on the jump
walker and none on the clear one, a hand-over -- the guard fails after an optimistic block, whole blocks left, no
restart -- in some wave):
  part 2, all 24 (M, C) x 2 ray orders, guard 2^-4, no deck: walker 0 all four whole blocks optimistic in every wave;
    walker 1 a restart in two or three of its three waves (the last wave holds two wavenumbers: where neither passes
    thr_min inside block 1 the wave hands over at block 2); walker 2 zero to four optimistic blocks, then the hand-over:
    restarts (0, 2 | 3, 0).  Guard 1: walker 1 two or three, walker 2 restarts too in most shapes (0 to 3 waves).  Deck
    between layers 13 and 14 (kend at position 2 of block 2, which walker 0 walks optimistically without it): block 1
    optimistic on every walker, walker 1 restarts, and the deck's surface term follows a second walk
  part 3 (OUT; (4, 2) is a SCHED 1 shape, (4, 4) a SCHED 0 one -- the OUT build itself is SCHED 0): walker 1's
    one-walker launch restarts in three waves, walker 0's in none
  part 4 (EXT, C = 0 and C = 2): optimistic blocks on every walker, restarts on walker 1 (three waves) and, C = 0, one
    on walker 2; hand-overs on walkers 0 and 2.  Lanes far from every line hold exactly zero extinction on the upper
    layers: those waves also take the kernel's ray-by-ray fallback for zero-width panels
  part 5 (A = 1, 6, 7): walker 0 four optimistic blocks, walker 1 two restarts and a hand-over, walker 2 hand-overs
  part 6 (64 / 128 / 256 lanes, 300 wavenumbers, five waves): restarts (0, 5, 0) at 2^-4, (0, 5, 5) at guard 1
  part 7 (prefetched preparation): the (4, 2) case of part 2

Launches run in child processes, one per set of process-wide switches (BARTRT_KERNEL, BARTRT_BLOCK, the run-time
compiler's cache), looping over its cases and guards; the oracle runs in the parent.

Pytest durations on an MI355X, measured on this build (the module: 30 s): part 2, one child per (M, C) inside its first
test: 0.4-0.8 s each, 12 s for the 24; part 3: 0.4 s; part 4: 0.5 s (with the line-by-line oracle in the parent); part 5:
4.2 s, of which the launches are about 0.5 s as in the other children and the rest the three run-time compiles into the
module's cache directory; part 6: 1.3 s for the three children; part 7: 12.7 s, nearly all of it the child's cold
`import torch` and device start-up (run_batch_dev takes torch tensors); every test body itself 0.01-0.2 s."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_kernel_matrix import GRIDS, MC_LIST, child_env
from test_gpu_parity import forced_kernel, many_molecules, walkers
from test_gpu_slant_optimistic import jump_profile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
LBL_RTOL = 1e-7          # tests/test_lbl.py RTOL: the device's Faddeeva function against scipy's
G4 = 2.0 ** -4
KBLK = 6                 # layers per block (rt_eclipse_s1s.hpp kBlk)
NLAYERS, NWAVE, TOOMUCH = 31, 130, 10.0
JUMP = KBLK + 3          # walker 1's extinction jump: position 3 of block 1
DECK = 2 * KBLK + 2      # the deck's layer: position 2 of block 2
SHARP = 1e-6
# 5.5 decades of pressure over 30 intervals: tau grows by about a factor twelve per block, less than 1 / guard, so the forest
# column's waves find their guard failed at a block's START (the hand-over); the jump walker alone passes guard and
# threshold inside one block
PRESS = dict(ptop=1e-5, pbottom=3.0)
CLEAR, JUMPW, FOREST = 0, 1, 2


# ---- the predictor ---------------------------------------------------------------------------------------------------
def thr_min_of(grid, toomuch=TOOMUCH):
    """min_a thr_a, thr_a = the largest tau with tau * (1 / mu_a) <= toomuch (csrc/kernels.hpp slant_thresholds): toomuch *
    mu_a to a few ulp, which sharp() makes irrelevant."""
    return toomuch * float(np.min(np.cos(np.deg2rad(np.asarray(grid, float)))))


def _tm(tau, kend):
    """The running maximum of tau over the layers above [W][L], and kcut."""
    return np.maximum.accumulate(np.maximum(tau, 0.0), axis=1), min(kend, tau.shape[1] - 2)


def predict(tau, kend, thr_min, guard):
    """The path of every 64-lane wave of one walker: tau [W][L] (top-down), the column's last layer kend.
    -> (waves that walk twice, [optimistic blocks per wave], [hand-over per wave])."""
    tm, kcut = _tm(tau, kend)
    nopt, hand, twice = [], [], 0
    for lo in range(0, tau.shape[0], 64):
        t = tm[lo:lo + 64]           # (the lanes past the last wavenumber repeat it)
        b, n, h = 1, 0, False
        while guard > 0.0 and KBLK * b + KBLK - 1 <= kcut:
            if not (t[:, KBLK * b - 1] <= thr_min * guard).all():
                h = True             # the guard failed with whole blocks left: the flagged loop takes over
                break
            n += 1
            if (t[:, KBLK * b + KBLK - 1] > thr_min).any():
                twice += 1           # a ray died inside the block
                break
            b += 1
        nopt.append(n)
        hand.append(h)
    return twice, nopt, hand


def sharp(tau, kend, thr_min, guards):
    """No lane's tm at a block boundary within a relative 1e-6 of thr_min or of a guard."""
    tm, kcut = _tm(tau, kend)
    v = tm[:, np.arange(KBLK - 1, kcut + 1, KBLK)]
    return all((np.abs(v / lim - 1.0) > SHARP).all() for lim in [thr_min] + [thr_min * g for g in guards if g > 0.0])


class Oracle:
    """The oracle's spectra, and its optical depths under a `toomuch` no depth reaches (tau is then nowhere frozen), of one
    case's walkers; exts: per walker, the line-by-line extinction the product hands its kernel (or None)."""

    def __init__(self, tcfg, profs, grid, exts=None):
        from oracle import rt_oracle as orc
        self.o = orc.OracleEngine(tcfg, integ=1, cut="slant")
        self.t = orc.OracleEngine(tcfg, integ=1, cut="slant")
        assert self.o.c.toomuch == TOOMUCH
        self.t.c.toomuch = 1e300
        self.profs, self.exts, self.thr_min = profs, exts, thr_min_of(grid)
        self.L = self.o.L

    def deck(self, logp):
        self.o.set_cloudtop(logp)
        self.t.set_cloudtop(logp)

    def kend(self):
        c = self.o.c
        if not c.has_cloud:
            return self.L - 1
        k = [k for k in range(self.L) if self.o.press[self.L - 1 - k] >= c.cloudtop]
        return k[0] if k else self.L - 1

    def _each(self, eng, fn):
        out = []
        for w, p in enumerate(self.profs):
            if self.exts is not None:
                eng.set_extra_extinction(self.exts[w])
            out.append(fn(eng, p))
        return out

    def spectra(self):
        return np.stack(self._each(self.o, lambda e, p: e.run(p)))

    def paths(self, guards):
        """{guard: ([restarts per walker], [[optimistic blocks per wave] per walker], [[hand-over per wave] per walker])};
        asserts the predictions sharp."""
        taus = self._each(self.t, lambda e, p: e.run(p, want_tau=True)[1])
        kend, res = self.kend(), {}
        for w, tau in enumerate(taus):
            assert sharp(tau, kend, self.thr_min, guards), "walker %d: a block boundary within 1e-6 of a limit" % w
        for g in guards:
            pr = [predict(tau, kend, self.thr_min, g) for tau in taus]
            res[g] = (np.array([p[0] for p in pr]), [p[1] for p in pr], [p[2] for p in pr])
        return res


def claims(paths, deck=False):
    """What a three-walker case is there for, on the predictor's word (guard 2^-4): optimistic blocks on the clear walker
    (every wave), a restart on the jump walker (every wave), none on the clear one; without a deck, a hand-over."""
    twice, nopt, hand = paths[G4]
    assert min(nopt[CLEAR]) >= 1 and twice[CLEAR] == 0, (nopt[CLEAR], twice)
    assert twice[JUMPW] >= 1, twice
    assert all(sum(n) >= 1 for n in nopt), nopt               # optimistic blocks: on every walker
    if not deck:
        assert any(h and n >= 1 for w in (CLEAR, JUMPW, FOREST) for h, n in zip(hand[w], nopt[w])), hand
    assert not paths[0.0][0].any()


def deck_logp(case):
    """log10 of a pressure (bar) between layers DECK - 1 and DECK from the top: kend = DECK."""
    L = len(case.press_bar)
    return float(0.5 * (np.log10(case.press_bar[L - DECK]) + np.log10(case.press_bar[L - 1 - DECK])))


def three_walkers(case, seed):
    profs = walkers(case, 3, seed=seed)
    profs[CLEAR] = jump_profile(case, profs[CLEAR], len(case.press_bar))     # (no layer lies below the jump: 1e-10 throughout)
    profs[JUMPW] = jump_profile(case, profs[JUMPW], JUMP)
    # the forest a tenth as strong: its strongest lanes stand below the guard when block 1 begins
    S, L = len(case.species), len(case.press_bar)
    f = profs[FOREST].reshape(S + 1, L)       # (a view)
    f[3:] *= 0.1
    q = 1.0 - f[3:].sum(0)
    f[1], f[2] = 0.15 * q, 0.85 * q            # He, H2
    return profs


def table_case(d, M, C, grid, nwave=NWAVE, seed=None):
    from bart_amd import synth
    keys = {"cia_interp": "linear"} if C == 1 else None
    c = synth.make_case(d, nlayers=NLAYERS, nwave=nwave, raygrid=grid, toomuch=TOOMUCH, cia={0: False, 1: 1, 2: 1, 4: 2}[C],
                        tlow=400.0, thigh=3000.0, tempdelt=650.0, extra_keys=keys, **PRESS, **many_molecules(M))
    profs = three_walkers(c, 10 * M + C if seed is None else seed)
    np.save(os.path.join(d, "p.npy"), profs)
    return c, profs


# ---- the children ----------------------------------------------------------------------------------------------------
CHILD = r"""
import json, sys
import numpy as np
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
from bart_amd import engine, transit_module as trm
out = {}
def launch(key, fn):
    engine.walked_begin(); s = fn(); name = engine.walked_end()[2]
    out[key + "/spec"] = s; out[key + "/restarts"] = engine.walked_restarts(); out[key + "/kernel"] = np.array(name)
for case in job["cases"]:
    p = np.load(case["profs"])
    n = case["name"]
    engine.init(case["tcfg"])
    for deck in case["decks"]:                       # (None first: a deck stays)
        if deck is not None:
            trm.set_cloudtop(deck)
        for g in case["guards"]:
            trm.set_slant_opt(g)
            launch("%s/%s/%r" % (n, "plain" if deck is None else "deck", g), lambda: engine.run_batch(p))
            for w in case.get("out", []):            # the one-walker launches with the tau / intensity outputs
                engine.run_batch(p)
                A, nw = trm.lib().bartrt_get_nangles(), trm.get_no_samples()
                key = "%s/out%d/%r" % (n, w, g)
                engine.walked_begin(); tau, last = engine.get_tau(walker=w); name = engine.walked_end()[2]
                out[key + "/tau"] = tau; out[key + "/last"] = last; out[key + "/kernel"] = np.array(name)
                out[key + "/restarts"] = engine.walked_restarts()
                inten = np.zeros((A, nw))
                engine.walked_begin(); trm.check(trm.lib().bartrt_get_intensity_of(w, trm._ptr(inten), A, nw))
                out[key + "/ikernel"] = np.array(engine.walked_end()[2]); out[key + "/irestarts"] = engine.walked_restarts()
                out[key + "/intens"] = inten
    if case.get("prefetch"):                         # a launch that carries the next batch's preparation, then that batch
        import torch
        trm.set_slant_opt(case["guards"][-1])
        d = torch.from_numpy(p).cuda()
        a, b = d[case["prefetch"]].contiguous(), d.contiguous()
        launch(n + "/head", lambda: engine.run_batch_dev(a, next_prof=b).cpu().numpy())
        launch(n + "/next", lambda: engine.run_batch_dev(b).cpu().numpy())
        launch(n + "/own", lambda: engine.run_batch(p[case["prefetch"]]))
    trm.free_memory()
np.savez(job["out"], **out)
print("RESULT" + json.dumps({"rtc": trm.get_rtc_stats()}))
"""


def run_child(d, cases, **env):
    """cases: [{name, tcfg, profs, decks, guards, ...}] in one child under `env` -> (its arrays, its run-time-compile record)."""
    job = {"root": ROOT, "cases": cases, "out": os.path.join(d, "out.npz")}
    json.dump(job, open(os.path.join(d, "job.json"), "w"))
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(d, "job.json")], env=child_env(**env), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, "the child ended with %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-4000:]
    rtc = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])["rtc"]
    return np.load(job["out"]), rtc


def job_of(name, c, guards, decks=(None,), **more):
    return dict(name=name, tcfg=c.tcfg, profs=os.path.join(c.dir, "p.npy"), guards=list(guards), decks=list(decks), **more)


def held(out, key, guards, ref, paths, kernel, rtol=RTOL, atol=1e-12):
    """The launches out[key/guard/...]: the kernel asked for; guard off: no restart; guard on: the guard-off bits, the
    oracle's numbers, and the restarts predicted."""
    off = out["%s/%r/spec" % (key, 0.0)]
    assert np.isfinite(off).all() and (off != 0.0).any()
    for g in guards:
        k = "%s/%r" % (key, g)
        assert str(out[k + "/kernel"]).split(" [")[0] == kernel, (k, str(out[k + "/kernel"]))
        print(k, "restarts", out[k + "/restarts"], "predicted", paths[g][0], "optimistic blocks", paths[g][1])
        assert np.array_equal(out[k + "/restarts"], paths[g][0]), (k, out[k + "/restarts"], paths[g][0])
        assert np.array_equal(out[k + "/spec"], off), (k, np.abs(out[k + "/spec"] - off).max())
        np.testing.assert_allclose(out[k + "/spec"], ref, rtol=rtol, atol=atol * np.abs(ref).max(), err_msg=k)


# ---- part 2: every five-angle ahead-of-time cell, both ray orders ---------------------------------------------------------
GUARDS = (0.0, G4, 1.0)


@pytest.fixture(scope="module")
def cells(tmp_path_factory):
    """(M, C) -> the pair's child, run on first use: both ray orders, without and with the deck, guards 0, 2^-4 and 1."""
    done = {}

    def get(M, C):
        if (M, C) not in done:
            d = str(tmp_path_factory.mktemp("mc%d_%d" % (M, C)))
            cases, jobs = [], []
            for g, grid in enumerate(GRIDS):
                c, profs = table_case(os.path.join(d, "g%d" % g), M, C, grid)
                cases.append((c, profs, grid))
                jobs.append(job_of("g%d" % g, c, GUARDS, (None, deck_logp(c))))
            done[M, C] = (cases, run_child(d, jobs, BARTRT_KERNEL="mono_ilp"))
        return done[M, C]
    return get


@pytest.mark.parametrize("g", (0, 1), ids=("sq", "nosq"))
@pytest.mark.parametrize("M,C", MC_LIST, ids=["M%d_C%d" % mc for mc in MC_LIST])
def test_every_aot_cell_takes_the_predicted_paths(cells, M, C, g):
    """<5, M, C, SQ, slant_sched(M, C)> of the ahead-of-time set (SQ: the ray grid with the 0 / 60 degree pair), forced by
    BARTRT_KERNEL=mono_ilp: guards 2^-4 and 1 give the bits of guard 0 and the oracle's numbers, and every walker's
    restarts are the predicted ones -- without a deck and with one in the middle of a block."""
    cases, (out, rtc) = cells(M, C)
    c, profs, grid = cases[g]
    assert rtc["compiled"] == 0 and rtc["from_disk"] == 0, rtc
    o = Oracle(c.tcfg, profs, grid)
    for deck in (False, True):
        if deck:
            o.deck(deck_logp(c))
            assert o.kend() == DECK
        paths = o.paths(GUARDS)
        claims(paths, deck)
        if deck:    # the block the deck cuts is one the clear walker walks optimistically without it
            assert min(plain[G4][1][CLEAR]) >= 2 and max(paths[G4][1][CLEAR]) == 1
        plain = paths
        assert paths[1.0][0][JUMPW] >= 1             # (guard 1: the check at the block's end is the only protection)
        held(out, "g%d/%s" % (g, "deck" if deck else "plain"), GUARDS, o.spectra(), paths, forced_kernel("mono_ilp", 1, "slant"))
    assert not np.allclose(out["g%d/plain/0.0/spec" % g], out["g%d/deck/0.0/spec" % g])      # the deck is reached


# ---- part 3: the build with the optical-depth / intensity outputs ----------------------------------------------------------
OUT_KERNEL = "rt_eclipse_simpson_slant (with optical-depth / intensity outputs)"


@pytest.fixture(scope="module")
def out_runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("out"))
    cases = {mc: table_case(os.path.join(d, "mc%d_%d" % mc), mc[0], mc[1], GRIDS[0]) for mc in ((4, 2), (4, 4))}
    jobs = [job_of("mc%d_%d" % mc, c, (0.0, G4), out=[CLEAR, JUMPW]) for mc, (c, _) in cases.items()]
    return cases, run_child(d, jobs)      # (the default kernel choice: a forced form serves no output launch)


@pytest.mark.parametrize("M,C", [(4, 2), (4, 4)], ids=["OUT_M4_C2_sched1", "OUT_M4_C4_sched0"])
def test_outputs_of_a_wave_that_walked_twice(out_runs, M, C):
    """<5, M, C, false, 0, false, OUT = true> writes tau, last and the per-ray intensities DURING the walk, so a wave
    that walks twice writes them twice.  The jump walker's launch restarts in every wave, the clear walker's in none:
    the same bits as with the guard off, the oracle's values, `last` exactly, and the layers past `last` repeat tau[last]."""
    cases, (out, rtc) = out_runs
    c, profs = cases[M, C]
    o = Oracle(c.tcfg, profs, GRIDS[0])
    paths = o.paths((0.0, G4))
    claims(paths)
    name = "mc%d_%d" % (M, C)
    for w in (CLEAR, JUMPW):
        off = {k: out["%s/out%d/%r/%s" % (name, w, 0.0, k)] for k in ("tau", "last", "intens")}
        _, rtau, rlast = o.o.run(profs[w], want_tau=True)
        rint = o.o.intensity(profs[w])
        for g in (0.0, G4):
            key = "%s/out%d/%r/" % (name, w, g)
            tau, last, inten = out[key + "tau"], out[key + "last"], out[key + "intens"]
            for k in ("kernel", "ikernel"):
                assert str(out[key + k]).split(" [")[0] == OUT_KERNEL, (key, str(out[key + k]))
            for k in ("restarts", "irestarts"):      # (a launch of this one walker)
                print(key + k, out[key + k], "predicted", paths[g][0][w])
                assert np.array_equal(out[key + k], paths[g][0][w:w + 1]), (key + k, out[key + k], paths[g][0][w])
            assert np.array_equal(tau, off["tau"]) and np.array_equal(last, off["last"]) and np.array_equal(inten, off["intens"]), key
            assert np.array_equal(last, rlast), key
            np.testing.assert_allclose(tau, rtau, rtol=RTOL, atol=1e-300, err_msg=key)
            np.testing.assert_allclose(inten, rint, rtol=RTOL, atol=1e-12 * np.abs(rint).max(), err_msg=key)
            assert w == CLEAR or (last < NLAYERS - 1).any()      # (the jump walker's columns end above the bottom)
            for i in range(tau.shape[0]):
                assert (tau[i, last[i]:] == tau[i, last[i]]).all(), (key, i)


# ---- part 4: the line-by-line extinction hand-off ----------------------------------------------------------------------------
EXT_KERNEL = "single-wave `cut slant` kernel (line-by-line extinction)"


@pytest.fixture(scope="module")
def ext_runs(tmp_path_factory):
    from bart_amd import synth_lbl
    from oracle import lbl_oracle
    d = str(tmp_path_factory.mktemp("ext"))
    cases, jobs = {}, []
    for cia in (0, 1):
        c = synth_lbl.make_lbl_case(os.path.join(d, "cia%d" % cia), nlines=400, nwave=NWAVE, nlayers=NLAYERS, cia=cia or False,
                                    toomuch=TOOMUCH, **EXT_PRESS)
        profs = three_walkers(c, 40 + cia)
        np.save(os.path.join(c.dir, "p.npy"), profs)
        lo = lbl_oracle.LblOracle(c.tcfg)
        cases[cia] = (c, profs, [lo.extinction(p.reshape(len(c.species) + 1, -1)) for p in profs])
        jobs.append(job_of("cia%d" % cia, c, (0.0, G4)))
    return cases, run_child(d, jobs, BARTRT_KERNEL="mono_ilp")


# (the lines are far weaker than the table's forest: the column reaches deeper before a ray dies)
EXT_PRESS = dict(ptop=1e-4, pbottom=100.0)


@pytest.mark.parametrize("cia", (0, 1), ids=["EXT_C0", "EXT_C2"])
def test_line_by_line_hand_off_takes_the_predicted_paths(ext_runs, cia):
    """<5, 0, C, SQ, 1, EXT = true>: the extinction of a line list as one more load per layer, without a cross-section
    file (C = 0) and with one under the spline (C = 2).  BARTRT_KERNEL does not reach this launch (rt_launch.hpp
    launch_rt_spec takes the hand-off before it looks at the forced form), so the kernel is asserted by its name alone.
    The oracle is given its own line-by-line extinction; tolerance: tests/test_lbl.py's for this comparison."""
    cases, (out, rtc) = ext_runs
    c, profs, exts = cases[cia]
    assert rtc["compiled"] == 0, rtc
    o = Oracle(c.tcfg, profs, GRIDS[0], exts=exts)
    paths = o.paths((0.0, G4))
    claims(paths)
    held(out, "cia%d/plain" % cia, (0.0, G4), o.spectra(), paths, EXT_KERNEL, rtol=LBL_RTOL, atol=0.0)


# ---- part 5: other ray-grid sizes (instantiated at run time) -----------------------------------------------------------------
ANGLES = {1: (35.0,), 6: tuple(np.round(np.linspace(0.0, 84.0, 6), 3)), 7: tuple(np.round(np.linspace(0.0, 84.0, 7), 3))}


@pytest.fixture(scope="module")
def angle_runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("angles"))
    cases = {A: table_case(os.path.join(d, "a%d" % A), 4, 2, grid, seed=50 + A) for A, grid in ANGLES.items()}
    jobs = [job_of("a%d" % A, c, (0.0, G4)) for A, (c, _) in cases.items()]
    return cases, run_child(d, jobs, BARTRT_KERNEL="mono_ilp", BARTRT_RTC_CACHE=os.path.join(d, "cache"))


@pytest.mark.parametrize("A", list(ANGLES), ids=["A%d" % a for a in ANGLES])
def test_other_ray_grid_sizes_take_the_predicted_paths(angle_runs, A):
    """<A, 4, 2, false, SCHED>: one angle (thr_min == thr_max), six (the widest SCHED 1), seven (the first SCHED 0)."""
    cases, (out, rtc) = angle_runs
    c, profs = cases[A]
    assert rtc["failed"] == 0 and rtc["compiled"] + rtc["from_disk"] >= len(ANGLES), rtc
    o = Oracle(c.tcfg, profs, ANGLES[A])
    paths = o.paths((0.0, G4))
    claims(paths)
    assert "[instantiated at run time]" in str(out["a%d/plain/%r/kernel" % (A, G4)])
    held(out, "a%d/plain" % A, (0.0, G4), o.spectra(), paths, "rt_eclipse_simpson_slant (ray grid of another size)")


# ---- part 6: lanes per workgroup ------------------------------------------------------------------------------------------
NWAVE_BLOCK = 300        # 256 lanes: two tiles, the second partial (and three of its four waves past the last wavenumber)
BLOCK_CASES = [(M, C, g) for M, C in ((4, 2), (4, 4)) for g in (0, 1)]


@pytest.fixture(scope="module")
def block_runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("block"))
    cases = {k: table_case(os.path.join(d, "mc%d_%d_g%d" % k), k[0], k[1], GRIDS[k[2]], nwave=NWAVE_BLOCK) for k in BLOCK_CASES}
    jobs = [job_of("mc%d_%d_g%d" % k, c, GUARDS) for k, (c, _) in cases.items()]
    runs = {}
    for block in (64, 128, 256):
        os.mkdir(os.path.join(d, str(block)))
        runs[block] = run_child(os.path.join(d, str(block)), jobs, BARTRT_KERNEL="mono_ilp", BARTRT_BLOCK=str(block))
    return cases, runs


@pytest.mark.parametrize("block", (64, 128, 256), ids=lambda b: "block%d" % b)
@pytest.mark.parametrize("M,C,g", BLOCK_CASES, ids=["M%d_C%d_%s" % (M, C, ("sq", "nosq")[g]) for M, C, g in BLOCK_CASES])
def test_lanes_per_workgroup_change_nothing(block_runs, M, C, g, block):
    """BARTRT_BLOCK=128 / 256: the event log's addressing and the restart count follow the workgroup's size; a wave
    decides alone, so the spectra and every walker's restarts are those of one wave per workgroup -- the predicted ones."""
    cases, runs = block_runs
    c, profs = cases[M, C, g]
    out, rtc = runs[block]
    assert rtc["compiled"] == 0 and rtc["from_disk"] == 0, rtc
    o = Oracle(c.tcfg, profs, GRIDS[g])
    paths = o.paths(GUARDS)
    claims(paths)
    name = "mc%d_%d_g%d/plain" % (M, C, g)
    held(out, name, GUARDS, o.spectra(), paths, forced_kernel("mono_ilp", 1, "slant"))
    for gd in GUARDS:
        for k in ("spec", "restarts"):
            assert np.array_equal(out["%s/%r/%s" % (name, gd, k)], runs[64][0]["%s/%r/%s" % (name, gd, k)]), (block, gd, k)


# ---- part 7: a launch that carries the next batch's preparation ---------------------------------------------------------
@pytest.fixture(scope="module")
def prefetch_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("prefetch"))
    c, profs = table_case(os.path.join(d, "c"), 4, 2, GRIDS[0])
    return c, profs, run_child(d, [job_of("pf", c, (0.0, G4), prefetch=[CLEAR, FOREST])], BARTRT_KERNEL="mono_ilp")


def test_a_launch_that_prepares_the_next_batch(prefetch_run):
    """run_batch_dev(a, next_prof=b): the head of a's grid prepares b's layer records (nprep > 0, the walk's block ids
    shifted), and b's launch -- the jump walker's -- reads them: run_batch's bits both times, the predicted restarts."""
    c, profs, (out, rtc) = prefetch_run
    assert rtc["compiled"] == 0 and rtc["from_disk"] == 0, rtc
    o = Oracle(c.tcfg, profs, GRIDS[0])
    paths = o.paths((0.0, G4))
    claims(paths)
    held(out, "pf/plain", (0.0, G4), o.spectra(), paths, forced_kernel("mono_ilp", 1, "slant"))
    for k in ("head", "next", "own"):
        assert str(out["pf/%s/kernel" % k]).split(" [")[0] == forced_kernel("mono_ilp", 1, "slant"), str(out["pf/%s/kernel" % k])
    assert np.array_equal(out["pf/head/spec"], out["pf/own/spec"])
    assert np.array_equal(out["pf/head/spec"], out["pf/plain/%r/spec" % G4][[CLEAR, FOREST]])
    assert np.array_equal(out["pf/next/spec"], out["pf/plain/%r/spec" % G4])
    want = paths[G4][0]
    print("restarts head", out["pf/head/restarts"], "next", out["pf/next/restarts"], "predicted", want)
    assert np.array_equal(out["pf/head/restarts"], want[[CLEAR, FOREST]]) and np.array_equal(out["pf/own/restarts"], want[[CLEAR, FOREST]])
    assert np.array_equal(out["pf/next/restarts"], want) and want[JUMPW] > 0
