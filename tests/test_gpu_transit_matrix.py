"""Every instantiation of the transit-geometry kernels (csrc/transit_geom.hip) against the oracle (oracle/rt_oracle.c
column_transit) on all columns, and against the exact restatement of the column (tests/transit_restate.py: mpmath at
50 digits, fed the doubles the kernel itself reads -- its layer records, the table values at their offsets, its
radii) within that module's DERIVED running error bound on the checked columns of walker 1.

rt_transit_mfma<M, C, KT> is built for the 24 (table molecules, CIA slots) pairs of BARTRT_MC_LIST x three depths (KT
= 8, 16, 20 row tiles of 16 chords: up to 128, 256, 320 layers).  One small case per pair and depth: 37 / 150 / 260
layers (a partial last tile in each), 70 samples (one full 64-sample workgroup, one with a partial wave and three
waves that return at once), two walkers, `toomuch 1`, without and with a cloud deck in the middle of the column,
without and with `transparent`.  The same cells run through the scalar kernel (BARTRT_KERNEL=generic), which also has
the optical-depth output: its tau and `last` are held to the exact ones.  The `toomuch` sweep puts the cut on every
one of the 16 row positions and on every row tile (tests/test_transit_restate_cpu.py checks that on the oracle);
zero extinction, the shortest columns and the chord table (bartrt_get_chord_table) have tests of their own.

BARTRT_KERNEL is read once per process: each forced form runs in a child that loops over the cases and reports the
kernel every launch took; the oracle and the restatement run in the parent.  The cases come from tests/transit_cases.py,
which tests/test_transit_restate_cpu.py holds to the conditions that make these tests able to fail.

No column is skipped: a chord within 1000 bounds of `toomuch` is an AssertionError (a condition on the inputs).
Every test prints its worst |device - exact| / bound before asserting it (pytest -s); MEASUREMENTS.md has the figures.

The whole file takes about 31 s on an MI355X (pytest durations: the line-by-line form 5.5 s, 260 layers 4.6 s, the rest
0.5 - 3 s each, most of it mpmath in the parent), measured on this build."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import transit_cases as tc
import transit_restate as tr
from test_gpu_kernel_matrix import child_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
MFMA, SCALAR, MFMA_EXT = "rt_transit_mfma", "rt_transit", "rt_transit_mfma (line-by-line extinction)"

CHILD = r"""
import json, pickle, sys
import numpy as np
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
from bart_amd import engine, transit_module as trm
out = []
for case in job["cases"]:
    p, res = np.load(case["profs"]), []
    for tcfg, deck, _ in case["variants"]:
        engine.init(tcfg)
        if deck is not None:
            trm.set_cloudtop(deck)
        engine.walked_begin(); spec = engine.run_batch(p); name = engine.walked_end()[2]
        r = {"spec": spec, "name": name}
        if case["exact"]:
            coef, idx, kstop, ok = engine.prep_records(1)
            r.update(coef=coef, idx=idx, kstop=kstop, ok=ok, rtop=engine.chord_table(1)[0],
                     wn=trm.get_waveno_arr(trm.get_no_samples()))
            if case["lbl"]:
                r["ext"] = engine.lbl_extinction(p[1])
        if case["tau"]:
            r["tau"], r["last"] = engine.get_tau(1)      # (walker 1 again, as a batch of one with the depth output)
        trm.free_memory()
        res.append(r)
    out.append(res)
pickle.dump({"res": out, "rtc": trm.get_rtc_stats()}, open(job["out"], "wb"))
"""


def run_child(tmp, tag, cases, mode=None, tau=False, lbl=False):
    """The cases' variants in a child under BARTRT_KERNEL=mode (None: the default choice) -> res[case][variant]."""
    tmp = str(tmp)
    jc = []
    for n, c in enumerate(cases):
        pf = os.path.join(c.dir, "p.npy")
        np.save(pf, c.profs)
        jc.append({"profs": pf, "variants": c.variants, "exact": bool(c.checked) and tc.exact_here(c), "tau": tau, "lbl": lbl})
    job = {"root": ROOT, "cases": jc, "out": os.path.join(tmp, tag + ".pkl")}
    jfile = os.path.join(tmp, tag + ".json")
    json.dump(job, open(jfile, "w"))
    r = subprocess.run([sys.executable, "-c", CHILD, jfile], env=child_env(**({"BARTRT_KERNEL": mode} if mode else {})),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = pickle.load(open(job["out"], "rb"))
    # the ahead-of-time set served every launch: no kernel was compiled or loaded at run time
    assert out["rtc"]["compiled"] == 0 and out["rtc"]["from_disk"] == 0, out["rtc"]
    return out["res"]


def oracle_of(c, variant, ext=None):
    from oracle import rt_oracle as orc
    tcfg, deck, transparent = variant
    o = orc.OracleEngine(tcfg)
    assert o.c.solution == 1 and bool(o.c.transparent) == bool(transparent)
    if deck is not None:
        o.set_cloudtop(deck)
    return o


def exact_column(c, o, r, ext=None, exp_rt=False):
    """The exact column of what the device read for walker 1 on the case's checked columns."""
    cf, v, allow = tr.table_inputs(o, r["coef"], r["idx"], c.checked, wn=r["wn"])
    e, de, A = tr.extinction(cf, v, allow, None if ext is None else ext[::-1][:, c.checked])
    ch = c.__dict__.setdefault("_chords", {})
    key = r["rtop"].tobytes()
    if key not in ch:
        ch[key] = tr.Chords(r["rtop"])
    col = tr.columns(e, de, A, ch[key], tr.kend_of(r["kstop"]), o.c.toomuch, o.c.transparent, o.c.starrad, exp_rt=exp_rt)
    assert tr.undecided(col) == [], (c.dir, "a chord within 1000 bounds of toomuch: change the case's inputs")
    return col


def check(c, res, kernel, worst, refs=None, lbl_oracle=None):
    """One case's variants: the kernel's name, all columns against the oracle, the checked columns of walker 1 against
    the exact value.  worst: the running maxima of error / bound."""
    rt2 = None
    for n, (v, r) in enumerate(zip(c.variants, res)):
        what = "%s M, C = %s, L = %d, deck %s, transparent %d: %s" % (os.path.basename(v[0]), c.mc, len(c.press_bar), v[1], v[2], r["name"])
        assert r["name"] == kernel, what
        o = oracle_of(c, v)
        if refs is not None and n in refs:
            ref = refs[n]
        elif lbl_oracle is not None:
            ref = []
            for p in c.profs:
                o.set_extra_extinction(lbl_oracle.extinction(p.reshape(len(c.species) + 1, -1)))
                ref.append(o.run(p))
            ref = np.array(ref)
        else:
            ref = o.run_batch(c.profs)
        if refs is not None:
            refs[n] = ref
        assert np.all(np.isfinite(r["spec"])), what
        rt2 = (o.extinction(c.profs[0])[1].max() / o.c.starrad) ** 2 if rt2 is None else rt2
        rtol = 1e-9 if lbl_oracle is not None else RTOL
        np.testing.assert_allclose(r["spec"], ref, rtol=rtol, atol=rtol * rt2 if v[2] else 0.0, err_msg=what)
        if "coef" not in r:
            continue
        assert r["ok"] == 1
        col = exact_column(c, o, r, r.get("ext"), exp_rt=kernel != SCALAR)
        ratio = tr.absdev(r["spec"][1, c.checked], col.M) / col.dM
        worst["M"] = max(worst["M"], ratio.max())
        assert np.all(ratio <= 1.0), (what, ratio)
        if tr.kend_of(r["kstop"]) == 0 and v[2]:
            assert np.all(r["spec"] == 0.0), what           # nothing below the top: r_top^2 - 0 - r_top^2
        if "tau" in r:
            assert np.array_equal(r["last"][c.checked], col.last), what
            for m, i in enumerate(c.checked):
                k = int(col.last[m]) + 1
                dev = tr.absdev(r["tau"][i, :k], col.tau[:k, m])
                assert dev[0] == 0.0
                assert np.all(dev[1:] <= col.dtau[1:k, m]), (what, i)
                nz = dev[1:] > 0
                if nz.any():
                    worst["tau"] = max(worst["tau"], (dev[1:][nz] / col.dtau[1:k, m][nz]).max())
                assert np.all(r["tau"][i, k:] == r["tau"][i, k - 1]), (what, i)


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    """The oracle's spectra per (case dir, variant): computed once, shared by the matrix-tile and the scalar runs."""
    return {"root": str(tmp_path_factory.mktemp("transit_matrix")), "refs": {}, "cases": {}, "named": set()}


def _cases(shared, key, make):
    if key not in shared["cases"]:
        shared["cases"][key] = make()
    return shared["cases"][key]


@pytest.mark.parametrize("L", tc.DEPTHS)
def test_every_table_cell_at_every_depth(shared, tmp_path, L):
    """rt_transit_mfma<M, C, KT>: 24 cells x {8, 16, 20} row tiles; deck x transparent."""
    cases = _cases(shared, "L%d" % L, lambda: tc.matrix_cases(shared["root"], L))
    res = run_child(tmp_path, "mfma%d" % L, cases)
    worst = {"M": 0.0, "tau": 0.0}
    for c, rs in zip(cases, res):
        check(c, rs, MFMA, worst, shared["refs"].setdefault(c.dir, {}))
        shared["named"].add((c.mc, (L + 127) // 128 if L <= 256 else 3))
        assert not np.allclose(rs[0]["spec"], rs[1]["spec"]) and not np.allclose(rs[0]["spec"], rs[2]["spec"])
    print("matrix tiles, L = %d: worst |M - exact| / bound = %.3f" % (L, worst["M"]))
    # every table cell of this depth was launched and named
    assert {mc for mc, d in shared["named"] if d == ((L + 127) // 128 if L <= 256 else 3)} == set(tc.MC_LIST)


def test_the_same_cells_through_the_scalar_kernel(shared, tmp_path):
    """BARTRT_KERNEL=generic at 37 layers, with the optical-depth output: tau and `last` against the exact ones.
    Cells off the ahead-of-time list (seven and eight molecules, three CIA tables) take it by default."""
    cases = _cases(shared, "L37", lambda: tc.matrix_cases(shared["root"], 37))
    worst = {"M": 0.0, "tau": 0.0}
    for c, rs in zip(cases, run_child(tmp_path, "generic", cases, mode="generic", tau=True)):
        check(c, rs, SCALAR, worst, shared["refs"].setdefault(c.dir, {}))
    off = tc.off_list_cases(shared["root"])
    for c, rs in zip(off, run_child(tmp_path, "off", off, tau=True)):
        check(c, rs, SCALAR, worst)
    print("scalar kernel: worst |M - exact| / bound = %.3f, |tau - exact| / bound = %.3f" % (worst["M"], worst["tau"]))


@pytest.mark.parametrize("mode", [None, "generic"])
def test_cut_sweep(shared, tmp_path, mode):
    """toomuch from "the first chord already" to "never" x decks (none, in row tile 1, above the top: kend = 0, below
    the bottom) x transparent, through both kernels: the cut on every row position and row tile, different cuts among
    the 16 wavenumbers of a wave and the four of a lane."""
    from test_transit_restate_cpu import sweep_coverage
    c = _cases(shared, "sweep", lambda: [tc.sweep_case(shared["root"])])[0]
    res = run_child(tmp_path, "sweep", [c], mode=mode, tau=mode is not None)[0]
    worst = {"M": 0.0, "tau": 0.0}
    refs = shared["refs"].setdefault(c.dir, {})
    check(c, res, SCALAR if mode else MFMA, worst, refs)
    lasts = {}
    for n, v in enumerate(c.variants):
        lasts[n] = np.array(oracle_of(c, v).run(c.profs[1], want_tau=True)[2])
        if mode:
            assert np.array_equal(res[n]["last"], lasts[n])
    sweep_coverage(c, lasts)
    print("cut sweep (%s): worst |M - exact| / bound = %.3f, |tau - exact| / bound = %.3f" % (mode or "matrix tiles", worst["M"], worst["tau"]))


@pytest.mark.parametrize("mode", [None, "generic"])
def test_zero_extinction(shared, tmp_path, mode):
    """Exactly zero extinction in the top layers, everywhere, in a band: finite, within the bound of the exact value;
    everywhere + transparent: within the absolute bound of 0."""
    cases = _cases(shared, "zero", lambda: tc.zero_cases(shared["root"]))
    worst = {"M": 0.0, "tau": 0.0}
    for c, rs in zip(cases, run_child(tmp_path, "zero", cases, mode=mode, tau=mode is not None)):
        check(c, rs, SCALAR if mode else MFMA, worst, shared["refs"].setdefault(c.dir, {}))
        if c.tag == "all":
            rt2 = (rs[1]["rtop"][0] / tc.RSTAR) ** 2
            assert np.all(np.abs(rs[1]["spec"]) <= 13 * tr.U * rt2), np.abs(rs[1]["spec"]).max() / rt2
    print("zero extinction (%s): worst |M - exact| / bound = %.3f" % (mode or "matrix tiles", worst["M"]))


@pytest.mark.parametrize("mode", [None, "generic"])
def test_shortest_columns(shared, tmp_path, mode):
    """2 .. 33 layers (all columns exact) and the depths around the kernels' tile counts (128 / 129, 256 / 257, 320)."""
    cases = _cases(shared, "short", lambda: tc.short_cases(shared["root"]))
    worst = {"M": 0.0, "tau": 0.0}
    for c, rs in zip(cases, run_child(tmp_path, "short", cases, mode=mode, tau=mode is not None)):
        check(c, rs, SCALAR if mode else MFMA, worst, shared["refs"].setdefault(c.dir, {}))
    print("shortest columns (%s): worst |M - exact| / bound = %.3f, |tau - exact| / bound = %.3f"
          % (mode or "matrix tiles", worst["M"], worst["tau"]))


def test_line_by_line_form(shared, tmp_path):
    """rt_transit_mfma<0, C, KT, EXT>: C in {0, 1, 2, 4} x 16 / 150 / 260 layers.  Against the oracle's chord
    integration over the line-by-line oracle's extinction at 1e-9, and against the exact column of the DEVICE's own
    extinction array within the bound: that isolates the RT from the line sums."""
    from bart_amd import synth_lbl
    from oracle import lbl_oracle
    from test_gpu_parity import walkers
    worst = {"M": 0.0, "tau": 0.0}
    cases = []
    for L in (16, 150, 260):
        for C in (0, 1, 2, 4):
            keys = dict(tc.TKEYS, **({"cia_interp": "linear"} if C == 1 else {}))
            c = synth_lbl.make_lbl_case(os.path.join(shared["root"], "lbl%d_%d" % (L, C)), nlines=200, nwave=70, nlayers=L,
                                        cia={0: False, 1: 1, 2: 1, 4: 2}[C], extra_keys=keys)
            c.mc, c.checked = (0, C), tc.checked_columns(70)
            c.profs = np.array([c.profiles().ravel(), c.profiles(temp=c.temp0 * 1.1).ravel()])
            c.variants = [(c.tcfg, None, 0), (tc._variant(c, "tr", transparent=1), None, 1)]
            cases.append(c)
    named = set()
    for c, rs in zip(cases, run_child(tmp_path, "lbl", cases, lbl=True)):
        check(c, rs, MFMA_EXT, worst, lbl_oracle=lbl_oracle.LblOracle(c.tcfg))
        named.add((c.mc[1], len(c.press_bar)))
    assert named == {(C, L) for C in (0, 1, 2, 4) for L in (16, 150, 260)}
    print("line-by-line form: worst |M - exact| / bound = %.3f" % worst["M"])


CHORD_CHILD = r"""
import json, pickle, sys
import numpy as np
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
from bart_amd import engine, transit_module as trm
out = []
for tcfg, pfile in job["cases"]:
    engine.init(tcfg)
    engine.run_batch(np.load(pfile))
    r = {"t0": engine.chord_table(0), "t1": engine.chord_table(1), "rad": engine.get_radius()}
    bad = []
    for w in (2, -1):
        try:
            engine.chord_table(w); bad.append(None)
        except trm.TransitError as e:
            bad.append(str(e))
    lib = trm.lib()
    L = engine.nlayers()
    a, b = np.zeros(L), np.zeros((L, L))
    r["codes"] = [lib.bartrt_get_chord_table(0, None, trm._ptr(b), None), lib.bartrt_get_chord_table(0, trm._ptr(a), None, None),
                  lib.bartrt_get_chord_table(2, trm._ptr(a), trm._ptr(b), None)]
    r["bad"] = bad
    trm.free_memory()
    out.append(r)
engine.init(job["eclipse"])
engine.run_batch(np.load(job["eclipse_profs"]))
L = engine.nlayers()
a, b = np.zeros(L), np.zeros((L, L))
ecl = trm.lib().bartrt_get_chord_table(0, trm._ptr(a), trm._ptr(b), None)
msg = trm.lib().bartrt_last_error().decode()
trm.free_memory()
pickle.dump({"res": out, "eclipse": (ecl, msg)}, open(job["out"], "wb"))
"""


def test_chord_table(shared, tmp_path):
    """bartrt_get_chord_table: every entry within its own bound of the exact DS(k, j) (3.5 u (s_{j-1} + s_j) + u DS:
    the cancellation of the two roots, stated exactly), the radii, the exact zeros the matrix product relies on, and
    the getter's refusals."""
    from bart_amd import synth
    from test_gpu_parity import walkers
    cases = tc.chord_cases(shared["root"])
    ecl = synth.make_case(str(tmp_path / "ecl"), nlayers=12, nwave=20)
    np.save(str(tmp_path / "ecl.npy"), walkers(ecl, 2, seed=1))
    for c in cases:
        np.save(os.path.join(c.dir, "p.npy"), c.profs)
    job = {"root": ROOT, "cases": [(c.tcfg, os.path.join(c.dir, "p.npy")) for c in cases], "eclipse": ecl.tcfg,
           "eclipse_profs": str(tmp_path / "ecl.npy"), "out": str(tmp_path / "chords.pkl")}
    json.dump(job, open(str(tmp_path / "job.json"), "w"))
    r = subprocess.run([sys.executable, "-c", CHORD_CHILD, str(tmp_path / "job.json")], env=child_env(), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = pickle.load(open(job["out"], "rb"))
    EINVAL = -1          # include/bartrt.h
    worst = {"wide": 0.0, "thin": 0.0}
    for c, res in zip(cases, out["res"]):
        L = len(c.press_bar)
        rtop, ds, raw = res["t0"]
        assert np.array_equal(rtop, res["rad"][::-1]), c.dir            # (get_radius: the batch's first profile)
        assert np.all(np.diff(rtop) < 0)
        ch = tr.Chords(rtop)
        _, bound = ch.dense()
        dev = ch.exact_minus(ds)
        lower = np.tril(np.ones((L, L), bool))
        lower[:, 0] = False
        assert np.all(dev[~lower] == 0.0) and np.all(ds[lower] > 0.0), c.dir
        ratio = dev[lower] / bound[lower]
        worst[c.tag] = max(worst[c.tag], ratio.max())
        assert np.all(ratio <= 1.0), (c.dir, ratio.max())
        # the raw block: entry by entry the dense table where a chord and a layer exist, +0.0 everywhere else of the
        # steps the kernels read (row tile kt: steps 0 .. 4 kt + 3)
        nkt = (L + 15) // 16
        assert raw.shape == (nkt, 4 * nkt, 64)
        for kt in range(nkt):
            for s in range(4 * kt + 4):
                lane = np.arange(64)
                k, j = 16 * kt + lane % 16, 4 * s + lane // 16
                real = (k < L) & (j >= 1) & (j <= k)
                want = np.where(real, ds[np.minimum(k, L - 1), np.minimum(j, L - 1)], 0.0)
                assert np.array_equal(raw[kt, s].view(np.int64), want.view(np.int64)), (c.dir, kt, s)
        # the second walker's table is its own
        rtop1, ds1, _ = res["t1"]
        assert not np.array_equal(rtop1, rtop) and not np.array_equal(ds1, ds)
        d1 = tr.Chords(rtop1).exact_minus(ds1)
        assert np.all(d1[lower] <= tr.Chords(rtop1).dense()[1][lower])
        # refusals
        assert all(b is not None and "outside the latest batch" in b for b in res["bad"]), res["bad"]
        assert res["codes"] == [EINVAL, EINVAL, EINVAL], res["codes"]
    assert out["eclipse"][0] == EINVAL and "transit geometry only" in out["eclipse"][1], out["eclipse"]
    print("chord table: worst |entry - exact| / bound = %.3f (eight decades), %.3f (one decade)" % (worst["wide"], worst["thin"]))
