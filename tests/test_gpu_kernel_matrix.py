"""Every ahead-of-time cell of the specialised RT kernels against the oracle (oracle/rt_oracle.c column_eclipse).

Each kernel form is built for every (table molecules, CIA slots) pair of BARTRT_MC_LIST (csrc/kernels.hpp), with and
without the square-root ray order (SQ: the default ray grid 0 20 40 60 80 takes it, 10 35 50 65 85 does not).  One
small case per pair and ray grid: 37 layers (a partial last step at 8, 16 and 32 rows), 200 samples (a partial last
column), two walkers, `toomuch 1` (the cut lands between layers 14 and 32 of the column), without and with a cloud deck
in the middle of the column.  C = 0: no CIA; 1: one file under `cia_interp linear`; 2: one file under the default
spline; 4: two files under the spline.

BARTRT_KERNEL, BARTRT_WINDOW and BARTRT_FOLD are read once per process, so each forced form runs in a child that loops
over all cases and reports the kernel every launch took; the oracle runs once per (case, rule, cut, deck) in the parent.
Every launch must be the forced form, taken from the ahead-of-time set: no "[instantiated at run time]" note and no
run-time compile in the child (csrc/rtc.hpp).  With BARTRT_WINDOW=1 the row-per-layer forms address the table through
the moving window of a table above 4 GB (csrc/kernels.hpp row_window_base, rt_eclipse_qadj.hpp): the same arithmetic
from another base, so the same bits as without it.  tests/test_gpu_bigtable.py runs the window on a real big table.

The whole file takes about 12 s on an MI355X (pytest durations: each child 0.5-0.6 s, the folded / prefetched one 2 s),
measured on this build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import forced_kernel, many_molecules, walkers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
# BARTRT_MC_LIST (csrc/kernels.hpp); BARTRT_QADJ_LIST is the same list
MC_LIST = [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2),
           (5, 0), (5, 1), (5, 2), (6, 0), (6, 1), (6, 2), (1, 4), (2, 4), (3, 4), (4, 4), (5, 4), (6, 4)]
GRIDS = ((0, 20, 40, 60, 80), (10, 35, 50, 65, 85))      # SQ on / off
NLAYERS, NWAVE, NWALKERS, TOOMUCH = 37, 200, 2, 1.0
WINDOW_NOTE = "[table through a moving window]"

SLANT_ALL = [(1, "slant"), (0, "slant"), (2, "slant")]
VERT_ALL = [(0, "vertical"), (1, "vertical"), (2, "vertical")]
# BARTRT_KERNEL value -> the (rule, cut) launches it serves
FORMS = {
    "adj8": [(1, "slant")], "adj16": [(1, "slant")], "hexa": [(1, "slant")], "r32": [(1, "slant")],
    "quad": SLANT_ALL + VERT_ALL, "octo": SLANT_ALL + VERT_ALL, "mono_ilp": SLANT_ALL + VERT_ALL,
    "mono_occ": VERT_ALL, "split": [(0, "vertical"), (2, "vertical")],
}
ROW_PER_LAYER = ("adj8", "adj16", "quad", "octo", "hexa", "r32")
# the switches that choose a launch's kernel or change how it runs (read once per process): a child runs under its own
# settings only, whatever the caller's environment holds
SWITCHES = ("BARTRT_KERNEL", "BARTRT_WINDOW", "BARTRT_FOLD", "BARTRT_SQ", "BARTRT_ADJ", "BARTRT_INTEG", "BARTRT_CUT",
            "BARTRT_CIA_INTERP", "BARTRT_BLOCK", "BARTRT_KERNEL_BY", "BARTRT_RTC")


def child_env(**switches):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    return env

CHILD = r"""
import json, sys
import numpy as np
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
from bart_amd import engine, transit_module as trm
spectra, names = [], []
for case in job["cases"]:
    engine.init(case["tcfg"])
    p = np.load(case["profs"])
    got, nm = np.zeros((len(job["combos"]), 2, p.shape[0], trm.get_no_samples())), []
    for deck in (0, 1):
        if deck:
            trm.set_cloudtop(case["cloudtop"])
        for i, (rule, cut) in enumerate(job["combos"]):
            trm.set_integ(rule); trm.set_cut(cut)
            engine.walked_begin(); got[i, deck] = engine.run_batch(p); nm.append(engine.walked_end()[2])
    trm.free_memory()
    spectra.append(got); names.append(nm)
np.save(job["out"], np.array(spectra))
print("RESULT" + json.dumps({"names": names, "rtc": trm.get_rtc_stats()}))
"""


def _case(d, M, C, grid, **extra):
    from bart_amd import synth
    keys = {"cia_interp": "linear"} if C == 1 else {}
    keys.update(extra)
    c = synth.make_case(d, nlayers=NLAYERS, nwave=NWAVE, raygrid=grid, toomuch=TOOMUCH, cia={0: False, 1: 1, 2: 1, 4: 2}[C],
                        tlow=400.0, thigh=3000.0, tempdelt=650.0, extra_keys=keys or None, **many_molecules(M))
    np.save(os.path.join(d, "p.npy"), walkers(c, NWALKERS, seed=10 * M + C))
    c.cloudtop = float(np.log10(c.press_bar[NLAYERS // 2 - 2]))    # (layer 20 from the top: some columns reach it)
    return c


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    """The cases, the oracle's spectra [case][(rule, cut, deck)] and the children's results (filled as they run)."""
    from oracle import rt_oracle as orc
    cases = []
    for M, C in MC_LIST:
        for g, grid in enumerate(GRIDS):
            c = _case(str(tmp_path_factory.mktemp("mc%d_%d_g%d" % (M, C, g))), M, C, grid)
            c.mc = (M, C)
            cases.append(c)
    refs = []
    for c in cases:
        p, r = np.load(os.path.join(c.dir, "p.npy")), {}
        for rule in (0, 1, 2):
            for cut in ("slant", "vertical"):
                o = orc.OracleEngine(c.tcfg, integ=rule, cut=cut)
                r[rule, cut, 0] = o.run_batch(p)
                o.set_cloudtop(c.cloudtop)
                r[rule, cut, 1] = o.run_batch(p)
        refs.append(r)
    return {"cases": cases, "refs": refs, "runs": {}, "dir": str(tmp_path_factory.mktemp("matrix_out"))}


def _run(matrix, mode, window):
    """The child of BARTRT_KERNEL=mode (window: BARTRT_WINDOW=1) over every case -> (spectra, names)."""
    if (mode, window) in matrix["runs"]:
        return matrix["runs"][mode, window]
    tag = "%s_w%d" % (mode, window)
    job = {"root": ROOT, "combos": FORMS[mode], "out": os.path.join(matrix["dir"], tag + ".npy"),
           "cases": [{"tcfg": c.tcfg, "profs": os.path.join(c.dir, "p.npy"), "cloudtop": c.cloudtop} for c in matrix["cases"]]}
    jfile = os.path.join(matrix["dir"], tag + ".json")
    json.dump(job, open(jfile, "w"))
    env = child_env(BARTRT_KERNEL=mode, **({"BARTRT_WINDOW": "1"} if window else {}))
    r = subprocess.run([sys.executable, "-c", CHILD, jfile], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])
    # the ahead-of-time set served every launch: no kernel was compiled or loaded at run time
    assert res["rtc"]["compiled"] == 0 and res["rtc"]["from_disk"] == 0, (mode, res["rtc"])
    matrix["runs"][mode, window] = (np.load(job["out"]), res["names"])
    return matrix["runs"][mode, window]


@pytest.mark.parametrize("mode", list(FORMS))
def test_every_aot_cell_matches_oracle(matrix, mode):
    """BARTRT_KERNEL=mode on all 48 cases, every rule and cut the form serves, without and with a deck."""
    got, names = _run(matrix, mode, False)
    combos = FORMS[mode]
    for k, (c, ref) in enumerate(zip(matrix["cases"], matrix["refs"])):
        for deck in (0, 1):
            for i, (rule, cut) in enumerate(combos):
                kname = names[k][deck * len(combos) + i]
                what = "M, C = %s, grid %d, rule %d, cut %s, deck %d: %s" % (c.mc, k % 2, rule, cut, deck, kname)
                assert kname.split(" [")[0] == forced_kernel(mode, rule, cut), what
                assert "[instantiated at run time]" not in kname and WINDOW_NOTE not in kname, what
                r = ref[rule, cut, deck]
                np.testing.assert_allclose(got[k, i, deck], r, rtol=RTOL, atol=1e-12 * np.abs(r).max() if rule == 1 else 0.0,
                                           err_msg=what)
        for i in range(len(combos)):
            assert not np.allclose(got[k, i, 0], got[k, i, 1])      # the deck is reached


@pytest.mark.parametrize("mode", ROW_PER_LAYER)
def test_moving_window_gives_the_same_bits(matrix, mode):
    """BARTRT_WINDOW=1: the row-per-layer forms rebuild their table descriptor per step around the step's smallest
    plane offset.  Same kernels, same spectra bit for bit; the launch record says the window was used."""
    off, _ = _run(matrix, mode, False)
    on, names = _run(matrix, mode, True)
    combos = FORMS[mode]
    for k, c in enumerate(matrix["cases"]):
        for j, kname in enumerate(names[k]):
            rule, cut = combos[j % len(combos)]
            assert kname.split(" [")[0] == forced_kernel(mode, rule, cut) and WINDOW_NOTE in kname, (c.mc, kname)
            assert "[instantiated at run time]" not in kname, (c.mc, kname)
    assert np.array_equal(on, off)


TRANSIT_CHILD = r"""
import json, sys
import numpy as np
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
from bart_amd import engine, transit_module as trm
out, names = [], []
for tcfg, pfile, ct in job["cases"]:
    engine.init(tcfg)
    if ct is not None:
        trm.set_cloudtop(ct)
    engine.walked_begin(); out.append(engine.run_batch(np.load(pfile))); names.append(engine.walked_end()[2])
    trm.free_memory()
np.save(job["out"], np.array(out))
print("RESULT" + json.dumps(names))
"""


def test_transit_kernel_through_the_window(tmp_path):
    """The matrix-tile transit kernel (transit_geom.hip rt_transit_mfma) with BARTRT_WINDOW=1 against the oracle:
    four molecules + two CIA files, and six + one with a cloud deck."""
    from oracle import rt_oracle as orc
    tr = {"solution": "transit", "starrad": 1.145}
    cases = [(_case(str(tmp_path / "t44"), 4, 4, GRIDS[0], **tr), None), (_case(str(tmp_path / "t62"), 6, 2, GRIDS[0], **tr), True)]
    job = {"root": ROOT, "out": str(tmp_path / "transit.npy"),
           "cases": [(c.tcfg, os.path.join(c.dir, "p.npy"), c.cloudtop if deck else None) for c, deck in cases]}
    json.dump(job, open(str(tmp_path / "job.json"), "w"))
    r = subprocess.run([sys.executable, "-c", TRANSIT_CHILD, str(tmp_path / "job.json")], env=child_env(BARTRT_WINDOW="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(job["out"])
    names = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])
    for k, (c, deck) in enumerate(cases):
        assert names[k] == "rt_transit_mfma " + WINDOW_NOTE, names[k]
        o = orc.OracleEngine(c.tcfg)
        plain = o.run_batch(np.load(os.path.join(c.dir, "p.npy")))
        if deck:
            o.set_cloudtop(c.cloudtop)
        ref = o.run_batch(np.load(os.path.join(c.dir, "p.npy")))
        np.testing.assert_allclose(got[k], ref, rtol=RTOL, err_msg=c.tcfg)
        assert not deck or not np.allclose(ref, plain)


FOLD_CHILD = r"""
import json, sys
import numpy as np
import torch
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
from bart_amd import engine, transit_module as trm
res = []
for tcfg, pfile in job["cases"]:
    engine.init(tcfg)
    p = np.load(pfile)
    engine.walked_begin(); one = engine.run_batch(p[:1]); k1 = engine.walked_end()[2]
    two = engine.run_batch(p[1:2])
    d = torch.from_numpy(p).cuda()
    a, b = d[:1].contiguous(), d[1:2].contiguous()
    # the launch that carries the next batch's preparation, then the launch that uses it
    engine.walked_begin(); head = engine.run_batch_dev(a, next_prof=b).cpu().numpy(); k0 = engine.walked_end()[2]
    engine.walked_begin(); pre = engine.run_batch_dev(b).cpu().numpy(); k2 = engine.walked_end()[2]
    trm.free_memory()
    res.append({"one": one.tolist(), "two": two.tolist(), "head": head.tolist(), "pre": pre.tolist(), "k0": k0, "k1": k1,
                "k2": k2})
print("RESULT" + json.dumps({"res": res, "rtc": trm.get_rtc_stats()}))
"""


def test_folded_and_prefetched_preparation_through_the_window(matrix):
    """One walker under the default conventions with BARTRT_WINDOW=1: the adjacent-rows kernel prepares its own
    walker's layer records (PrepFold) and reads the table through the window; with the next batch prefetched
    (run_batch_dev(..., next_prof=)) the launch carrying the next batch's preparation and the launch that uses the
    prepared records (neither prepares its own walker: no fold note) give the same bits as the folded ones."""
    cases = [(k, c) for k, c in enumerate(matrix["cases"]) if c.mc in ((1, 0), (4, 4), (6, 2), (3, 1))]
    jfile = os.path.join(matrix["dir"], "fold.json")
    json.dump({"root": ROOT, "cases": [(c.tcfg, os.path.join(c.dir, "p.npy")) for _, c in cases]}, open(jfile, "w"))
    r = subprocess.run([sys.executable, "-c", FOLD_CHILD, jfile], env=child_env(BARTRT_WINDOW="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])
    assert out["rtc"]["compiled"] == 0 and out["rtc"]["from_disk"] == 0, out["rtc"]
    for (k, c), res in zip(cases, out["res"]):
        assert res["k1"].startswith("rt_eclipse_qadj<R=") and "[prepares its own walkers]" in res["k1"], (c.mc, res["k1"])
        fold = "[prepares its own walkers]"
        for kn in (res["k0"], res["k2"]):
            assert kn.startswith(res["k1"].split(" [")[0]) and WINDOW_NOTE in kn and fold not in kn, (c.mc, kn)
        assert WINDOW_NOTE in res["k1"], (c.mc, res["k1"])
        ref = matrix["refs"][k][1, "slant", 0]
        np.testing.assert_allclose(np.array(res["one"])[0], ref[0], rtol=RTOL, atol=1e-12 * np.abs(ref).max())
        assert np.array_equal(res["head"], res["one"]) and np.array_equal(res["pre"], res["two"]), c.mc
