"""The optimistic loop of rule 1's single-wave `cut slant` kernel (csrc/rt_eclipse_s1s.hpp): whole six-layer blocks
walked without ray flags and event log while every lane's optical depth stands below a guard, a check at each such
block's end, and a second, flagged walk of the column for a wave that finds a ray dead there.

Every case runs its batch with the guard off (bartrt_set_slant_opt(0)) and on in ONE process and asks for the same
bits; the guard-on spectra are also held to the oracle at the suite's 1e-10.  The shape is the <5, 4, 2> instantiation
of the kernel: five ray angles, four table molecules, one CIA file under the spline; 130 wavenumbers are three
single-wave tiles, the last one partial; three walkers.  The columns are chosen so that each path of the kernel's
control flow is the one exercised (the comments on CASES).  BARTRT_KERNEL is read once per process, so the launches
run in one child that loops over all cases; the oracle runs once per case in the parent.

The restarted-wave counts come from the kernel's diagnostic record (engine.walked_restarts, filled with the
layers-walked record only).  About 2 s on an MI355X, most of it the child's start-up."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_kernel_matrix import child_env
from test_gpu_parity import forced_kernel, walkers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
NWAVE, NWALKERS = 130, 3
G4 = 2.0 ** -4

# name -> (make_case keywords, guards run after the guard-off launch, layer of the extinction jump or None)
CASES = {
    # a transparent column: every whole block is optimistic.  31 layers: five whole blocks and a masked one;
    # 20 layers: kcut = 18, three whole blocks and a short masked one
    "clear31": (dict(nlayers=31, kappa_model="survey8d"), (G4,), None),
    "clear20": (dict(nlayers=20, kappa_model="survey8d"), (G4,), None),
    # rays die in mid-column: the optimistic loop hands over to the flagged one.  Guard 2^0 is the tightest: the
    # check at the block's end is then the only protection
    "forest40": (dict(nlayers=40), (G4, 1.0), None),
    # walker 1's extinction jumps by far more than 1e3 on layer 6 b + 3, in the MIDDLE of whole block b: tau passes
    # from below the guard to above the smallest threshold inside one optimistic block, and the wave walks again
    "jump_b1": (dict(nlayers=31), (G4,), 9),
    "jump_b2": (dict(nlayers=31), (G4,), 15),
    # every threshold the largest double: every whole block optimistic, whatever the depth
    "nocut": (dict(nlayers=31, toomuch=1e100), (G4,), None),
    # the first layer with any depth kills the 80-degree ray: nothing is optimistic
    "allcut": (dict(nlayers=31, toomuch=1e-30), (G4,), None),
    # the whole column is the single masked block
    "short5": (dict(nlayers=5), (G4,), None),
}
SHARDED = "forest40"     # also run as two wavenumber blocks under `kernel_by whole`

CHILD = r"""
import json, sys
import numpy as np
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
from bart_amd import engine, transit_module as trm
out = {}
def launch(p, guard):
    trm.set_slant_opt(guard)
    engine.walked_begin(); s = engine.run_batch(p); name = engine.walked_end()[2]
    return s, name, engine.walked_restarts()
for case in job["cases"]:
    p = np.load(case["profs"])
    engine.init(case["tcfg"])
    for g in [0.0] + case["guards"]:
        s, name, rs = launch(p, g)
        out["%s/spec/%r" % (case["name"], g)] = s
        out["%s/restarts/%r" % (case["name"], g)] = rs
        out["%s/kernel/%r" % (case["name"], g)] = np.array(name)
    trm.free_memory()
    if case["sharded"]:
        for r in range(2):
            engine.init(case["tcfg"], shard=(r, 2), kernel_by="whole")
            s, name, rs = launch(p, case["guards"][0])
            out["%s/shard%d" % (case["name"], r)] = s
            out["%s/shard%d/kernel" % (case["name"], r)] = np.array(name)
            trm.free_memory()
np.savez(job["out"], **out)
print("RESULT" + json.dumps({"rtc": trm.get_rtc_stats()}))
"""


def jump_profile(case, prof, layer):
    """prof with the table molecules' abundances 1e-10 above `layer` (counted from the top) and 3e-3 from it down."""
    L, S = len(case.press_bar), len(case.species)
    p = prof.reshape(S + 1, L).copy()
    below = np.arange(L) <= L - 1 - layer          # (atm order: index 0 is the bottom layer)
    p[3:] = np.where(below, 3e-3, 1e-10)[None, :]
    q = 1.0 - p[3:].sum(0)
    p[1], p[2] = 0.15 * q, 0.85 * q                # He, H2
    return p.ravel()


def build_case(d, name):
    from bart_amd import synth
    kw, guards, jump = CASES[name]
    c = synth.make_case(d, nwave=NWAVE, cia=1, tlow=400.0, thigh=3000.0, tempdelt=650.0, **kw)
    profs = walkers(c, NWALKERS, seed=len(name))
    if jump is not None:
        profs[1] = jump_profile(c, profs[1], jump)
    np.save(os.path.join(d, "p.npy"), profs)
    return c, profs


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """name -> {"ref": the oracle's spectra, "spec": {guard: spectra}, "restarts": {guard: counts}, ...}."""
    from oracle import rt_oracle as orc
    res, jobs = {}, []
    for name, (kw, guards, jump) in CASES.items():
        c, profs = build_case(str(tmp_path_factory.mktemp(name)), name)
        res[name] = {"ref": orc.OracleEngine(c.tcfg, integ=1, cut="slant").run_batch(profs)}
        jobs.append({"name": name, "tcfg": c.tcfg, "profs": os.path.join(c.dir, "p.npy"), "guards": list(guards),
                     "sharded": name == SHARDED})
    d = str(tmp_path_factory.mktemp("out"))
    job = {"root": ROOT, "cases": jobs, "out": os.path.join(d, "out.npz")}
    json.dump(job, open(os.path.join(d, "job.json"), "w"))
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(d, "job.json")], env=child_env(BARTRT_KERNEL="mono_ilp"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rtc = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])["rtc"]
    assert rtc["compiled"] == 0 and rtc["from_disk"] == 0, rtc      # the ahead-of-time <5, 4, 2> served every launch
    out = np.load(job["out"])
    want = forced_kernel("mono_ilp", 1, "slant")
    for name, (kw, guards, jump) in CASES.items():
        e = res[name]
        e["spec"] = {g: out["%s/spec/%r" % (name, g)] for g in (0.0,) + guards}
        e["restarts"] = {g: out["%s/restarts/%r" % (name, g)] for g in (0.0,) + guards}
        for g in (0.0,) + guards:
            assert str(out["%s/kernel/%r" % (name, g)]) == want, (name, g, str(out["%s/kernel/%r" % (name, g)]))
    res[SHARDED]["shards"] = [out["%s/shard%d" % (SHARDED, r)] for r in range(2)]
    for r in range(2):
        assert str(out["%s/shard%d/kernel" % (SHARDED, r)]) == want
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_guard_on_gives_the_bits_of_guard_off(runs, name):
    """Both loops give every lane the same bits, on every path: the spectra with the optimistic loop are those
    without it, bit for bit, and the oracle's to 1e-10."""
    e = runs[name]
    off = e["spec"][0.0]
    assert np.isfinite(off).all() and (off != 0.0).any()
    assert not e["restarts"][0.0].any()          # guard off: no optimistic block, no second walk
    for g in CASES[name][1]:
        assert np.array_equal(e["spec"][g], off), (name, g, np.abs(e["spec"][g] - off).max())
        np.testing.assert_allclose(e["spec"][g], e["ref"], rtol=RTOL, atol=1e-12 * np.abs(e["ref"]).max(),
                                   err_msg="%s, guard %r" % (name, g))


@pytest.mark.parametrize("name", ["clear31", "clear20", "nocut", "allcut", "short5"])
def test_no_wave_walks_twice_where_no_ray_dies_inside_a_block(runs, name):
    """A transparent column, thresholds no depth reaches, a column without an optimistic block: no restart."""
    assert not runs[name]["restarts"][G4].any(), runs[name]["restarts"][G4]


@pytest.mark.parametrize("name", ["jump_b1", "jump_b2"])
def test_a_jump_inside_a_block_restarts_the_wave(runs, name):
    """The walker with the extinction jump in mid-block has waves that walked twice (its neighbours' bits and its
    own are the guard-off ones: test_guard_on_gives_the_bits_of_guard_off)."""
    rs = runs[name]["restarts"][G4]
    assert rs.shape == (NWALKERS,) and rs[1] > 0, rs
    assert rs[1] <= 3, rs                         # (three waves per walker)


def test_shards_concatenate_to_the_unsharded_bits(runs):
    """Two wavenumber blocks under `kernel_by whole`: a block's tiles start elsewhere, so its waves hold other
    wavenumbers and hand over or restart on their own -- the concatenation is the unsharded spectrum bit for bit only
    because either loop gives a lane the same bits."""
    e = runs[SHARDED]
    cat = np.concatenate(e["shards"], axis=1)
    assert cat.shape == e["spec"][G4].shape
    assert np.array_equal(cat, e["spec"][G4])
