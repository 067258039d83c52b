"""A real opacity table above 4 GiB: 100 layers x 60 temperatures x 6 molecules x 16 003 samples = 4.61 GB.

The row-per-layer kernels (rt_eclipse_quad, rt_eclipse_qadj, rt_transit_mfma) address the table with per-lane 32-bit
offsets; from `kappa_bytes >= 2^32 - 4096` on they rebuild their buffer descriptor every step around the smallest plane
offset of the step's rows (csrc/kernels.hpp row_window_base, the loop in rt_eclipse_qadj.hpp, transit_geom.hip).
A base that is off reads the wrong planes only where offsets pass 4 GiB -- here the top seven layers of the column,
which every walk crosses -- so a small grid cannot catch it (tests/test_gpu_kernel_matrix.py forces the window there and
checks that it leaves the bits alone).

One walker under the default conventions takes qadj<R=8> with its own preparation (500 workgroups: one round), two
and twelve the single-wave slant kernel; forced forms run in children (BARTRT_KERNEL is read once per process).
Everything against the oracle on three slices of 200 samples, the grid's ragged last column included.

Cost: 4.6 GB of temporary disk (removed at teardown), a few GB of host memory; 11 s for the module on an MI355X host
(pytest durations: 3.3 s of fixture set-up writing the table, about 1 s per child that loads it), measured on this
build."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_kernel_matrix import child_env
from test_gpu_parity import many_molecules, walkers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
L, M, W = 100, 6, 16003
SLICES = ((0, 200), (7900, 8100), (W - 200, W))
WINDOW_NOTE = "[table through a moving window]"


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """(eclipse case, transit cfg) on one table file; the directory is removed at the end of the module."""
    from bart_amd import synth
    d = str(tmp_path_factory.mktemp("bigtable"))
    try:
        c = synth.make_case(d, nlayers=L, nwave=W, tlow=400.0, thigh=3055.0, tempdelt=45.0, **many_molecules(M))
        nt = len(c.tgrid)
        assert nt == 60 and L * nt * M * W * 8 >= 2 ** 32
        assert os.path.getsize(c.opacity) > 2 ** 32
        txt = open(c.tcfg).read()
        assert "solution eclipse\n" in txt
        tcfg = os.path.join(d, "transit_geom.cfg")
        open(tcfg, "w").write(txt.replace("solution eclipse\n", "solution transit\nstarrad 1.145\n"))
        yield c, tcfg
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _oracle_slices(tcfg, profs, **kw):
    from oracle import rt_oracle as orc
    out = []
    for lo, hi in SLICES:
        o = orc.OracleEngine(tcfg, wn_lo=lo, wn_hi=hi, **kw)
        out.append(o.run_batch(profs))
    return out


def _check_slices(got, refs, rule=1, what=""):
    """(rule 1 on coarse columns: also 1e-12 of the largest sample, as in test_gpu_fuzz.py; transit: rule=0)"""
    for (lo, hi), ref in zip(SLICES, refs):
        np.testing.assert_allclose(got[:, lo:hi], ref, rtol=RTOL, atol=1e-12 * np.abs(ref).max() if rule == 1 else 0.0,
                                   err_msg="%s [%d, %d)" % (what, lo, hi))


def test_eclipse_default_choice(big):
    """1 walker: qadj<R=8>, folded, through the window; 1 walker with the next one prefetched; 2 and 12 walkers: the
    single-wave slant kernel.  The walk of every column crosses the layers stored above 4 GiB."""
    import torch
    from bart_amd import engine, transit_module as trm
    c, _ = big
    profs = walkers(c, 12, seed=41)
    refs = _oracle_slices(c.tcfg, profs[[0, 1, 11]])
    engine.init(c.tcfg)
    try:
        assert trm.get_integ() == 1 and trm.get_cut() == "slant" and trm.get_no_samples() == W
        ncol = (W + 63) // 64
        assert trm.lib().bartrt_kernel_choice(M, ncol).decode() == "adj8"
        engine.walked_begin()
        one = engine.run_batch(profs[:1])
        walked, wpc, kname = engine.walked_end()
        assert kname.startswith("rt_eclipse_qadj<R=8> ") and "[prepares its own walkers]" in kname and WINDOW_NOTE in kname, kname
        # (layers l >= 94 of the table, walk steps 0 .. 6 from the top, lie wholly above 4 GiB: every column of the grid
        # passes them -- the launch's padding columns past it walk nothing)
        walked = walked[:, :(W + wpc - 1) // wpc]
        assert walked.shape == (1, 2001) and walked.min() >= 8, walked.min()
        _check_slices(one, [r[:1] for r in refs], what=kname)
        # the next walker prefetched: the launch that carries its preparation (head-of-grid workgroups), then the one
        # that uses the prepared records -- neither prepares its own walker
        d = torch.from_numpy(profs[:2]).cuda()
        engine.walked_begin()
        head = engine.run_batch_dev(d[:1].contiguous(), next_prof=d[1:2].contiguous()).cpu().numpy()
        khead = engine.walked_end()[2]
        engine.walked_begin()
        pre = engine.run_batch_dev(d[1:2].contiguous()).cpu().numpy()
        kpre = engine.walked_end()[2]
        for kn in (khead, kpre):
            assert kn.startswith("rt_eclipse_qadj<R=8> ") and WINDOW_NOTE in kn and "[prepares its own walkers]" not in kn, kn
        assert np.array_equal(head, one)
        assert np.array_equal(pre, engine.run_batch(profs[1:2]))
        for n in (2, 12):
            assert trm.lib().bartrt_kernel_choice(M, n * ncol).decode() == "single"
            engine.walked_begin()
            got = engine.run_batch(profs[:n])
            kname = engine.walked_end()[2]
            assert kname.startswith("rt_eclipse_simpson_slant"), kname
            _check_slices(got[[0, 1, n - 1]] if n == 12 else got, [r[:n] if n == 2 else r for r in refs], what=kname)
    finally:
        trm.free_memory()


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from bart_amd import engine, transit_module as trm
tcfg, pfile, out = sys.argv[2:5]
p = np.load(pfile)
engine.init(tcfg)
res, names, deepest = [], [], []
for rule, cut in json.loads(sys.argv[5]):
    trm.set_integ(rule); trm.set_cut(cut)
    engine.walked_begin(); res.append(engine.run_batch(p)); w, wpc, kname = engine.walked_end()
    names.append(kname)
    # the fewest layers any column of the grid walked (the launch's padding columns past it walk nothing)
    deepest.append(int(w[:, :(trm.get_no_samples() + wpc - 1) // wpc].min()))
trm.free_memory()
np.save(out, np.array(res))
print("NAMES" + json.dumps([names, deepest]))
"""
# BARTRT_KERNEL -> (rule, cut) launches, the form each must name
FORCED = {
    "adj16": [((1, "slant"), "rt_eclipse_qadj<R=16> ")],
    "quad": [((1, "slant"), "rt_eclipse_quad<R=4, all rays per lane>"), ((0, "slant"), "rt_eclipse_quad<R=4, one ray per lane>"),
             ((1, "vertical"), "rt_eclipse_quad<R=4> ")],
    "hexa": [((1, "slant"), "rt_eclipse_quad<R=16, all rays per lane>")],
    "r32": [((1, "slant"), "rt_eclipse_quad<R=32, all rays per lane>")],
}


@pytest.mark.parametrize("mode", list(FORCED))
def test_eclipse_forced_forms(big, tmp_path, mode):
    """The other row-per-layer forms through the window, two walkers each, in a child per BARTRT_KERNEL value."""
    c, _ = big
    profs = walkers(c, 2, seed=43)
    np.save(str(tmp_path / "p.npy"), profs)
    combos = [rc for rc, _ in FORCED[mode]]
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, c.tcfg, str(tmp_path / "p.npy"), str(tmp_path / "s.npy"),
                        json.dumps(combos)], env=child_env(BARTRT_KERNEL=mode), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    names, deepest = json.loads([l for l in r.stdout.splitlines() if l.startswith("NAMES")][0][5:])
    got = np.load(str(tmp_path / "s.npy"))
    for k, ((rule, cut), want) in enumerate(FORCED[mode]):
        assert names[k].startswith(want) and WINDOW_NOTE in names[k], names[k]
        assert deepest[k] >= 8, (names[k], deepest[k])      # every column walks past the layers above 4 GiB
        _check_slices(got[k], _oracle_slices(c.tcfg, profs, integ=rule, cut=cut), rule=rule, what=names[k])


def test_transit_geometry(big):
    """The matrix-tile transit kernel through the window, one and six walkers."""
    from bart_amd import engine, transit_module as trm
    c, tcfg = big
    profs = walkers(c, 6, seed=47)
    refs = _oracle_slices(tcfg, profs)
    engine.init(tcfg)
    try:
        for n in (1, 6):
            engine.walked_begin()
            got = engine.run_batch(profs[:n])
            assert engine.walked_end()[2] == "rt_transit_mfma " + WINDOW_NOTE
            _check_slices(got, [r[:n] for r in refs], rule=0, what="transit, %d walkers" % n)
    finally:
        trm.free_memory()


def test_contribution_functions(big, tmp_path):
    """engine.contribution on the big grid (its own walk of the table, no toomuch cut) against the oracle's optical
    depth at `toomuch 1e100` through the tests' restatement of code/cf.py, per wavenumber on the three slices."""
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    from test_gpu_cf import TOL, _rel, cf_restate, inf_cfg, write_filters
    c, _ = big
    prof = walkers(c, 1, seed=53)
    files = write_filters(str(tmp_path), c.wn)
    engine.init(c.tcfg)
    try:
        band, full = engine.contribution(prof, files, normalize=False, full=True)
    finally:
        trm.free_memory()
    assert full.shape == (1, W, L) and np.all(np.isfinite(band))
    cfg = inf_cfg(c, str(tmp_path))
    for lo, hi in SLICES:
        o = orc.OracleEngine(cfg, wn_lo=lo, wn_hi=hi)
        _, tau, _ = o.run(prof[0], want_tau=True)
        ref = cf_restate.contribution(prof[0, :L], c.press_bar, tau.T, o.wn).T[:, ::-1]
        assert _rel(full[0, lo:hi], ref) < TOL, (lo, hi)
