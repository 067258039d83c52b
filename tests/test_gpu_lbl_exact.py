"""GPU: lbl_states and the four accumulation kernels of csrc/lbl.hip against the exact restatement of tests/lbl_restate.py
(mpmath, 34 digits) on the cases of tests/lbl_cases.py, under the bound derived there -- the branch claims lbl.hip
documents, exp_core's and rcp_n1's documented errors and counted roundings.  No other tolerance appears.

  states      engine.lbl_states (bartrt_lbl_get_states: what lbl_states / lbl_smax wrote) against the restated state:
              T the input's bits, dv exact wherever its comparison is decided, the Doppler factor within 5 roundings,
              the Lorentz half-width within 16, SIGCTE * scale within 13, smax within its line's strength bound
              (lbl_restate's docstring counts them)
  extinction  engine.lbl_extinction (the opacity file for `table`) on every point: inside the bound where decided,
              exact zeros where no kept line reaches, inside the widened interval where undecided; prints the worst
              error / bound per case and per owner
  bits        the same column in a single call, in five and in two wavenumber blocks (cuts at 64, 128, 192, 256 | 65 and
              at 160 | 161), and the states of walker 2 of a three-walker batch with the spectrum it gives: all to the bit
              (the per-walker extinction of a batch has no read-back; its states and its spectrum have)

The restated values are computed once per process (lbl_cases.get) and shared; `mid` runs in a child process
(BARTRT_MID_REACH is read once per process).
Worst error / bound on an MI355X: 0.97 (doppler, the pair kernel); per case and owner in MEASUREMENTS.md, row 31.
Pytest durations on an MI355X: 7.3 s for the module; mixed 1.8 s, pressure 1.3 s, osamp 1.0 s (the restatement), every
other test below 0.8 s."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lbl_cases as LC
import lbl_owner_restate as R
import lbl_restate as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOP_U, LOR_U, SCALE_U = 5, 16, X.N_SCALE
_dev = {}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("lbl_exact"))
    return lambda name: LC.get(name, root)


def _device(cs, tmp=None):
    """dict(ext[L, W] or [L, G, W], states or None, owners or None) of a fresh engine's single call, once per case."""
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    if cs.name in _dev:
        return _dev[cs.name]
    if cs.mid_reach:
        f = lambda n: os.path.join(cs.c.dir, n)
        np.save(f("p.npy"), cs.prof)
        code = ("import numpy as np, sys; sys.path.insert(0, %r)\n"
                "from bart_amd import engine, transit_module as trm\n"
                "p = np.load(%r); engine.init(%r)\n"
                "s = engine.lbl_states(p)\n"
                "np.savez(%r, own=engine.lbl_owners(p), ext=engine.lbl_extinction(p), **s); trm.free_memory()\n"
                % (ROOT, f("p.npy"), cs.c.tcfg, f("dev.npz")))
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, BARTRT_MID_REACH=str(cs.mid_reach)),
                              timeout=120)
        z = np.load(f("dev.npz"))
        out = dict(ext=z["ext"], owners=z["own"], states={k: z[k] for k in ("T", "dv", "dop", "lor", "scale", "smax")})
    else:
        engine.init(cs.c.tcfg)
        try:
            if cs.per_gram:
                op = orc.read_opacity(cs.c.keys["opacityfile"])
                assert list(op["temps"]) == [1000.0, 1100.0] and op["kappa"].shape == (LC.NLAYERS, 2, 2, cs.W)
                out = dict(ext=op["kappa"][:, 0], owners=None, states=None)
            else:
                states = engine.lbl_states(cs.prof)
                out = dict(ext=engine.lbl_extinction(cs.prof), owners=engine.lbl_owners(cs.prof), states=states)
        finally:
            trm.free_memory()
    _dev[cs.name] = out
    return out


@pytest.mark.parametrize("name", [n for n in LC.GPU_CASES if n != "table"])
def test_states_against_the_restated_state(case, name):
    cs = case(name)
    cs.sharp()
    dev = _device(cs)["states"]
    want = cs.restated_states()
    rs = X.Restatement(cs.su)
    assert dev["T"].shape == (LC.NLAYERS,) and dev["dop"].shape == (LC.NLAYERS, 3) and dev["smax"].shape == (LC.NLAYERS, 2)
    worst = dict(dop=0.0, lor=0.0, scale=0.0, smax=0.0)
    for l, st in enumerate(want):
        assert dev["T"][l] == cs.prof[0, l]
        assert st["dv_margin"] >= X.D_DV, "choose the inputs so that every divisor is decided"
        assert dev["dv"][l] == st["dv"], (name, l, dev["dv"][l], st["dv"])
        for key, n in (("dop", DOP_U), ("lor", LOR_U), ("scale", SCALE_U)):
            for i in range(3):
                e, g = st[key][i], float(dev[key][l, i])
                if e == 0:
                    assert g == 0.0            # (no collider: the Lorentz width is exactly 0)
                    continue
                r = float(abs(X.mpf(g) / e - 1)) / (n * X.U)
                worst[key] = max(worst[key], r)
        for g in range(2):
            S = rs.strengths(st, g)
            smax, eps = max(S, key=lambda t: t[0])
            r = float(abs(X.mpf(float(dev["smax"][l, g])) / smax - 1)) / eps
            worst["smax"] = max(worst["smax"], r)
    print("%s states: largest error / counted roundings %s" % (name, {k: round(v, 3) for k, v in worst.items()}))
    assert all(v <= 1 for v in worst.values()), worst


@pytest.mark.parametrize("name", LC.GPU_CASES)
def test_extinction_inside_the_bound(case, name):
    cs = case(name)
    cs.sharp()
    dev = _device(cs)
    res = cs.restated()
    if dev["owners"] is not None:
        assert np.array_equal(dev["owners"], cs.owners), (dev["owners"].T, cs.owners.T)
        pts = R.point_owners(cs.owners, cs.W)
    worst, n_und, n_all, checks = {}, 0, 0, []
    for key, r in res.items():
        got = dev["ext"][key] if cs.per_gram else dev["ext"][key]
        assert got.shape == (cs.W,) and np.all(np.isfinite(got))
        v, dec = r.v, ~r.undecided
        n_und += int(r.undecided.sum()); n_all += cs.W
        pos = dec & (r.bound > 0)
        ratio = np.abs(got - v)[pos] / r.bound[pos]
        own = pts[key][pos] if dev["owners"] is not None else np.full(pos.sum(), -1)
        for o in np.unique(own):
            worst[int(o)] = max(worst.get(int(o), 0.0), float(ratio[own == o].max()))
        checks.append((key, got, r, dec & (v == 0)))
    print("%s: %d of %d points undecided; largest error / bound per owner %s"
          % (name, n_und, n_all, {k: round(v, 4) for k, v in worst.items()}))
    assert n_und <= LC.MAX_UNDECIDED * n_all
    for key, got, r, zero in checks:
        assert np.array_equal(got[zero], np.zeros(zero.sum())), "nonzero where no kept line reaches"
        assert np.all((got >= r.lo) & (got <= r.hi)), (name, key, np.argwhere((got < r.lo) | (got > r.hi))[:4].T)
    assert max(worst.values()) <= 1.0, worst


def test_pair_budget_of_the_module(case):
    assert sum(r.pairs for n in LC.GPU_CASES for r in case(n).restated().values()) <= LC.MAX_PAIRS_MODULE


@pytest.mark.parametrize("name", ["mixed", "osamp", "grid"])
def test_blocks_and_a_batch_give_the_same_bits(case, name):
    from bart_amd import engine, transit_module as trm
    cs = case(name)
    one = _device(cs)
    for n in (5, 2):
        parts = []
        for r in range(n):
            engine.init(cs.c.tcfg, shard=(r, n))
            try:
                assert engine.local_range() == (cs.W * r // n, cs.W * (r + 1) // n)
                parts.append(engine.lbl_extinction(cs.prof))
            finally:
                trm.free_memory()
        got = np.concatenate(parts, axis=1)
        assert np.array_equal(got, one["ext"]), (name, n, np.argwhere(got != one["ext"])[:4].T)
    hot = cs.prof.copy()
    hot[0] *= 1.3
    engine.init(cs.c.tcfg)
    try:
        alone = engine.run_batch(np.array([cs.prof.ravel()]))
        spec = engine.run_batch(np.array([hot.ravel(), hot.ravel() * 1.0, cs.prof.ravel()]))
        st = engine.lbl_states(None)
    finally:
        trm.free_memory()
    assert np.array_equal(spec[2], alone[0])
    L = LC.NLAYERS
    assert st["T"].shape == (3 * L,)
    for k in ("T", "dv", "dop", "lor", "scale", "smax"):
        assert np.array_equal(st[k][2 * L:], one["states"][k]), k
        assert not np.array_equal(st[k][:L], one["states"][k]) or k == "dv"
