"""Each line-by-line accumulation kernel (csrc/lbl.hip) held to the oracle on the points it owns.

Four kernels turn a line list into extinction; `sv[1] > 1`, narrow_state and mid_state decide ON THE DEVICE which of
them writes a (layer state, 256-point tile), and nobody clears the output first.  tests/lbl_owner_restate.py restates
the rule on the oracle's half-widths; here

  owners     every case asserts on the CPU that no decision lies within 1e-6 of its threshold and that the owners it
             claims occur, then engine.lbl_owners (the device's own predicates) must equal the prediction byte for
             byte, with no tile unowned (255) or owned twice (bit 7)
  parity     engine.lbl_extinction against lbl_oracle separately on the points of each owner, with the absolute floor
             1e-13 of the (state, tile)'s OWN oracle maximum instead of the whole array's, and exact zeros where the
             oracle has no line in reach
  stale      a hot, dense profile first (one walker, then three), then the case's profile on the same engine: the bits
             of a fresh engine's single call -- an unowned tile would keep the first call's numbers
  flip       a Doppler-dominated layer whose temperature is bisected on the predictor so that it sits on narrow_state's
             threshold inside the grid: halving the grid moves the tile boundaries, >= 64 points change between the pair
             kernel and the tile kernel, and the blocks must still be the unsharded bits
  rounds     the pair kernel's queue at its edges, each counted on the host from the oracle's line ranges before the
             run: a wave with more than 128 queued lines (the ring wraps), rounds of more than 240 pairs (split, lines
             left queued), a 64-line window without a kept line between two with, a line centred beyond the grid's
             end, and lines that reach 63 and 64 points of the grid, slack included.  2 * 31 + 3 = nmax itself cannot
             occur in a state the pair kernel owns: narrow_state holds the widest cut to 31 / 1.011 spacings and to
             31 exactly only AT the threshold, so at most 62 points lie inside a cut; the test asserts that no line of
             the case exceeds nmax and that 63 and 64 are reached.

All cases: 12 layers, 700 wavenumbers (two whole tiles and a ragged one of 188 points = two whole waves and one of 60),
at most 1 500 lines, plus the mixed column at 1, 2, 256, 257 and 513 wavenumbers (narrow_state's `ilast <= tile0` branch
and one-point last tiles; the engine refuses a one-point grid, so 1 is the second block of the two-point grid halved).
The oracle (scipy's wofz) runs once per case and is shared by the tests of the module.

Pytest durations on an MI355X: 1.7 s for the module; every test below 0.5 s."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lbl_owner_restate as R

pytestmark = pytest.mark.gpu

RTOL = 1e-7              # the oracle comparison's tolerance (tests/test_lbl.py), kept as it stands: NOT the accuracy of
                         # voigt_k, which lbl.hip puts at 3e-13 .. 1.4e-11 per branch and tests/test_gpu_voigt_exact.py
                         # and tests/test_gpu_lbl_exact.py hold against mpmath under a derived bound
FLOOR = 1e-13            # of the (state, tile)'s own oracle maximum
SHARP = 1e-6
NLAYERS, NWAVE = 12, 700
FINE = 0.0042            # cm-1: 20 Doppler half-widths x 1.011 of H2O at 1450 K and 2000 cm-1 are 31 of these
FLIP_LAYER = 9           # 1.9e-5 bar: Doppler-dominated
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "doppler": dict(kw=dict(ptop=1e-6, pbottom=1e-3), owners={R.PAIRS}),
    "pressure": dict(kw=dict(ptop=1.0, pbottom=100.0, wndelt=0.02), owners={R.TILE_K}),
    "mixed": dict(kw=dict(ptop=1e-6, pbottom=100.0, wndelt=FINE), owners={R.TILE_K, R.PAIRS}),
    "osamp": dict(kw=dict(ptop=1e-6, pbottom=100.0, wnosamp=90), owners={R.TILE_K, R.FINE_OVER}),
    "grid": dict(kw=dict(ptop=1e-5, pbottom=100.0, extra_keys=dict(voigt="grid")), owners={R.GRID}),
    "mid": dict(kw=dict(ptop=0.1, pbottom=10.0), owners={R.TILE_K, R.PAIRS, R.FINE_MID}, mid_reach=48),
    "rounds": dict(kw=dict(ptop=1e-6, pbottom=1e-3, wndelt=FINE), owners={R.PAIRS}),
}
for _n in (2, 256, 257, 513):
    CASES["mixed%d" % _n] = dict(kw=dict(ptop=1e-6, pbottom=100.0, wndelt=FINE, nwave=_n), owners=None)
# (the engine refuses a grid of one point: a block of one point is the second half of the two-point grid)
CASES["mixed1"] = dict(kw=dict(ptop=1e-6, pbottom=100.0, wndelt=FINE, nwave=2), owners=None, shard=(1, 2))
IN_PROCESS = [n for n in CASES if n != "mid"]


def _narrow_limit(o, prof, layer, wn, ilast):
    """Temperature of `layer` at which narrow_state's cany equals its threshold for a tile ending at point `ilast`:
    bisection ON THE PREDICTOR (a tile of its own, so only this threshold is asked)."""
    def narrow(T):
        p = prof.copy()
        p[0, layer] = T
        one = np.asarray(wn[max(ilast - 255, 0):ilast + 1])
        return R.predict(o, p[:, layer:layer + 1], wn=one, voigt_grid=False)[0][0, 0] == R.PAIRS
    o_press = o.press
    o.press = o.press[layer:layer + 1]
    try:
        lo, hi = 800.0, 3000.0
        assert narrow(lo) and not narrow(hi)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if narrow(mid) else (lo, mid)
    finally:
        o.press = o_press
    return lo


def _craft_rounds(c, o, prof):
    """The line list of the `rounds` case: the synthetic lists plus, in the first database, two blocks of 100 strong
    lines inside wave 1 with 130 lines far below the strength threshold between them, a line centred beyond the last
    grid point, one centred on a grid point and one half-way between two."""
    from bart_amd import synth
    wn = o.wn
    db = c.linedbs[0]
    rng = np.random.default_rng(5)
    mid = 0.5 * (wn[95] + wn[96])
    dense = np.concatenate([rng.uniform(wn[66], mid - 0.01, 100), rng.uniform(mid + 0.01, wn[125], 100)])
    weak = mid + np.linspace(-1e-4, 1e-4, 130)
    special = np.array([wn[-1] + 0.05, wn[600], 0.5 * (wn[660] + wn[661])])
    add = lambda key, vals: db.__setitem__(key, np.concatenate([np.asarray(db[key]), vals]))
    add("wn", np.concatenate([dense, weak, special]))
    add("iso", np.zeros(333, int))
    add("elow", np.concatenate([rng.uniform(100.0, 1500.0, 200), np.full(130, 8000.0), np.full(3, 300.0)]))
    add("gf", np.concatenate([10 ** rng.uniform(-4.0, -2.0, 200), np.full(130, 1e-12), np.full(3, 1e-2)]))
    synth.write_tli(c.tli, c.linedbs, wn[0] - 30.0, wn[-1] + 30.0)


class Case:
    """Inputs, oracle, prediction and (lazily) the oracle's extinction of one case."""

    def __init__(self, name, root):
        from bart_amd import synth_lbl
        from oracle import lbl_oracle
        spec = CASES[name]
        kw = dict(nlines=500 if name == "rounds" else 750, nwave=NWAVE, nlayers=NLAYERS)
        kw.update(spec["kw"])
        self.name, self.claims, self.mid_reach = name, spec["owners"], spec.get("mid_reach", 0)
        self.shard = spec.get("shard")
        self.c = synth_lbl.make_lbl_case(os.path.join(root, name), **kw)
        self.o = lbl_oracle.LblOracle(self.c.tcfg)
        if self.shard:
            r, n = self.shard
            W = len(self.o.wn)
            self.o = lbl_oracle.LblOracle(self.c.tcfg, wn_slice=(W * r // n, W * (r + 1) // n))
        self.prof = self.c.profiles()
        if name.startswith("mixed"):
            # a hot Doppler-dominated layer on top (the tile kernel on Doppler cores), and FLIP_LAYER on
            # narrow_state's threshold between points 511 and 605: the pair kernel's in tiles 0 and 1, the tile
            # kernel's in tile 2 -- and, when the grid is halved at point 350, from point 350 on
            full = self.o.wn_first + FINE * np.arange(NWAVE)
            t511, t605 = (_narrow_limit(self.o, self.prof, FLIP_LAYER, full, i) for i in (511, 605))
            assert t605 < t511
            self.prof[0, FLIP_LAYER] = np.sqrt(t511 * t605)
            self.prof[0, NLAYERS - 1] = 1900.0
        if name == "rounds":
            # layer 6 a little below the threshold of the last tile: its cuts span 30.6 spacings there
            self.prof[0, 6] = _narrow_limit(self.o, self.prof, 6, self.o.wn, NWAVE - 1) * (1.0 - 0.004)
            _craft_rounds(self.c, self.o, self.prof)
            self.o = lbl_oracle.LblOracle(self.c.tcfg)
        assert sum(len(db["wn"]) for db in self.o.dbs) <= 1500
        self.W = len(self.o.wn)
        self.owners, self.margin = R.predict(self.o, self.prof, mid_reach=self.mid_reach)
        self._ref = None
        self.dev = None          # (owner map, extinction) of a fresh engine's single call

    def block(self, r, n):
        """Oracle and prediction of block r of n of the grid."""
        from oracle import lbl_oracle
        lo, hi = self.W * r // n, self.W * (r + 1) // n
        o = lbl_oracle.LblOracle(self.c.tcfg, wn_slice=(lo, hi))
        return (lo, hi), R.predict(o, self.prof, mid_reach=self.mid_reach)

    @property
    def ref(self):
        if self._ref is None:
            self._ref = self.o.extinction(self.prof)
            self._ref.setflags(write=False)
        return self._ref

    def hot(self):
        """A hot, dense profile: every temperature x 1.5, the absorbers fifty times as abundant."""
        p = self.prof.copy()
        p[0] *= 1.5
        for db in self.o.dbs:
            p[1 + self.o.species.index(db["molecule"])] *= 50.0
        return p

    def sharp(self):
        assert self.margin.min() > SHARP, (self.name, self.margin.min())
        have = set(np.unique(self.owners))
        if self.claims is not None:
            assert have == self.claims, (self.name, have)
        assert have <= {R.TILE_K, R.PAIRS, R.FINE_OVER, R.FINE_MID, R.GRID}


_cases = {}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("lbl_owners"))

    def get(name):
        if name not in _cases:
            _cases[name] = Case(name, root)
        return _cases[name]
    return get


def _fresh(cs):
    """Owner map and extinction of a fresh engine's single call (run once per case)."""
    from bart_amd import engine, transit_module as trm
    if cs.dev is None:
        assert cs.mid_reach == 0
        engine.init(cs.c.tcfg, shard=cs.shard)
        try:
            assert engine.local_range()[1] - engine.local_range()[0] == cs.W
            cs.dev = (engine.lbl_owners(cs.prof), engine.lbl_extinction(cs.prof))
        finally:
            trm.free_memory()
    return cs.dev


def _check_owners(cs, got, want=None):
    want = cs.owners if want is None else want
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert not (got == R.NONE).any(), "a (state, tile) no kernel claims: %s" % (np.argwhere(got == R.NONE)[:4],)
    assert not (got & R.MULTI).any(), "a (state, tile) claimed twice: %s" % (np.argwhere(got & R.MULTI)[:4],)
    assert np.array_equal(got, want), (cs.name, got.T, want.T)


def _check_parity(cs, ext, ref=None, owners=None):
    """ext against the oracle, owner by owner: |ext - ref| <= RTOL |ref| + FLOOR max(ref[state, tile]); exact zeros
    where the oracle's are.  Prints the largest error / bound per owner."""
    ref = cs.ref if ref is None else ref
    owners = cs.owners if owners is None else owners
    assert ext.shape == ref.shape and np.all(np.isfinite(ext))
    W = ref.shape[1]
    pad = np.zeros((ref.shape[0], owners.shape[1] * R.TILE))
    pad[:, :W] = ref
    tmax = np.repeat(pad.reshape(ref.shape[0], -1, R.TILE).max(axis=2), R.TILE, axis=1)[:, :W]
    bound = RTOL * np.abs(ref) + FLOOR * tmax
    err = np.abs(ext - ref)
    pts = R.point_owners(owners, W)
    worst = {}
    for code in np.unique(pts):
        m = pts == code
        assert ref[m].max() > 0 or cs.claims is None, (cs.name, code)      # (a two-point grid may lie between the lines)
        pos = m & (bound > 0)
        worst[int(code)] = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0     # (all zero: held exactly below)
        print("%s owner %d: %d points, largest error / bound %.3g" % (cs.name, code, m.sum(), worst[int(code)]))
    zero = ref == 0
    assert np.array_equal(ext[zero], ref[zero]), "nonzero where no line is in reach"
    assert (err <= bound).all(), (cs.name, worst)
    return worst


@pytest.mark.parametrize("name", IN_PROCESS)
def test_owners_as_predicted_and_parity_per_owner(case, name):
    cs = case(name)
    cs.sharp()                                   # on the oracle's numbers, before anything runs on the device
    if name == "rounds":
        _rounds_claims(cs)
    own, ext = _fresh(cs)
    _check_owners(cs, own)
    _check_parity(cs, ext)


def test_mid_reach_owner_in_a_child_process(case, tmp_path):
    """BARTRT_MID_REACH is read once per process: a child of its own."""
    cs = case("mid")
    cs.sharp()
    f = lambda n: str(tmp_path / n)
    np.save(f("p.npy"), cs.prof)
    code = ("import numpy as np, sys; sys.path.insert(0, %r)\n"
            "from bart_amd import engine, transit_module as trm\n"
            "p = np.load(%r); engine.init(%r)\n"
            "np.save(%r, engine.lbl_owners(p)); np.save(%r, engine.lbl_extinction(p)); trm.free_memory()\n"
            % (ROOT, f("p.npy"), cs.c.tcfg, f("own.npy"), f("ext.npy")))
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, BARTRT_MID_REACH="48"), timeout=120)
    _check_owners(cs, np.load(f("own.npy")))
    _check_parity(cs, np.load(f("ext.npy")))


@pytest.mark.parametrize("walkers", [1, 3])
@pytest.mark.parametrize("name", ["mixed", "osamp"])
def test_no_stale_output(case, name, walkers):
    """Nobody clears the output: after a call that filled it with other numbers (three walkers: a larger region than
    the second call's), every point must be written again -- the bits of a fresh engine's single call."""
    from bart_amd import engine, transit_module as trm
    cs = case(name)
    cs.sharp()
    _, fresh = _fresh(cs)
    hot = cs.hot()
    engine.init(cs.c.tcfg)
    try:
        if walkers == 1:
            first = engine.lbl_extinction(hot)
            assert (first != fresh)[fresh > 0].all()      # what a hole would keep is not the answer
        else:
            spec = engine.run_batch(np.array([hot.ravel()] * walkers))
            assert np.all(np.isfinite(spec))
        again = engine.lbl_extinction(cs.prof)
    finally:
        trm.free_memory()
    assert np.array_equal(again, fresh), np.argwhere(again != fresh)[:4]


def test_points_that_change_owner_keep_their_bits(case):
    """lbl_accumulate: "a state may change owner between two tilings of the grid -- the bits must not"."""
    from bart_amd import engine, transit_module as trm
    cs = case("mixed")
    cs.sharp()
    whole = R.point_owners(cs.owners, cs.W)
    blocks = [cs.block(r, 2) for r in range(2)]
    assert all(m.min() > SHARP for _, (_, m) in blocks)
    halves = np.concatenate([R.point_owners(own, hi - lo) for (lo, hi), (own, _) in blocks], axis=1)
    moved = (whole[FLIP_LAYER] != halves[FLIP_LAYER])
    assert set(zip(whole[FLIP_LAYER][moved], halves[FLIP_LAYER][moved])) <= {(R.PAIRS, R.TILE_K), (R.TILE_K, R.PAIRS)}
    print("mixed: %d points of layer %d change owner between the whole grid and its halves (all layers: %d)"
          % (moved.sum(), FLIP_LAYER, (whole != halves).sum()))
    assert moved.sum() >= 64
    own, ext = _fresh(cs)
    _check_owners(cs, own)
    parts = []
    for r, ((lo, hi), (want, _)) in enumerate(blocks):
        assert lo % R.TILE or hi % R.TILE
        engine.init(cs.c.tcfg, shard=(r, 2))
        try:
            assert engine.local_range() == (lo, hi)
            _check_owners(cs, engine.lbl_owners(cs.prof), want)
            parts.append(engine.lbl_extinction(cs.prof))
        finally:
            trm.free_memory()
    got = np.concatenate(parts, axis=1)
    diff = got != ext
    assert not diff.any(), ("layers %s: %d points, %d of them among those that changed owner"
                            % (np.unique(np.nonzero(diff)[0]), diff.sum(), (diff & (whole != halves)).sum()))


def _rounds_claims(cs):
    """The `rounds` case reaches the pair kernel's edges: counted from the oracle's line ranges."""
    o, prof = cs.o, cs.prof
    cool, near = R.pair_rounds(o, prof, 3), R.pair_rounds(o, prof, 6)
    for waves in (cool, near):
        assert all(w["reach"].max() <= R.NMAX for w in waves if len(w["reach"]))
    # the ring wraps: more lines pass through a wave's queue than it has slots
    queued = max(len(w["n"]) for w in cool)
    assert queued > R.RING
    # rounds that split: 64 lines looked at, fewer taken, and never more than kPairCap pairs
    rounds = [r for waves in (cool, near) for w in waves for r in w["rounds"]]
    split = [r for r in rounds if r[1] < r[0]]
    assert split and max(r[2] for r in rounds) <= R.PAIR_CAP and any(r[0] == 64 for r in split)
    most = max(sum(w["n"][:64]) for w in cool if len(w["n"]) >= 64)
    assert most > R.PAIR_CAP
    # the widest lines a narrow state can hold: 61 and 62 points inside the cut, one of slack either side
    reach = np.concatenate([w["reach"] for w in near])
    assert (reach == 2 * R.PAIR_REACH + 1).any() and (reach == 2 * R.PAIR_REACH + 2).any()
    # a line centred beyond the last grid point whose cut reaches back into the last, ragged wave
    last = o.wn[-1]
    assert cs.W % 64 and any(((nu0 > last) & (nu0 - cut <= last - o.wndelt)).any()
                             for nu0, cut in R.kept_lines(o, prof[0, 3], o.press[3], prof[1:, 3]))
    # a window of 64 lines none of which is kept, between two with kept lines that reach wave 1: a run of 127 such
    # lines holds a whole window wherever the windows start
    db = o.dbs[0]
    S, aD, aL = o._strengths(db, prof[0, 3], o.press[3], prof[1:, 3], False)
    keep = (S >= o.ethresh * S.max()) & (S > 0)
    cut = o.nwidth * np.maximum(aD, aL)
    in_wave = keep & (db["wn"] + cut >= o.wn[64]) & (db["wn"] - cut <= o.wn[127])
    idx = np.nonzero(in_wave)[0]
    gaps = np.diff(idx) - 1
    assert gaps.max() >= 127 and not keep[idx[gaps.argmax()] + 1: idx[gaps.argmax() + 1]].any()
    print("rounds: %d lines queued in one wave, %d rounds of which %d split, most pairs offered to a round %d, "
          "widest reach %d points" % (queued, len(rounds), len(split), most, reach.max()))
