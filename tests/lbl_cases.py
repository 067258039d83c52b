"""The cases tests/test_lbl_restate_cpu.py and tests/test_gpu_lbl_exact.py share: small line-by-line input sets built to
reach every accumulation kernel of csrc/lbl.hip and the edges of lbl_states, each with its exact restatement
(tests/lbl_restate.py) computed once per process.

Shapes: six layers, W = 321 points (one whole 256-point tile and a ragged one of 65 = one whole wave and one point), two
databases (H2O with two isotopes on four temperature nodes, CO with one), at most 120 lines; between them the layers
span 1e-6 .. 100 bar.  mpmath's w(z) costs 0.5 - 3 ms, so every case stays at or below 15 000 (line, point) pairs
(counted by the restatement, asserted by the CPU test) and the list GPU_CASES below 60 000.

  doppler   1e-6 .. 1e-3 bar: the pair kernel.  CO on ONE temperature node; the strongest H2O line 25 cm-1 beyond the
            grid, out of reach of every point (the threshold comes from a line that contributes nothing)
  pressure  1 .. 100 bar: the tile kernel, every branch of voigt_k out to voigt_far
  mixed     1e-6 .. 100 bar on a fine grid: tile and pair kernel; T below the first partition-function node (450 K),
            on a node (1000 K) and above the last (2300 K)
  osamp     wnosamp 12, nwidth 6, the spacing chosen on the oracle's widths so that an odd (3) and, in the top layer cooled to 600 K,
            an even divisor (4) occur: the line-major kernel, and the tile kernel below
  grid      voigt grid: the width-grid kernel
  mid       0.1 .. 7.5 bar under BARTRT_MID_REACH=48 (a child process): the line-major kernel's mid-reach walk
  y0        no H2 and no He among the species: aL = 0, y = 0 in every kernel
  table     opacity per gram through the opacity-grid generator (nodes 1000 and 1100 K; the first one is restated)

Every list carries a line centred on a grid point, one exactly half-way between two (except `grid`, where the centre's
nearest sampling point would be undecided over the line's whole reach), one beyond each end of the grid within
reach, weak lines far below the strength threshold, and a line whose lower-state energy drives the exponent under
kExpMin."""
from __future__ import annotations

import os

import numpy as np

import lbl_owner_restate as R
import lbl_restate as X

NLAYERS, NWAVE = 6, 321
TEMPS = np.array([500.0, 1000.0, 1500.0, 2000.0])
FINE = 0.0042
SHARP = 1e-6
MAX_PAIRS, MAX_PAIRS_MODULE = 15000, 60000
MAX_UNDECIDED = 0.02

CASES = {
    "doppler": dict(kw=dict(ptop=1e-6, pbottom=1e-3), nstrong=40, owners={R.PAIRS}, one_node=True, far_strong=True),
    "pressure": dict(kw=dict(ptop=1.0, pbottom=100.0, wndelt=0.02), nstrong=2, owners={R.TILE_K}, few_edges=True),
    "mixed": dict(kw=dict(ptop=1e-6, pbottom=100.0, wndelt=FINE), nstrong=3, owners={R.TILE_K, R.PAIRS},
                  temps={5: 450.0, 4: 1000.0, 3: 2300.0}),
    "osamp": dict(kw=dict(ptop=1e-6, pbottom=100.0, wnosamp=12, nwidth=6), nstrong=3, owners={R.TILE_K, R.FINE_OVER},
                  tune_dv=True, temps={5: 600.0}),
    "grid": dict(kw=dict(ptop=1e-5, pbottom=100.0, extra_keys=dict(voigt="grid")), nstrong=4, owners={R.GRID},
                 no_half=True),
    "mid": dict(kw=dict(ptop=0.1, pbottom=7.5), nstrong=4, owners={R.TILE_K, R.PAIRS, R.FINE_MID}, mid_reach=48),
    "y0": dict(kw=dict(ptop=1e-6, pbottom=100.0, species=("CO", "CO2", "CH4", "H2O"), abund=(0.3, 0.3, 0.2, 0.2)),
               nstrong=40, owners={R.PAIRS}, far_strong=True),
    "table": dict(kw=dict(ptop=1e-4, pbottom=1.0, with_table=True, tlow=1000.0, thigh=1100.0, tempdelt=100.0),
                  nstrong=6, owners=None, per_gram=True),
}
GPU_CASES = list(CASES)


def line_lists(wn, spec, seed):
    """The two databases of a case on the grid `wn` (module docstring)."""
    rng = np.random.default_rng(seed)
    d = wn[1] - wn[0]
    n = spec["nstrong"]
    z = lambda mass_ratio: 50.0 * mass_ratio * (TEMPS / 296.0) ** 1.5
    dbs = []
    for k, (mol, mass) in enumerate((("H2O", 18.01528), ("CO", 28.0101))):
        one = spec.get("one_node") and k == 1
        temps = TEMPS[1:2] if one else TEMPS
        isos = [dict(name="%s_%d" % (mol, i + 1), mass=mass + i, ratio=r, Z=(z(1 + 0.1 * i)[1:2] if one else z(1 + 0.1 * i)))
                for i, r in (((0, 0.98), (1, 0.02)) if k == 0 else ((0, 1.0),))]
        cen = list(rng.uniform(wn[0] - d, wn[-1] + d, n))
        gf = list(10 ** rng.uniform(-3.0, -2.0, n))
        elow = list(rng.uniform(100.0, 1500.0, n))
        # weak lines far below any threshold, and one whose exponent falls under kExpMin
        cen += list(rng.uniform(wn[0], wn[-1], 6)) + [float(wn[150]) + 0.3 * d]
        gf += [1e-12] * 6 + [0.1]
        elow += [8000.0] * 6 + [1.0e6]
        if k == 0:
            cen += [float(wn[100])]
            if not spec.get("no_half"):
                cen += [0.5 * (float(wn[200]) + float(wn[201]))]
            if not spec.get("few_edges"):
                cen += [float(wn[0]) - 1.5 * d, float(wn[-1]) + 1.5 * d]
            m = len(cen) - len(gf)
            gf += [5e-3] * m
            elow += [300.0] * m
            if spec.get("far_strong"):
                cen += [float(wn[-1]) + 25.0]
                gf += [1.0]
                elow += [100.0]
        elif spec.get("far_strong"):
            # kept at 1e-5 of CO's own strongest line; a threshold taken over both databases (H2O's far line is a
            # hundred times stronger) would drop it
            cen += [float(wn[50]) + 0.2 * d]
            gf += [1e-7]
            elow += [300.0]
        iso = rng.choice(len(isos), len(cen), p=[0.7, 0.3] if k == 0 else [1.0])
        dbs.append(dict(name="exact_%s" % mol, molecule=mol, temps=temps, isotopes=isos, wn=np.array(cen),
                        iso=iso, elow=np.array(elow), gf=np.array(gf)))
    return dbs


def setup_of(o):
    """lbl_restate.Setup from the inputs an LblOracle has read (arrays only; none of its formulas)."""
    dbs = []
    for db in o.dbs:
        keep = (db["wn"] >= o.wn_first - 500.0) & (db["wn"] <= o.wn_last + 500.0)
        dbs.append(dict(sp=o.species.index(db["molecule"]), temps=np.asarray(db["temps"]),
                        isotopes=[(i["mass"], i["ratio"], np.asarray(i["Z"])) for i in db["isotopes"]],
                        wn=db["wn"][keep], iso=db["iso"][keep], elow=db["elow"][keep], gf=db["gf"][keep]))
    grid = None
    if o.voigt == "grid":
        grid = dict(dgrid=o.dgrid, lgrid=o.lgrid, d_ln0=float(o.d_ln0), d_dln=float(o.d_dln), l_ln0=float(o.l_ln0),
                    l_dln=float(o.l_dln))
    sp = o.species
    return X.Setup(press=o.press, mass=o.mass, diam=o.diam, iH2=sp.index("H2") if "H2" in sp else -1,
                   iHe=sp.index("He") if "He" in sp else -1, dbs=dbs, nwidth=o.nwidth, ethresh=o.ethresh, wn=o.wn,
                   wn_first=float(o.wn_first), wndelt=float(o.wndelt), wfull=len(o.wn), osamp=o.osamp, grid=grid)


class Case:
    def __init__(self, name, root):
        from bart_amd import synth, synth_lbl
        from oracle import lbl_oracle
        spec = CASES[name]
        self.name, self.spec = name, spec
        self.claims, self.mid_reach, self.per_gram = spec["owners"], spec.get("mid_reach", 0), spec.get("per_gram", False)
        kw = dict(nlines=10, nwave=NWAVE, nlayers=NLAYERS)
        kw.update(spec["kw"])
        d = os.path.join(root, name)
        c = synth_lbl.make_lbl_case(d, **kw)
        if spec.get("tune_dv"):
            # the spacing at which the 0.063 bar layer takes dv = 3: wndelt / 3 <= wmin / 2 < wndelt / 2
            o = lbl_oracle.LblOracle(c.tcfg)
            prof = c.profiles()
            dop, lor = R.state_widths(o, prof[0, 2], o.press[2], prof[1:, 2])
            wmin = float(np.min(np.maximum(o.wn_first * dop, lor)))
            kw["wndelt"] = float("%.5f" % (1.25 * wmin))
            c = synth_lbl.make_lbl_case(d, **kw)
        wn = c.wn
        c.linedbs = line_lists(wn, spec, seed=len(name) + 11)
        assert sum(len(db["wn"]) for db in c.linedbs) <= 120
        synth.write_tli(c.tli, c.linedbs, wn[0] - 30.0, wn[-1] + 30.0)
        self.c = c
        self.o = lbl_oracle.LblOracle(c.tcfg)
        assert np.array_equal(self.o.wn, wn) and len(wn) == NWAVE
        self.prof = c.profiles()
        for l, T in spec.get("temps", {}).items():
            self.prof[0, l] = T
        self.su = setup_of(self.o)
        self.W = NWAVE
        self.owners, self.margin = R.predict(self.o, self.prof, mid_reach=self.mid_reach)
        self._res = {}

    def sharp(self):
        """The owners the case is meant to exercise occur, no ownership decision within SHARP of its threshold."""
        assert self.margin.min() > SHARP, (self.name, self.margin.min())
        if self.claims is not None:
            assert set(np.unique(self.owners)) == self.claims, (self.name, set(np.unique(self.owners)))

    def states(self):
        """(T, p, q) per restated state: the profile's layers, or the atmosphere file's at the table's one temperature."""
        if self.per_gram:
            return [(1000.0, self.o.press[l], self.o.abund0[l]) for l in range(NLAYERS)]
        return [(self.prof[0, l], self.o.press[l], self.prof[1:, l]) for l in range(NLAYERS)]

    def restated(self, mutant=None, layers=None, fad=None):
        """{layer: Result} (per_gram: {(layer, group): Result}); the unmutated one is computed once and shared."""
        key = mutant
        if key in self._res and layers is None:
            return self._res[key]
        fad = self.fad if fad is None else fad
        rs = X.Restatement(self.su, mutant, fad)
        out = {}
        for l, (T, p, q) in enumerate(self.states()):
            if layers is not None and l not in layers:
                continue
            if self.per_gram:
                for g in range(len(self.su.dbs)):
                    out[(l, g)] = rs.layer(T, p, q, True, groups=[g])
            else:
                out[l] = rs.layer(T, p, q)
        if layers is None:
            self._res[key] = out
        return out

    @property
    def fad(self):
        if not hasattr(self, "_fad"):
            self._fad = X.Faddeeva()
        return self._fad

    def restated_states(self):
        rs = X.Restatement(self.su)
        return [rs.state(T, p, q, self.per_gram) for (T, p, q) in self.states()]


_cases = {}


def get(name, root):
    if name not in _cases:
        _cases[name] = Case(name, root)
    return _cases[name]
