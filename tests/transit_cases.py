"""The cases of tests/test_gpu_transit_matrix.py, built in one place so that tests/test_transit_restate_cpu.py holds
its conditions (sensitivity, decidability, coverage of the cut) on exactly what the GPU tests run -- TEST
INFRASTRUCTURE ONLY.

A case is a synth.Case with .profs (its walkers' profiles), .variants (a list of (tcfg, cloudtop or None,
transparent)), .checked (the columns of walker 1 held to the exact restatement) and .mc."""
import os

import numpy as np

from test_gpu_parity import many_molecules, walkers

TKEYS = {"solution": "transit", "starrad": 1.145}
RSTAR = 1.145 * 6.96e10
# BARTRT_MC_LIST (csrc/kernels.hpp)
MC_LIST = [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2),
           (5, 0), (5, 1), (5, 2), (6, 0), (6, 1), (6, 2), (1, 4), (2, 4), (3, 4), (4, 4), (5, 4), (6, 4)]
EXACT_DEEP = [(1, 0), (4, 2), (6, 4)]         # the cells held to the exact value at 150 and 260 layers
OFF_LIST = [(7, 1), (8, 2), (4, 3)]           # no matrix-tile build: the scalar kernel by default
DEPTHS = (37, 150, 260)                       # KT = 8, 16, 20, each with a partial last tile
W = 70
TOOMUCH_SWEEP = [1e-9, 1e-6, 1e-4, 3e-3, 0.05, 0.3, 0.7, 2.0, 5.0, 10.0, 40.0, 300.0, 1e30]   # tests/test_gpu_simpson.py
SHORT = [(L, 17) for L in (2, 3, 4, 15, 16, 17, 31, 32, 33)] + [(L, 20) for L in (128, 129, 256, 257, 320)]
CHORD_L = (2, 3, 16, 17, 33, 129, 320)


def checked_columns(nwave):
    return sorted({c for c in (0, 15, 16, 63, 64, nwave - 1) if c < nwave})


def _variant(c, tag, **keys):
    from bart_amd import synth
    path = os.path.join(c.dir, "transit_%s.cfg" % tag)
    k = dict(c.keys)
    k.update(keys)
    synth.write_tcfg(path, k)
    return path


def cell_case(d, M, C, L, nwave=W, toomuch=1.0, seed=None, nwalkers=2, **kw):
    """M table molecules and C cross-section tables: C = 0 none, 1 one file under `cia_interp linear`, 2 one file under
    the spline, 3 three files under linear, 4 two files under the spline."""
    from bart_amd import synth
    keys = dict(TKEYS)
    if C in (1, 3):
        keys["cia_interp"] = "linear"
    c = synth.make_case(d, nlayers=L, nwave=nwave, toomuch=toomuch, cia={0: False, 1: 1, 2: 1, 3: 3, 4: 2}[C],
                        tlow=400.0, thigh=3000.0, tempdelt=650.0, extra_keys=keys, **many_molecules(M), **kw)
    c.mc = (M, C)
    c.profs = walkers(c, nwalkers, seed=10 * M + C if seed is None else seed)
    c.checked = checked_columns(nwave)
    return c


def four_variants(c):
    """Without / with a mid-column cloud deck, without / with `transparent`."""
    L = len(c.press_bar)
    # chord 20 of 37; a third of the way down the deeper columns: above the cut of `toomuch 1`, so that columns reach it
    deck = float(np.log10(c.press_bar[L // 2 - 2 if L <= 37 else L - 1 - L // 3]))
    tr = _variant(c, "tr", transparent=1)
    c.variants = [(c.tcfg, None, 0), (c.tcfg, deck, 0), (tr, None, 1), (tr, deck, 1)]
    c.matrix = True
    return c


# A short column from 1e-8 bar: the cut of `toomuch 1` then lies below layer 16 on some checked column of every cell, so
# that a mistake at the first tile seam shows (tests/test_transit_restate_cpu.py, sensitivity)
SHORT_TOP = dict(ptop=1e-8)


def matrix_cases(root, L):
    kw = SHORT_TOP if L == 37 else {}
    return [four_variants(cell_case(os.path.join(root, "m%d_%d_L%d" % (M, C, L)), M, C, L, **kw)) for M, C in MC_LIST]


def off_list_cases(root):
    return [four_variants(cell_case(os.path.join(root, "off%d_%d" % mc), mc[0], mc[1], 37, **SHORT_TOP)) for mc in OFF_LIST]


def exact_here(c):
    """Whether the case's checked columns are held to the exact value: every case but the cells of the 150- and
    260-layer matrix outside EXACT_DEEP (mpmath time)."""
    return not getattr(c, "matrix", False) or len(c.press_bar) <= 37 or c.mc in EXACT_DEEP


SWEEP_SEED = 4


def sweep_case(root):
    """The cut sweep: 50 layers, 130 samples, two molecules and one spline file; thirteen values of toomuch x
    {no deck, a deck in row tile 1, above the top layer (kend = 0), below the bottom} x transparent."""
    c = cell_case(os.path.join(root, "sweep"), 2, 2, 50, nwave=130, seed=SWEEP_SEED)
    lp = np.log10(c.press_bar)             # atm order: index 0 = bottom
    decks = [None, float(lp[50 - 1 - 20]), float(lp.min() - 0.3), float(lp.max() + 0.3)]
    c.variants = []
    for i, tm in enumerate(TOOMUCH_SWEEP):
        for tr in (0, 1):
            cfg = _variant(c, "tm%d_t%d" % (i, tr), toomuch=tm, **({"transparent": 1} if tr else {}))
            c.variants += [(cfg, d, tr) for d in decks]
    return c


def zero_cases(root):
    """Exactly zero extinction in the top layers, everywhere, and in a band in the middle (tests/test_gpu_simpson.py,
    mode `zero`), no CIA; without / with `transparent`."""
    from bart_amd import synth
    from oracle import rt_oracle as orc
    out = []
    for tag, zero in (("top", slice(-9, None)), ("all", slice(None)), ("mid", slice(5, 11))):       # (chords 18 .. 24: beside the tile seam, not on it)
        c = synth.make_case(os.path.join(root, "z" + tag), nlayers=30, nwave=W, cia=False, toomuch=1.0,
                            extra_keys=dict(TKEYS), **SHORT_TOP)
        op = orc.read_opacity(c.opacity)
        k = op["kappa"].copy()
        k[zero] = 0.0                      # atm order: index 0 = bottom
        ids, tg, pr, wnn = op["ids"].copy(), op["temps"].copy(), op["press"].copy(), op["wn"].copy(); del op
        synth.write_opacity(c.opacity, ids, tg, pr, wnn, kappa=k)
        c.mc, c.tag = (4, 0), tag
        c.profs = walkers(c, 2, seed=11)
        c.checked = checked_columns(W)
        c.variants = [(c.tcfg, None, 0), (_variant(c, "tr", transparent=1), None, 1)]
        out.append(c)
    return out


def short_cases(root):
    out = []
    for L, nw in SHORT:
        c = cell_case(os.path.join(root, "s%d" % L), 1, 0, L, nwave=nw, seed=L)
        c.checked = list(range(nw)) if L <= 33 else [0, 16, nw - 1]
        c.variants = [(c.tcfg, None, 0), (_variant(c, "tr", transparent=1), None, 1)]
        out.append(c)
    return out


def chord_cases(root):
    """Eight decades of pressure, and a thin one-decade atmosphere (the worst cancellation in s_{j-1} - s_j)."""
    out = []
    for L in CHORD_L:
        for tag, kw in (("wide", dict(ptop=1e-6, pbottom=100.0)), ("thin", dict(ptop=1e-2, pbottom=1e-1))):
            c = cell_case(os.path.join(root, "c%d_%s" % (L, tag)), 1, 0, L, nwave=17, seed=L, **kw)
            c.tag = tag
            out.append(c)
    return out


def oracle_inputs(c, variant, walker=1):
    """-> (o, e[L, W] doubles from the top, r[L] top to bottom, kend): the oracle's own extinction and radii of one
    walker under a variant (tcfg, cloudtop, transparent)."""
    from oracle import rt_oracle as orc
    tcfg, deck, _ = variant
    o = orc.OracleEngine(tcfg)
    if deck is not None:
        o.set_cloudtop(deck)
    ext, rad = o.extinction(c.profs[walker])
    L = len(rad)
    kend = L - 1
    if o.c.has_cloud:
        for k in range(L):
            if o.press[L - 1 - k] >= o.c.cloudtop:
                kend = k
                break
    return o, ext[::-1].copy(), rad[::-1].copy(), kend


def oracle_column(c, variant, cols=None, walker=1, chords=None):
    """The exact column of the oracle's own extinction and radii (doubles, each taken exactly) on the columns `cols`
    (default: the case's checked ones) -> (transit_restate column, oracle engine, Chords).  The extinction's bound is
    the kernels' operation count on |e| (the oracle's terms are not visible from here; all are positive but the
    spline's curvature terms) plus 64 u, which stands in for the input allowance of the resampled CIA planes."""
    import transit_restate as tr
    o, e, r, kend = oracle_inputs(c, variant, walker)
    cols = c.checked if cols is None else cols
    ch = chords or tr.Chords(r)
    M, C = c.mc
    A = np.abs(e[:, cols])
    de = (2 * M + 2 * C + 2 + 4 + 64) * tr.U * A
    col = tr.columns(tr.mp_array(e[:, cols]), de, A, ch, kend, o.c.toomuch, o.c.transparent, o.c.starrad)
    return col, o, ch
