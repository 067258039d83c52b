"""The cases of tests/test_gpu_eclipse_exact.py, built in one place so that tests/test_eclipse_restate_cpu.py holds its
conditions (sensitivity, decidability, non-vacuity of the bound) on exactly what the GPU tests run -- TEST
INFRASTRUCTURE ONLY.

A case is a synth.Case with .profs (its walkers' profiles), .cloudtop (the deck of the `deck` variant), .checked (the
columns of walker 1 held to the exact restatement, tests/eclipse_restate.py) and .mc."""
import os

import mpmath
import numpy as np

import eclipse_restate as er
import transit_restate as tr
from test_gpu_kernel_matrix import GRIDS, MC_LIST, NLAYERS, NWALKERS, NWAVE, TOOMUCH, _case
from test_gpu_parity import walkers

RULES_CUTS = [(rule, cut) for rule in (0, 1, 2) for cut in ("slant", "vertical")]
# the wave seams of 200 samples, and a dozen more (tests/test_eclipse_restate_cpu.py holds their coverage: every parity of
# each ray's last layer, both pad outcomes)
SEAMS = (0, 63, 64, 127, 128, 199)
DOZEN = (7, 21, 38, 50, 77, 90, 101, 115, 140, 155, 170, 186)
CHECKED = sorted(SEAMS + DOZEN)
FOUR_CELLS = [(1, 0), (4, 2), (4, 4), (6, 2)]
LENGTHS = list(range(2, 14)) + list(range(29, 34))
ZERO_BANDS = (("top", slice(-9, None)), ("mid", slice(17, 23)), ("all", slice(None)))     # atm order: index 0 = bottom


def matrix_cases(root, cells=MC_LIST):
    """tests/test_gpu_kernel_matrix.py's cases: 37 layers, 200 samples, two walkers, both ray grids."""
    out = []
    for M, C in cells:
        for g, grid in enumerate(GRIDS):
            c = _case(os.path.join(root, "mc%d_%d_g%d" % (M, C, g)), M, C, grid)
            c.mc, c.grid, c.profs, c.checked = (M, C), g, np.load(os.path.join(c.dir, "p.npy")), CHECKED
            out.append(c)
    return out


def zero_cases(root):
    """Exactly zero extinction in the top band, in a middle band and everywhere, 30 layers, 70 samples (one full wave
    and a partial one: the middle band lies beside the wave seam's columns 63 / 64), no CIA."""
    from bart_amd import synth
    from oracle import rt_oracle as orc
    out = []
    for tag, zero in ZERO_BANDS:
        c = synth.make_case(os.path.join(root, "z" + tag), nlayers=30, nwave=70, cia=False, toomuch=TOOMUCH, ptop=1e-8)
        op = orc.read_opacity(c.opacity)
        k = op["kappa"].copy()
        k[zero] = 0.0
        ids, tg, pr, wnn = op["ids"].copy(), op["temps"].copy(), op["press"].copy(), op["wn"].copy(); del op
        synth.write_opacity(c.opacity, ids, tg, pr, wnn, kappa=k)
        c.mc, c.tag, c.grid = (len(ids), 0), tag, 0
        c.profs = walkers(c, NWALKERS, seed=11)
        np.save(os.path.join(c.dir, "p.npy"), c.profs)
        c.cloudtop = float(np.log10(c.press_bar[30 // 2 - 2]))
        c.checked = [0, 15, 31, 62, 63, 64, 69]
        out.append(c)
    return out


def length_cases(root):
    """2 .. 13 and 29 .. 33 layers on one cell, 20 samples, every column checked."""
    from bart_amd import synth
    from test_gpu_parity import many_molecules
    out = []
    for L in LENGTHS:
        c = synth.make_case(os.path.join(root, "len%d" % L), nlayers=L, nwave=20, toomuch=TOOMUCH, cia=1, tlow=400.0,
                            thigh=3000.0, tempdelt=650.0, **many_molecules(4))
        c.mc, c.grid = (4, 2), 0
        c.profs = walkers(c, NWALKERS, seed=L)
        np.save(os.path.join(c.dir, "p.npy"), c.profs)
        c.cloudtop = float(np.log10(c.press_bar[max(L // 2 - 2, 0)]))
        c.checked = list(range(20))
        out.append(c)
    return out


PATH_GRID = {(1, 0): 0, (4, 2): 1, (4, 4): 0, (6, 2): 1}       # both ray orders among the four cells
PATH_CHECKED = [0, 1, 31, 63, 64, 65, 100, 127, 128, 129]      # 130 samples: three waves, the last of two lanes
WALKER_COUNTS = (1, 2, 10, 26)
SWEEP = [1e-9, 1e-6, 1e-4, 3e-3, 0.05, 0.3, 0.7, 2.0, 5.0, 10.0, 40.0, 300.0, 1e30]      # tests/test_gpu_simpson.py, mode `cuts`
SWEEP_CHECKED = [0, 40, 63, 64, 101, 127, 128, 150, 191, 192, 230, 259]


def path_cases(root):
    """tests/test_gpu_slant_paths.py's three walkers (clear, jump, forest: the single-wave slant kernel's optimistic,
    restart and flagged paths) at 31 layers x 130 samples, `toomuch 10`, on the four cells; .walkers: the walkers held."""
    import test_gpu_slant_paths as sp
    out = []
    for M, C in FOUR_CELLS:
        g = PATH_GRID[M, C]
        c, profs = sp.table_case(os.path.join(root, "path%d_%d" % (M, C)), M, C, GRIDS[g])
        c.mc, c.grid, c.profs, c.checked, c.walkers = (M, C), g, profs, PATH_CHECKED, (sp.CLEAR, sp.JUMPW, sp.FOREST)
        c.cloudtop = sp.deck_logp(c)
        out.append(c)
    return out


def batch_of(n):
    """The walkers of a batch of n, as indices into a path case's three: each kind alone at n = 1 (three batches),
    then cyclic from the jump walker."""
    return [[w] for w in range(3)] if n == 1 else [[(1 + j) % 3 for j in range(n)]]


def sweep_cases(root):
    """One 43-layer column set, 260 samples, under the thirteen values of `toomuch` (one cfg each; .toomuch)."""
    import re
    from bart_amd import synth
    from test_gpu_parity import many_molecules
    base = synth.make_case(os.path.join(root, "sweep"), nlayers=43, nwave=260, cia=1, tlow=400.0, thigh=3000.0,
                           tempdelt=650.0, **many_molecules(4))
    profs = walkers(base, NWALKERS, seed=4)
    np.save(os.path.join(base.dir, "p.npy"), profs)
    txt = open(base.tcfg).read()
    out = []
    for i, tm in enumerate(SWEEP):
        import copy
        c = copy.copy(base)
        c.tcfg = base.tcfg + ".tm%d" % i
        open(c.tcfg, "w").write(re.sub(r"(?m)^toomuch .*$", "toomuch %r" % tm, txt))
        c.mc, c.grid, c.profs, c.checked, c.toomuch, c.tag = (4, 2), 0, profs, SWEEP_CHECKED, tm, "tm%d" % i
        c.cloudtop = float(np.log10(base.press_bar[20]))
        out.append(c)
    return out


def planck_exponents(c1, nu):
    """x[L, nc] mpf = c1_k nu_i, each product exact."""
    with mpmath.workdps(tr.DPS):
        return tr.mp_array(c1)[:, None] * tr.mp_array(nu)[None, :]


def device_columns(c, o, rec, rays):
    """The exact columns of what the device read for walker 1: rec = dict(coef, idx, kstop, wn) of engine.prep_records."""
    cf, v, allow = tr.table_inputs(o, rec["coef"], rec["idx"], c.checked, wn=rec["wn"])
    e, de, _ = tr.extinction(cf, v, allow)
    nu = np.asarray(rec["wn"], float)[c.checked]
    ks = int(rec["kstop"])
    return er.prepare(e, de, rec["coef"][:, 0], planck_exponents(rec["coef"][:, 1], nu), nu, rays, tr.kend_of(ks),
                      bool(ks & tr.DECK_BIT), o.c.toomuch, rec["coef"].shape[0])


def oracle_columns(c, deck, walker=1, toomuch=None, cols=None):
    """The exact columns of the ORACLE's own extinction, radii and temperatures (doubles, each taken exactly) -> (Col,
    oracle engine)."""
    from oracle import rt_oracle as orc
    o = orc.OracleEngine(c.tcfg)
    if toomuch is not None:
        o.c.toomuch = float(toomuch)
    if deck:
        o.set_cloudtop(c.cloudtop)
    prof = np.asarray(c.profs[walker], float).ravel()
    ext, rad = o.extinction(prof)
    L = len(rad)
    kend, found = L - 1, False
    if o.c.has_cloud:
        for k in range(L):
            if o.press[L - 1 - k] >= o.c.cloudtop:
                kend, found = k, True
                break
    cols = c.checked if cols is None else cols
    e = ext[::-1][:, cols]
    r = rad[::-1]
    dr = np.concatenate([[0.0], r[:-1] - r[1:]])
    T = prof[:L][::-1]
    de = np.zeros(e.shape)        # (the oracle's own extinction is the input here, taken exactly: nothing to allow for)
    nu = np.asarray(o.wn, float)[cols]
    with mpmath.workdps(tr.DPS):
        x = (er.mpf(er.K_H) * tr.mp_array(nu)[None, :] * er.mpf(er.K_LS)) / (er.mpf(er.K_KB) * tr.mp_array(T)[:, None])
    rays = er.Rays.from_grid(o.angles, o.c.toomuch)
    return er.prepare(tr.mp_array(e), de, dr, x, nu, rays, kend, found, o.c.toomuch, L), o
