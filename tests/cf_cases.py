"""The cases of tests/test_gpu_cf_exact.py, built in one place so that tests/test_cf_exact_cpu.py holds its conditions
(the size of the derived bound, the sensitivity to every mutant) on exactly what the GPU tests run -- TEST
INFRASTRUCTURE ONLY.

A case is a synth.Case with .profs (three walkers), .windows ((idx0, npts, resp, trapz) as bart_amd.cf.filter_windows
returns them), .cols (every grid sample the exact restatement is computed on: the windows' samples and the checked
columns), .checked (the columns of the full output held to the exact value), .rules, .kinds, .decks (cloud tops in
log10 bar, None = no deck), .group and .tag.  Grids are narrow: 130 samples (three tiles, the last of two lanes)
unless the case is about the grid."""
import os

import numpy as np

CHECKED_130 = [0, 1, 31, 62, 63, 64, 65, 127, 128, 129]
LAYERS = (2, 3, 15, 16, 17, 31, 32, 33, 48)
RULES = (0, 1, 2)
CF, TR = 0, 1
ROWS, PITCH = 16, 65


def _resp(n, seed):
    x = np.linspace(0.0, 1.0, n)
    return 0.2 + 0.8 * np.sin(np.pi * x + 0.1 * seed) ** 2


def make_windows(spans, zero_at=()):
    """spans [(first, end)] -> (idx0, npts, resp, trapz); equal spans get equal responses; zero_at: indices into
    `spans` whose response is zero at both ends and at one interior sample."""
    idx0 = np.array([a for a, _ in spans], np.int32)
    npts = np.array([b - a for a, b in spans], np.int32)
    rs = []
    for n, (a, b) in enumerate(spans):
        r = _resp(b - a, a + b)
        if n in zero_at:
            r[0] = r[-1] = r[(b - a) // 2] = 0.0
        rs.append(r)
    trapz = np.array([float(np.sum(0.5 * (r[1:] + r[:-1]))) for r in rs])
    return idx0, npts, np.concatenate(rs), trapz


# a two-sample window, windows ending on lane 63 / 64 and lying across the seam, exactly one tile, the whole grid, the
# partial last tile alone, two identical windows, a response with zeros
SPANS_130 = [(0, 2), (63, 65), (62, 66), (64, 128), (0, 130), (128, 130), (62, 66), (10, 40), (0, 64)]
# narrow windows for the deep columns (W = 70: few exact columns), the partial tile [64, 70) among them
SPANS_70 = [(0, 2), (63, 65), (62, 66), (64, 70)]


def window_list(win):
    idx0, npts, resp, _ = win
    off = np.concatenate([[0], np.cumsum(npts)])
    return [(int(idx0[f]), int(npts[f]), np.asarray(resp[off[f]:off[f + 1]], float)) for f in range(len(idx0))]


def _finish(c, group, tag, win, checked, rules=RULES, kinds=(CF, TR), decks=(None,), seed=3, profs=None):
    from test_gpu_parity import walkers
    c.group, c.tag, c.windows, c.checked, c.rules, c.kinds, c.decks = group, tag, win, list(checked), tuple(rules), tuple(kinds), tuple(decks)
    need = set(c.checked)
    for a, n, _ in window_list(win):
        need |= set(range(a, a + n))
    c.cols = sorted(need)
    c.profs = walkers(c, 3, seed=seed) if profs is None else profs
    return c


def _make(root, name, **kw):
    from bart_amd import synth
    from test_gpu_parity import many_molecules
    kw.setdefault("nwave", 130)
    kw.setdefault("cia", 1)
    nm = kw.pop("many", 4)
    return synth.make_case(os.path.join(root, name), tlow=400.0, thigh=3000.0, tempdelt=650.0, **many_molecules(nm), **kw)


def layer_cases(root):
    """2 .. 48 layers: below, on and past one and two reduction blocks of 16; every rule, both kinds."""
    win = make_windows(SPANS_130, zero_at=(7,))
    return [_finish(_make(root, "L%d" % L, nlayers=L), "layers", "L%d" % L, win, CHECKED_130, seed=L) for L in LAYERS]


def deck_logp(c, k):
    """A cloud top between the pressures of layers k - 1 and k from the top (atm order: bottom first): kend = k."""
    p = c.press_bar[::-1]
    if k <= 0:
        return float(np.log10(p[0]) - 1.0)          # above the top layer: the deck on the top layer
    if k >= len(p):
        return float(np.log10(p[-1]) + 1.0)         # below the bottom layer: no layer reaches it
    return float(0.5 * (np.log10(p[k - 1]) + np.log10(p[k])))


DECK_ROWS = (15, 16, 17, 0, 33)


def deck_cases(root):
    """33 layers, the deck on rows 15, 16 and 17 (the last row of a block, the first of the next, one further), above
    the top layer and below the bottom one."""
    c = _make(root, "deck", nlayers=33, ptop=1e-2)
    win = make_windows([(0, 2), (63, 65), (62, 66), (128, 130)])
    # (absorbers at thirty times their abundance from 0.01 bar down: the column above row 15 is deep enough for the
    # rows to stand above the transmittances' own error -- tests/test_cf_exact_cpu.py holds that)
    return [_finish(c, "deck", "deck", win, CHECKED_130, rules=(0, 1), decks=[deck_logp(c, k) for k in DECK_ROWS],
                    profs=_scaled(c, 30.0, 33))]


def transit_lds(L, M, C, stage=True):
    """Dynamic LDS of cf_transit (csrc/contrib.hip, run_sums): records (staged), pair sums, the reduction block."""
    nc, ni = 4 + 2 * M + 2 * C, 1 + C
    return 8 * ((L * nc + L * ni if stage else 0) + L * 64 + ROWS * PITCH)


def transit_edges(M, C):
    """-> dict tag: (L, expected kernel form or None for the refusal): the last L under 64 kB and the first above it,
    the last staged and the first unstaged, the last that fits and the first refused."""
    first = lambda ok: next(L for L in range(2, 100000) if not ok(L))
    a = first(lambda L: transit_lds(L, M, C) <= 64 * 1024)
    b = first(lambda L: transit_lds(L, M, C) <= 160 * 1024)
    d = first(lambda L: transit_lds(L, M, C, False) <= 160 * 1024)
    return {"staged_last_64k": (a - 1, "cf_transit<staged>"), "staged_first_over_64k": (a, "cf_transit<staged>"),
            "staged_last": (b - 1, "cf_transit<staged>"), "unstaged_first": (b, "cf_transit<unstaged>"),
            "unstaged_last": (d - 1, "cf_transit<unstaged>"), "refused": (d, None)}


def deep_transit_cases(root, M=4, C=1):
    """Four molecules and one CIA file under `cia_interp linear` (one cross-section table: C = 1; the default spline
    counts a file twice): 89, 90, 243, 244, 303 and 304 layers.  The GPU tests recompute the edges from the engine's own
    M and C (bartrt_get_prep_shape) and hold the cases to them.  Transmittance only: the contribution is not defined on
    a transit engine (BARTRT_ENOTSUP, include/bartrt.h; tests/test_gpu_cf.py holds the refusal)."""
    out = []
    win = make_windows(SPANS_70)
    for tag, (L, form) in transit_edges(M, C).items():
        c = _make(root, "tdeep_" + tag, nlayers=L, nwave=70, many=M, cia=C, extra_keys={"solution": "transit", "starrad": 1.145, "cia_interp": "linear"})
        _finish(c, "deep_transit", tag, win, [0, 1, 62, 63, 64, 65, 69], rules=(0,), kinds=(TR,), seed=L)
        c.form = form
        out.append(c)
    return out


def deep_eclipse_cases(root):
    """Nine molecules, three CIA pairs, 300 layers: the records alone are above 64 kB under every rule.  (From 1e-9
    bar down: the bound on a row is the transmittances' 1.5e-13 over the row's largest transmittance STEP, about 0.37
    times a layer's step in ln p; 300 layers over seven decades leave the band rows' bound at 1.2e-11 of their
    maximum, over eleven decades it is inside 1e-11.)"""
    c = _make(root, "edeep", nlayers=300, nwave=70, many=9, cia=3, ptop=1e-9)
    return [_finish(c, "deep_eclipse", "edeep", make_windows(SPANS_70), [0, 1, 62, 63, 64, 65, 69], seed=300)]


def grid_cases(root):
    """577 samples: ten tiles, one full launch group of eight and two in the next; a filter on the first tile and one
    on the grid's last two samples (the last tile holds ONE sample and a window needs two: it spans tiles 8 and 9, so
    seven tiles have no entry).  63, 64 and 65 samples with the whole-grid window."""
    out = [_finish(_make(root, "W577", nlayers=17, nwave=577), "grid", "W577", make_windows([(5, 45), (575, 577)]),
                   [5, 44, 575, 576], rules=(1,), seed=577)]
    for W in (63, 64, 65):
        out.append(_finish(_make(root, "W%d" % W, nlayers=17, nwave=W), "grid", "W%d" % W, make_windows([(0, W)]),
                           sorted({0, 1, 31, 62, W - 1}), rules=(1,), seed=W))
    return out


def zero_cases(root):
    """eclipse_cases.zero_cases: exactly zero extinction in the top band, a middle band and everywhere (30 layers, 70
    samples, no CIA)."""
    import eclipse_cases as ec
    out = []
    for c in ec.zero_cases(root):
        out.append(_finish(c, "zero", "zero_" + c.tag, make_windows(SPANS_70), [0, 15, 31, 62, 63, 64, 69], rules=(0, 1), seed=11))
    return out


def _scaled(c, factor, seed):
    from test_gpu_parity import walkers
    base = walkers(c, 3, seed=seed)
    L, S = len(c.press_bar), len(c.species)
    out = []
    for p in base:
        p = p.reshape(S + 1, L).copy()
        p[3:] = c.abund0.T[2:] * factor
        q = 1 - p[3:].sum(0)
        p[2], p[1] = 0.85 * q, 0.15 * q
        out.append(p.ravel())
    return np.array(out)


THIN_TAU = 1e-10
CLAMP_TAU = 708.0


def extreme_cases(root):
    """thin: every optical depth below 1e-10 (absorbers at 1e-16 of their abundance, no CIA); thick: the depth passes
    708 above the bottom layer, where exp_rt's argument clamps (absorbers at 2e-2 each).  tests/test_cf_exact_cpu.py
    holds both statements on the oracle's depths."""
    win = make_windows(SPANS_70)
    thin = _make(root, "thin", nlayers=17, nwave=70, cia=False)
    thick = _make(root, "thick", nlayers=33, nwave=70)
    return [_finish(thin, "extreme", "thin", win, [0, 31, 63, 64, 69], profs=_scaled(thin, 1e-16, 5)),
            _finish(thick, "extreme", "thick", win, [0, 31, 63, 64, 69], profs=_scaled(thick, 200.0, 6))]


BLOCK_GRIDS = (126, 128, 130)


def block_cases(root):
    """Two ranks: the engine cuts a grid of W samples at W / 2, so 126, 128 and 130 samples put the cut at 63, 64 and
    65 (the issue's 63|67 and 64|66 of ONE 130-sample grid are no split the engine makes).  [63, 65) and [62, 66) lie
    across all three cuts; the whole-grid window and a two-sample window on rank 0 alone go with them.  At 64 the ranks'
    tiles are the unsharded engine's tiles, at 63 and 65 they are not."""
    out = []
    for W in BLOCK_GRIDS:
        c = _make(root, "B%d" % W, nlayers=17, nwave=W)
        win = make_windows([(63, 65), (62, 66), (0, 2), (0, W)])
        out.append(_finish(c, "blocks", "B%d" % W, win, [0, 1, 31, 62, 63, 64, 65, W - 1], rules=(1,), seed=W))
    return out


GROUPS = {"blocks": block_cases, "layers": layer_cases, "deck": deck_cases, "deep_transit": deep_transit_cases, "deep_eclipse": deep_eclipse_cases,
          "grid": grid_cases, "zero": zero_cases, "extreme": extreme_cases}
ABSOLUTE = ("thin", "zero_all")     # held in absolute terms: no value of the row stands above the transmittances' own error


def inf_cfg(c):
    """The case's configuration with `toomuch 1e100` (the oracle's optical depth without a cut)."""
    from bart_amd import synth
    keys = dict(c.keys)
    keys["toomuch"] = "1e100"
    p = os.path.join(c.dir, "inf.cfg")
    if not os.path.exists(p):
        synth.write_tcfg(p, keys)
    return p
