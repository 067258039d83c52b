"""Which accumulation kernel owns a (layer state, 256-point tile) of the line-by-line path, restated in numpy.

csrc/lbl.hip decides the owner on the device: `sv[1] > 1` (an oversampled state), `narrow_state` (every cut
reaches at most kPairReach points of this tile) and `mid_state` (BARTRT_MID_REACH).  This module restates the
three on the ORACLE's numbers -- the Doppler and Lorentz half-widths of oracle/lbl_oracle.py and its
oversampling divisor -- so that a test can say, before anything runs on the device, which kernel has to write
which points, and how far every decision lies from its threshold.  It also restates how the pair kernel
queues lines and cuts its rounds (`pair_rounds`), from the oracle's line ranges.

Owner codes (engine.lbl_owners): 0 lbl_accumulate, 1 lbl_accumulate_pairs, 2 lbl_accumulate_fine
(oversampled), 3 lbl_accumulate_fine (mid reach), 4 lbl_accumulate_grid, 255 none; bit 7: more than one."""
from __future__ import annotations

import numpy as np

from oracle.lbl_oracle import AMU, KB, LS

TILE = 256
PAIR_REACH = 31          # kPairReach
PAIR_CAP = 240           # kPairCap
RING = 128               # slots of the pair kernel's queue
NMAX = 2 * PAIR_REACH + 3
DOPPLER_SLACK = 1.011    # narrow_state / mid_state: the Doppler width at the tile's last point, with margin
TILE_K, PAIRS, FINE_OVER, FINE_MID, GRID, NONE, MULTI = 0, 1, 2, 3, 4, 255, 0x80


def state_widths(o, T, p, q):
    """Per isotope (database order, as the engine numbers them): Doppler half-width per unit wavenumber and
    Lorentz half-width, by the oracle's formulas (LblOracle.layer_dv / _strengths)."""
    ih2 = o.species.index("H2") if "H2" in o.species else -1
    ihe = o.species.index("He") if "He" in o.species else -1
    dop, lor = [], []
    for db in o.dbs:
        sp = o.species.index(db["molecule"])
        for info in db["isotopes"]:
            mi = info["mass"] * AMU
            dop.append(np.sqrt(2.0 * np.log(2.0) * KB * T / mi) / LS)
            s = sum(q[c] * (0.5 * (o.diam[sp] + o.diam[c])) ** 2 * np.sqrt(1.0 / mi + 1.0 / (o.mass[c] * AMU))
                    for c in (ih2, ihe) if c >= 0)
            lor.append(np.sqrt(2.0) / (LS * np.sqrt(np.pi * KB * T)) * p * s)
    return np.array(dop), np.array(lor)


def _rel(value, threshold):
    return abs(value / threshold - 1.0)


def predict(o, prof, wn=None, mid_reach=0, voigt_grid=None):
    """Owner map and threshold margins of one profile.

    o: LblOracle of the cfg (of the block, if the engine is sharded: wn_slice); prof [(S+1), L]; wn: the
    engine's local grid (default o.wn).  Returns (owners uint8 [L, ntile], margin [L, ntile]): margin is the
    smallest relative distance of a compared quantity from its threshold among the decisions taken for that
    (state, tile) -- narrow_state's cany against pair_reach * dnu, mid_state's against mid_reach * wndelt,
    and half the narrowest half-width against every divisor's spacing."""
    wn = o.wn if wn is None else np.asarray(wn)
    grid = (o.voigt == "grid") if voigt_grid is None else voigt_grid
    prof = np.asarray(prof, float).reshape(len(o.species) + 1, -1)
    L, W = prof.shape[1], len(wn)
    ntile = (W + TILE - 1) // TILE
    owners = np.zeros((L, ntile), np.uint8)
    margin = np.full((L, ntile), np.inf)
    for l in range(L):
        T, p, q = prof[0, l], o.press[l], prof[1:, l]
        dop, lor = state_widths(o, T, p, q)
        dv = o.layer_dv(T, p, q)
        m_state = np.inf
        if o.osamp > 1 and o.osamp_rule != "full":
            wmin = np.min(np.maximum(o.wn_first * dop, lor))
            for k in range(1, o.osamp + 1):
                if o.osamp % k == 0:
                    m_state = min(m_state, _rel(0.5 * wmin, o.wndelt / k))
        mid = False
        if mid_reach > 0 and dv == 1:
            cany = np.max(o.nwidth * np.maximum(lor, (o.wn_last + 1.0) * dop * DOPPLER_SLACK))
            mid = cany <= mid_reach * o.wndelt
            m_state = min(m_state, _rel(cany, mid_reach * o.wndelt))
        for t in range(ntile):
            tile0 = t * TILE
            ilast = min(tile0 + TILE - 1, W - 1)
            narrow, m = False, m_state
            if ilast > tile0:
                dnu = min(wn[tile0 + 1] - wn[tile0], wn[ilast] - wn[ilast - 1])
                cany = np.max(o.nwidth * np.maximum(lor, (wn[ilast] + 1.0) * dop * DOPPLER_SLACK))
                narrow = cany <= PAIR_REACH * dnu
                if dv == 1 and not grid:
                    m = min(m, _rel(cany, PAIR_REACH * dnu))
            owners[l, t] = GRID if grid else FINE_OVER if dv > 1 else PAIRS if narrow else FINE_MID if mid else TILE_K
            margin[l, t] = m
    return owners, margin


def point_owners(owners, W):
    """owners [L, ntile] -> [L, W]: the owner of every output point."""
    return np.repeat(owners, TILE, axis=1)[:, :W]


def kept_lines(o, T, p, q):
    """Per database, the oracle's kept lines of a state: (centres, cuts), list order."""
    out = []
    for db in o.dbs:
        S, aD, aL = o._strengths(db, T, p, q, False)
        keep = (S >= o.ethresh * S.max()) & (S > 0)
        out.append((db["wn"][keep], (o.nwidth * np.maximum(aD, aL))[keep]))
    return out


def pair_rounds(o, prof, layer, wn=None):
    """The pair kernel's queue for one state, from the oracle's line ranges: per 64-point wave, the lines that
    join the queue (list order, database after database) with the number of points each takes (one of slack
    either side, as the kernel counts them), and the rounds the queue is cut into (a round looks at the 64
    leading lines -- all that are left when the list is exhausted -- and takes those whose pairs fit
    kPairCap).  Returns a list of dicts per wave: n (points per queued line), reach (in-cut points per queued
    line over the WHOLE grid, plus the two of slack), rounds [(lines looked at, lines taken, pairs)]."""
    wn = o.wn if wn is None else np.asarray(wn)
    prof = np.asarray(prof, float).reshape(len(o.species) + 1, -1)
    lines = kept_lines(o, prof[0, layer], o.press[layer], prof[1:, layer])
    W = len(wn)
    waves = []
    for w0 in range(0, W, 64):
        pts = np.full(64, 1e300)
        pts[:min(64, W - w0)] = wn[w0:w0 + 64]
        nu_a, nu_b = wn[w0], wn[min(w0 + 63, W - 1)]
        ns, reach = [], []
        for nu0, cut in lines:
            for c0, ct in zip(nu0, cut):
                if not (c0 + ct >= nu_a and c0 - ct <= nu_b):
                    continue
                b = int(np.searchsorted(pts, c0 - ct, "left"))
                c = int(np.searchsorted(pts, c0 + ct, "right"))
                n = 0
                if c > b:
                    first = b - 1 if b > 0 else 0
                    n = min((c + 1 if c < 64 else 64) - first, NMAX)
                ns.append(n)
                reach.append(int(np.sum(np.abs(wn - c0) <= ct)) + 2)
        ns = np.array(ns, int)
        rounds, h = [], 0
        while h < len(ns):
            nq = min(len(ns) - h, 64)
            fit = np.cumsum(ns[h:h + nq]) <= PAIR_CAP
            m = nq if fit.all() else int(np.argmin(fit))
            assert m >= 1
            rounds.append((nq, m, int(ns[h:h + m].sum())))
            h += m
        waves.append(dict(n=ns, reach=np.array(reach, int), rounds=rounds))
    return waves
