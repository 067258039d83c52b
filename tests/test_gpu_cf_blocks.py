"""GPU, one device, no RCCL: contribution functions and band transmittance on wavenumber blocks (include/bartrt.h,
bartrt_cf_setup_block / _partials_dev / _combine_dev).  One process stands in for any rank count: for r = 0 .. n - 1
an engine on block r of n is initialised, its part of the band sums taken and the engine freed; the parts, stacked as
an all-gather would leave them, go through cf_combine_dev on an unsharded engine and are held to that engine's own
contribution_dev / transmittance_dev.

The grid of tests/test_gpu_step_blocks.py: 1777 samples (888 + 889; no block start for n = 2, 3, 5 is a multiple of
64), 60 layers, and its five windows per rank count: inside one block, across three or more blocks, two samples on
either side of a block edge, the grid's first 25 and last 30 samples.  Five walkers: walker 2 has a non-finite
temperature (ok = 0), walker 3 its own cloud top through `over`.

n = 1: the same bits (one slot: 0 + the tile-order sum, then the same division).  n > 1: the two results differ only
in how a sum of at most N window samples is associated; relative to the row's largest |value| that is bounded by
2 N 2^-53 times sum|terms| / max, about 5e-13 for N <= 2424, and 1e-11 is asserted: above the bound, two orders under
the 1e-9 at which the same rows are held to the oracle.  The per-wavenumber output of the blocks, concatenated, is the
unsharded output bit for bit: a lane's arithmetic does not depend on its block."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_cf import TOL, _rel, inf_cfg, oracle_band, walkers  # noqa: E402
from test_gpu_step_blocks import _filters, _starts  # noqa: E402

pytestmark = pytest.mark.gpu

NWAVE, NLAYERS = 1777, 60
BLOCK_TOL = 1e-11
ENOTSUP = -4
# name -> (extra cfg keys, integration rule or None for the cfg's, kinds)
CONFIGS = {
    "eclipse-integ0": (None, 0, ("cf", "tr")),
    "eclipse-integ1": (None, 1, ("cf", "tr")),
    "transit": ({"solution": "transit", "starrad": 1.145}, None, ("tr",)),
}
BAD, CLOUDY = 2, 3


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from bart_amd import synth
    made = {}

    def get(extra):
        key = "transit" if extra else "eclipse"
        if key not in made:
            d = str(tmp_path_factory.mktemp("cfblk_" + key))
            made[key] = synth.make_case(d, nlayers=NLAYERS, nwave=NWAVE, wnlow=1200.0, opmol=("CH4",), seed=11,
                                        extra_keys=extra)
        return made[key]
    return get


def batch(case):
    """-> (profiles with walker BAD's temperature broken, the clean profiles, over [5, 3])."""
    clean = walkers(case, 5, seed=29)
    bad = clean.copy()
    bad[BAD, 7] = np.nan
    over = np.full((5, 3), np.nan)
    over[CLOUDY, 1] = -1.5          # log10 bar: a deck inside the atmosphere
    return bad, clean, over


def windows(n):
    idx0, npts, resp, _ = _filters(NWAVE, n, np.random.default_rng(100 + n))
    off = np.concatenate([[0], np.cumsum(npts)])
    trapz = np.array([np.sum(0.5 * (resp[a:b][:-1] + resp[a:b][1:])) for a, b in zip(off[:-1], off[1:])])
    return idx0, npts, resp, trapz


def _call(engine, kind):
    return engine.CF_CONTRIB if kind == "cf" else engine.CF_TRANSMIT


def unsharded(case, integ, kinds, win, profs, over):
    """-> {kind: (band, full, ok)} of the unsharded engine's device calls."""
    import torch
    from bart_amd import engine, transit_module as trm
    out = {}
    engine.init(case.tcfg)
    try:
        if integ is not None:
            trm.set_integ(integ)
        engine.cf_setup(win)
        d, dov = torch.from_numpy(profs).cuda(), torch.from_numpy(over).cuda()
        for kind in kinds:
            ok = torch.zeros(len(profs), dtype=torch.uint8, device="cuda")
            fn = engine.contribution_dev if kind == "cf" else engine.transmittance_dev
            band, full = fn(d, full=True, d_ok=ok, over=dov)
            torch.cuda.synchronize()
            out[kind] = (band.clone(), full.clone(), ok.clone())
    finally:
        trm.free_memory()
    return out


def block_parts(case, integ, kinds, win, n, batches, over):
    """Rank by rank: -> {kind: [per batch: (parts [n][nw][nf][L], fulls [n] of [nw][W_r][L], oks [n])]}."""
    import torch
    from bart_amd import engine, transit_module as trm
    s = _starts(NWAVE, n)
    out = {kind: [([], [], []) for _ in batches] for kind in kinds}
    for r in range(n):
        engine.init(case.tcfg, shard=(r, n))
        try:
            assert engine.local_range() == (s[r], s[r + 1])
            if integ is not None:
                trm.set_integ(integ)
            if n > 1:      # bartrt_cf_setup keeps refusing a sharded engine that has no communicator
                idx0, npts, resp, _ = win
                assert trm.lib().bartrt_cf_setup(len(idx0), trm._ptr(idx0), trm._ptr(npts), trm._ptr(resp)) == ENOTSUP
            engine.cf_setup_block(win)
            dov = torch.from_numpy(over).cuda()
            for kind in kinds:
                for b, profs in enumerate(batches):
                    ok = torch.zeros(len(profs), dtype=torch.uint8, device="cuda")
                    part, full = engine.cf_partials_dev(torch.from_numpy(profs).cuda(), _call(engine, kind), full=True,
                                                        d_ok=ok, over=dov)
                    torch.cuda.synchronize()
                    assert full.shape == (len(profs), s[r + 1] - s[r], NLAYERS)
                    for lst, t in zip(out[kind][b], (part, full, ok)):
                        lst.append(t.clone())
        finally:
            trm.free_memory()
    return out


def combine(case, win, n, jobs):
    """jobs: (the ranks' parts, ok flags or None) each -> their band rows, on one unsharded engine."""
    import torch
    from bart_amd import engine, transit_module as trm
    engine.init(case.tcfg)
    try:
        engine.cf_setup_block(win)
        out = [engine.cf_combine_dev(torch.stack(slots).contiguous(), n, d_ok=ok) for slots, ok in jobs]
        torch.cuda.synchronize()
        return out
    finally:
        trm.free_memory()


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_block_parts_combine_to_the_unsharded_rows(cases, config, n):
    import torch
    extra, integ, kinds = CONFIGS[config]
    case = cases(extra)
    bad, clean, over = batch(case)
    win = windows(n)
    s = _starts(NWAVE, n)
    ref = unsharded(case, integ, kinds, win, bad, over)
    got = block_parts(case, integ, kinds, win, n, (bad, clean), over)
    good = [w for w in range(5) if w != BAD]
    if n >= 3:      # the "inside" window lies in one block: the other ranks hold no entry of it
        empty = [r for r in range(n) if s[r + 1] <= win[0][0] or s[r] >= win[0][0] + win[1][0]]
        assert len(empty) == n - 1
    for kind in kinds:
        rband, rfull, rok = ref[kind]
        parts, fulls, oks = got[kind][0]
        assert rok.tolist() == [1, 1, 0, 1, 1] and all(torch.equal(o, rok) for o in oks)
        cparts, _, coks = got[kind][1]
        band, cband = combine(case, win, n, [(parts, rok), (cparts, None)])
        assert torch.isnan(band[BAD]).all() and torch.isnan(rband[BAD]).all()
        assert torch.isfinite(band[good]).all()
        if n >= 3:
            for r in empty:
                assert (parts[r][:, 0] == 0.0).all()
        # the blocks' per-wavenumber values are the unsharded engine's, bit for bit
        assert torch.equal(torch.cat(fulls, dim=1)[good], rfull[good])
        diff = _rel(band[good].cpu().numpy(), rband[good].cpu().numpy())
        print("cf blocks %s %s n=%d: largest difference from the unsharded rows %.3e" % (config, kind, n, diff))
        if n == 1:
            assert torch.equal(band[good], rband[good])
        else:
            assert diff < BLOCK_TOL
        # the flagged walker leaves the others' rows as they are without it
        assert all(o.tolist() == [1] * 5 for o in coks)
        assert torch.equal(cband[good], band[good]) and torch.isfinite(cband).all()
        # walker CLOUDY's deck is its own: below it the depth repeats and its contribution is 0
        if kind == "cf":
            deep = case.press_bar >= 10 ** -1.5
            below = np.zeros_like(deep)
            below[:-1] = deep[:-1] & deep[1:]
            assert below.sum() > 5 and np.all(band[CLOUDY].cpu().numpy()[:, below] == 0.0)


def test_three_blocks_against_the_oracle(cases):
    """The n = 3 combined rows against tests/cf_restate.py on the oracle's `toomuch 1e100` optical depth, at the
    tolerance the unsharded rows are held to."""
    from oracle import rt_oracle as orc
    case = cases(None)
    _, clean, over = batch(case)
    win = windows(3)
    got = block_parts(case, None, ("cf", "tr"), win, 3, (clean,), over)
    cfg = inf_cfg(case, case.dir)
    for kind in ("cf", "tr"):
        parts, _, _ = got[kind][0]
        band = combine(case, win, 3, [(parts, None)])[0].cpu().numpy()
        for w in (0, 1, CLOUDY):
            o = orc.OracleEngine(cfg)
            if w == CLOUDY:
                o.set_cloudtop(-1.5)
            ref, _ = oracle_band(o, case, clean[w], win, kind)
            err = _rel(band[w], ref)
            print("cf blocks n=3 %s walker %d: against the oracle %.3e" % (kind, w, err))
            assert err < TOL


def test_partials_cut_into_chunks_are_the_one_chunk_bits(cases, monkeypatch):
    """cf_partials_dev is the one call shape no other test cuts into chunks: three walkers (walker 1 under its own
    cloud top, the others' override rows NaN) with `full` and d_ok, once under the default workspace cap (one chunk)
    and once under BARTRT_CF_WORKSPACE_BYTES=1 (one walker per chunk).  The sums, the per-wavenumber values and the
    flags are the same bytes, and cf_combine_dev over that one slot is contribution_dev on the same inputs."""
    import torch
    from bart_amd import engine, transit_module as trm
    case = cases(None)
    profs = batch(case)[1][:3]
    over = np.full((3, 3), np.nan)
    over[1, 1] = -1.5
    engine.init(case.tcfg)
    try:
        engine.cf_setup(windows(1))
        d, dov = torch.from_numpy(profs).cuda(), torch.from_numpy(over).cuda()

        def partials():
            ok = torch.zeros(3, dtype=torch.uint8, device="cuda")
            part, full = engine.cf_partials_dev(d, engine.CF_CONTRIB, full=True, d_ok=ok, over=dov)
            torch.cuda.synchronize()
            return [t.cpu().numpy() for t in (part, full, ok)], part

        monkeypatch.delenv("BARTRT_CF_WORKSPACE_BYTES", raising=False)
        one, _ = partials()
        monkeypatch.setenv("BARTRT_CF_WORKSPACE_BYTES", "1")
        cut, d_part = partials()
        monkeypatch.delenv("BARTRT_CF_WORKSPACE_BYTES")
        assert one[2].tolist() == [1, 1, 1] and np.isfinite(one[0]).all()
        for a, b in zip(one, cut):
            assert np.array_equal(a, b)
        ok = torch.zeros(3, dtype=torch.uint8, device="cuda")
        band = engine.cf_combine_dev(d_part, 1, d_ok=torch.from_numpy(cut[2]).cuda())
        rband, rfull = engine.contribution_dev(d, full=True, d_ok=ok, over=dov)
        torch.cuda.synchronize()
        assert np.array_equal(band.cpu().numpy(), rband.cpu().numpy())
        assert np.array_equal(cut[1], rfull.cpu().numpy()) and ok.cpu().numpy().tolist() == [1, 1, 1]
    finally:
        trm.free_memory()
