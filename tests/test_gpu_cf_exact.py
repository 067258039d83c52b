"""The contribution-function kernels (csrc/contrib.hip: cf_eclipse, cf_transit staged and unstaged, cf_flush's reduction,
cf_block_sums, cf_combine) against the exact restatement of tests/cf_exact.py -- mpmath at 50 digits, fed the doubles
the kernels themselves read through engine.cf_records (the walker's layer records, rdlp, the radii, the filter tables)
-- within that module's DERIVED bound, on the cases of tests/cf_cases.py, which tests/test_cf_exact_cpu.py holds to the
conditions that make these tests able to fail.  tests/test_gpu_cf.py keeps the oracle on all columns at 1e-9 of the
row's maximum; that comparison is repeated here on every case.

Per case, walker 1 of three, every rule, kind and deck of the case: the full output on the checked columns within the
bound; the band rows within the whole bound; the reduction ON ITS OWN -- the band rows recomputed from the device's own
full output with math.fsum and the read-back weights -- within the reduction's part of the bound; the read-back
weights the exact products h_i resp_i and trapz within its summation bound; row 0 of the contribution exactly 0, of a
transit engine's transmittance exactly 1; below a deck the contribution exactly 0 and the transmittance repeated to
the bit; the same bits alone, first and last of three and from device buffers.  No tolerance here is fitted to a run:
the worst |got - exact| / bound is printed per test (pytest -s; MEASUREMENTS.md has the figures)."""
import ctypes as C

import numpy as np
import pytest

import cf_cases as cc
import cf_exact as cx
import transit_restate as tr
from test_gpu_cf import TOL, _rel, oracle_band

pytestmark = pytest.mark.gpu
EINVAL = -1
SIMPSON_PAD = 8          # kSimpsonPad (csrc/integ.hpp)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("cf_exact"))


@pytest.fixture(scope="module")
def cases(root):
    made = {}

    def get(group):
        if group not in made:
            made[group] = cc.GROUPS[group](root)
        return made[group]
    return get


def _call(kind, profs, win):
    from bart_amd import engine
    if kind == cc.CF:
        return engine.contribution(profs, win, normalize=False, full=True)
    return engine.transmittance(profs, win, full=True)


def _tables(c, rec, W, lo=0):
    """The read-back filter tables against cf_setup's definition: the tile tables' structure, every weight the exact
    product (a half of a double is exact: equality), trapz within its summation bound.  W, lo: the samples and the
    first sample of the engine's block -- a window is clipped to it, its halves stay at its true ends, trapz is the
    whole window's, a filter without a sample in the block has no entry.  -> per filter the entries [(first sample ON
    THE FULL GRID, weights)] in tile order."""
    wins = cc.window_list(c.windows)
    ntiles = (W + 63) // 64
    assert rec["ntiles"] == ntiles and rec["nfilters"] == len(wins) and len(rec["tile_ptr"]) == ntiles + 1
    ent_tile = np.repeat(np.arange(ntiles), np.diff(rec["tile_ptr"]))
    rows = []
    for f, (idx0, npts, resp) in enumerate(wins):
        w, t, dt = cx.exact_weights(idx0, npts, resp)
        assert float(cx.absdev(rec["trapz"][f], t)) <= dt, (c.tag, f)
        ents = rec["f_ent"][rec["f_ptr"][f]:rec["f_ptr"][f + 1]]
        tiles = [int(ent_tile[e]) for e in ents]
        inside = [s for s in range(npts) if lo <= idx0 + s < lo + W]
        assert tiles == sorted(set((idx0 + s - lo) // 64 for s in inside)), (c.tag, f, tiles)
        want = np.zeros(ntiles * 64)
        for s in inside:
            want[idx0 + s - lo] = float(w[s])
        row = []
        for e, t_ in zip(ents, tiles):
            assert np.array_equal(rec["wt"][e], want[64 * t_:64 * t_ + 64]), (c.tag, f, t_)
            row.append((lo + 64 * t_, rec["wt"][e][:min(64, W - 64 * t_)]))
        rows.append(row)
    return rows


def _hold_case(c, worst):
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    o_tab = orc.OracleEngine(c.tcfg)
    engine.init(c.tcfg)
    try:
        wn = trm.get_waveno_arr(trm.get_no_samples())
        W, L = len(wn), len(c.press_bar)
        wins = cc.window_list(c.windows)
        bits_done = False
        for deck in c.decks:
            if deck is not None:
                trm.set_cloudtop(deck)
            exact = {}
            for rule in c.rules:
                trm.set_integ(rule)
                o = orc.OracleEngine(cc.inf_cfg(c), integ=rule)
                if deck is not None:
                    o.set_cloudtop(deck)
                for kind in c.kinds:
                    what = (c.tag, deck, rule, kind)
                    band, full = _call(kind, c.profs, c.windows)
                    rec = engine.cf_records(1)
                    assert rec["ok"] == 1 and rec["nwalkers"] == 3, what
                    if hasattr(c, "form"):
                        assert rec["kernel"] == c.form and rec["lds_bytes"] == cc.transit_lds(L, rec["nmol"], rec["ncs"], "<staged>" in c.form), (what, rec["kernel"], rec["lds_bytes"])
                        print("%s: L = %d, %s, %d bytes of LDS (%s 64 kB)" % (c.tag, L, rec["kernel"], rec["lds_bytes"], "above" if rec["lds_bytes"] > 65536 else "within"))
                    if c.group == "deep_eclipse":
                        # the launch above 64 kB, from the engine's own M and C (csrc/contrib.hip, "Dynamic LDS")
                        nrec = 4 + 2 * rec["nmol"] + 2 * rec["ncs"] + 1 + rec["ncs"]
                        want = 8 * L * nrec + 8 * cc.ROWS * cc.PITCH + (24 * (L + SIMPSON_PAD) if rule == 1 else 0)
                        assert rec["kernel"] == "cf_eclipse" and rec["lds_bytes"] == want and 65536 < want <= 163840, (what, rec["kernel"], rec["lds_bytes"], want)
                        print("%s rule %d: %s, %d bytes of LDS" % (c.tag, rule, rec["kernel"], rec["lds_bytes"]))
                    rows = _tables(c, rec, W)
                    key = rule == 1
                    if key not in exact:
                        col = cx.from_records(o_tab, rec, c.cols, wn)
                        exact[key] = (col,) + cx.depths(col, rule, transit=col.ch is not None)
                    col, tau, dtau = exact[key]
                    v, dv = cx.values(col, tau, dtau, kind)
                    b, db, dred = cx.band(col, v, dv, wins)
                    pos = [col.cols.index(i) for i in c.checked]
                    # the condition tests/test_cf_exact_cpu.py holds with the oracle's extinction taken exactly, here
                    # with the records' own error term de: the bound at most 1e-11 of every checked row's maximum
                    if c.tag not in cc.ABSOLUTE:
                        share = max(cx.ratio(dv[:, pos].max(axis=0), np.abs(tr.to_float(v[:, pos])).max(axis=0)),
                                    cx.ratio(db.max(axis=1), np.abs(tr.to_float(b)).max(axis=1)))
                        worst["share"] = max(worst["share"], share)
                        assert share <= 1e-11, (what, "bound / row max", share)
                    # the full output against the exact value (atm order: the bottom layer first)
                    got = full[1][c.checked].T                       # [L, checked], atm order
                    dev, bnd = cx.absdev(got, cx.atm(v)[:, pos]), cx.atm(dv)[:, pos]
                    r = cx.ratio(dev, bnd)
                    assert r <= 1.0, (what, "full", r)
                    # (printed apart: the rows past tau = 708, where the clamp's exp(-708) = 3.31e-308 stands against
                    # its allowance of 3.4e-308, 0.973 of it on every thick column)
                    big = bnd > 1e-300
                    worst["full"] = max(worst["full"], cx.ratio(dev[big], bnd[big]))
                    worst["clamp"] = max(worst["clamp"], cx.ratio(dev[~big], bnd[~big]))
                    # the band row against the exact band value, the whole bound
                    dev, bnd = cx.absdev(band[1], b[:, ::-1]), db[:, ::-1]
                    r = cx.ratio(dev, bnd)
                    assert r <= 1.0, (what, "band", r)
                    big = bnd > 1e-300
                    worst["band"] = max(worst["band"], cx.ratio(dev[big], bnd[big]))
                    worst["clamp"] = max(worst["clamp"], cx.ratio(dev[~big], bnd[~big]))
                    # the reduction on its own: the device's own full output, exactly summed
                    own, dro = cx.reduction_of(full[1].T[::-1], rows, rec["trapz"], 1)
                    r = cx.ratio(np.abs(band[1] - own[:, ::-1]), dro[:, ::-1])
                    worst["reduction"] = max(worst["reduction"], r)
                    assert r <= 1.0, (what, "reduction", r)
                    # the oracle on all columns, as tests/test_gpu_cf.py keeps it.  Not the contribution of the thin and
                    # all-zero columns: there every layer's value is a difference of transmittances that agree to ten
                    # digits and more, the oracle path (numpy's exp) and the kernel (exp_rt, 7.5e-14 of exp) each round
                    # it their own way, and "1e-9 of the row's maximum" compares the two roundings (measured on the
                    # thin case: 3.4e-4 of the row's maximum between them, the device 7e-4 of the ABSOLUTE bound from
                    # the exact value).  Those rows are held by the exact value above; their transmittance is held here.
                    for w in (0, 1, 2) if not (c.tag in cc.ABSOLUTE and kind == cc.CF) else ():
                        rb, rf = oracle_band(o, c, c.profs[w], c.windows, "cf" if kind == cc.CF else "tr")
                        assert _rel(band[w], rb) < TOL and _rel(full[w], rf) < TOL, (what, w)
                    # the exact rows
                    kend = col.kend
                    if kind == cc.CF:
                        assert np.all(full[:, :, L - 1] == 0.0) and np.all(band[:, :, L - 1] == 0.0), what
                        assert np.all(full[1][:, :L - 1 - kend] == 0.0) and np.all(band[1][:, :L - 1 - kend] == 0.0), what
                    else:
                        if col.ch is not None:
                            assert np.all(full[:, :, L - 1] == 1.0), what
                        assert np.all(full[1][:, :L - 1 - kend] == full[1][:, L - 1 - kend:L - kend]), what
                        assert np.all(band[1][:, :L - 1 - kend] == band[1][:, L - 1 - kend:L - kend]), what
                    if bits_done:
                        continue
                    bits_done = True
                    # the same bits alone, first and last of three, and from device buffers
                    for order, at in (([1], 0), ([1, 0, 2], 0), ([0, 2, 1], 2)):
                        b2, f2 = _call(kind, c.profs[order], c.windows)
                        assert np.array_equal(b2[at], band[1]) and np.array_equal(f2[at], full[1]), (what, order)
                    import torch
                    engine.cf_setup(c.windows)
                    d = torch.tensor(c.profs, dtype=torch.float64, device="cuda")
                    bd = engine.contribution_dev(d) if kind == cc.CF else engine.transmittance_dev(d)
                    torch.cuda.synchronize()
                    assert np.array_equal(bd.cpu().numpy(), band), what
    finally:
        trm.free_memory()


def _run_group(cases, group, tags=None):
    worst = {"full": 0.0, "band": 0.0, "reduction": 0.0, "clamp": 0.0, "share": 0.0}
    for c in cases(group):
        if tags is None or c.tag in tags:
            _hold_case(c, worst)
    print("%s %s: worst |got - exact| / bound: full %.3f, band %.3f, reduction alone %.3f, clamped rows %.3f; largest "
          "bound / row max %.2e" % (group, tags or "", worst["full"], worst["band"], worst["reduction"], worst["clamp"], worst["share"]))


@pytest.mark.parametrize("L", cc.LAYERS)
def test_layer_counts(cases, L):
    """2 .. 48 layers under rules 0, 1 and 2, contribution and transmittance: below one reduction block (rows j >= nk of
    the LDS block never written), exactly one, one more, two and one more, three."""
    _run_group(cases, "layers", ("L%d" % L,))


def test_deck_rows(cases):
    """The deck on rows 15, 16 and 17 of 33 layers, on the top layer and below the bottom one."""
    _run_group(cases, "deck")


@pytest.mark.parametrize("tag", ["staged_last_64k", "staged_first_over_64k", "staged_last", "unstaged_first", "unstaged_last"])
def test_deep_transit_columns(cases, tag):
    """The transit kernel at the edges of its launch paths, from the engine's own M and C: the last depth within 64 kB
    of dynamic LDS and the first above it (the raised attribute), the last staged and the first unstaged depth, the
    last that fits.  Each asserts the kernel form and the LDS bytes the read-back reports."""
    from bart_amd import engine, transit_module as trm
    c = [c for c in cases("deep_transit") if c.tag == tag][0]
    engine.init(c.tcfg)
    try:
        m, n = C.c_int(), C.c_int()
        trm.check(trm.lib().bartrt_get_prep_shape(C.byref(m), C.byref(n)))
        assert cc.transit_edges(m.value, n.value)[tag][0] == len(c.press_bar), (m.value, n.value)
    finally:
        trm.free_memory()
    _run_group(cases, "deep_transit", (tag,))


def test_deep_transit_refusal(cases):
    """One layer more than fits: BARTRT_EINVAL, the message names LDS, no chunk is left to read back."""
    from bart_amd import engine, transit_module as trm
    c = [c for c in cases("deep_transit") if c.tag == "refused"][0]
    engine.init(c.tcfg)
    try:
        m, n = C.c_int(), C.c_int()
        trm.check(trm.lib().bartrt_get_prep_shape(C.byref(m), C.byref(n)))
        L = len(c.press_bar)
        assert cc.transit_edges(m.value, n.value)["refused"][0] == L
        engine.cf_setup(c.windows)
        p = np.ascontiguousarray(c.profs)
        out = np.zeros((3, len(c.windows[0]), L))
        rc = trm.lib().bartrt_cf_batch(trm._ptr(p), 3, p.shape[1], cc.TR, trm._ptr(out), None, None)
        msg = trm.lib().bartrt_last_error()
        assert rc == EINVAL and b"LDS" in msg, (rc, msg)
        seen = engine.cf_launch()
        print("refused: L = %d, %s, %d bytes of LDS asked for: %s" % (L, seen["kernel"], seen["lds_bytes"], msg.decode()))
        assert seen["nwalkers"] == 0 and seen["kernel"] == "cf_transit<unstaged>" and seen["lds_bytes"] > 160 * 1024
        with pytest.raises(trm.TransitError, match="no contribution-function call"):
            engine.cf_records(0)
    finally:
        trm.free_memory()


def test_deep_eclipse_columns(cases):
    """Nine molecules, three CIA pairs, 300 layers: the eclipse kernels above 64 kB of dynamic LDS under every rule."""
    _run_group(cases, "deep_eclipse")


@pytest.mark.parametrize("tag", ["W577", "W63", "W64", "W65"])
def test_grids(cases, tag):
    """Ten tiles (a launch padded to sixteen; tiles without an entry) and the whole-grid window on 63, 64, 65 samples."""
    _run_group(cases, "grid", (tag,))


@pytest.mark.parametrize("tag", ["zero_top", "zero_mid", "zero_all", "thin", "thick"])
def test_optical_extremes(cases, tag):
    """Zero extinction in the top band, a middle band and everywhere; every depth below 1e-10; depths past 708."""
    _run_group(cases, "zero" if tag.startswith("zero") else "extreme", (tag,))


@pytest.mark.parametrize("W", cc.BLOCK_GRIDS)
def test_blocks(cases, W):
    """Two ranks one after the other on the one device (cf_setup_block, cf_partials_dev, cf_combine_dev), the cut at
    63, 64 and 65 with [63, 65) and [62, 66) across it: each rank's tables are the clipped windows (the halves at the
    windows' true ends, the whole window's trapz); the ranks' full outputs side by side are the unsharded engine's
    bits; the combined band rows lie within the bound of the exact band value, the reduction's part counting both
    ranks' tiles and two slots; and against the unsharded row, in the relation the header of csrc/contrib.hip states:
    the rounding of a differently associated sum -- both rows within their reduction bounds of the exactly summed
    row -- and, at the cut of 64, where the ranks' tiles ARE the unsharded tiles and every window here has at most one
    tile per rank, the same bits."""
    import torch
    from bart_amd import engine, transit_module as trm
    from oracle import rt_oracle as orc
    c = [c for c in cases("blocks") if c.tag == "B%d" % W][0]
    wins, L, cut = cc.window_list(c.windows), len(c.press_bar), W // 2
    los, rule = [0, cut], c.rules[0]
    uns, recs = {}, {}
    engine.init(c.tcfg)
    try:
        wn = trm.get_waveno_arr(trm.get_no_samples())
        trm.set_integ(rule)
        for kind in c.kinds:
            uns[kind] = _call(kind, c.profs, c.windows)
        rec_u = engine.cf_records(1)
        rows_u = _tables(c, rec_u, W)
    finally:
        trm.free_memory()
    parts, fulls, rows = {k: [] for k in c.kinds}, {k: [] for k in c.kinds}, [[] for _ in wins]
    for r in (0, 1):
        engine.init(c.tcfg, shard=(r, 2))
        try:
            lo, hi = engine.local_range()
            assert (lo, hi) == (los[r], W if r else cut)
            trm.set_integ(rule)
            engine.cf_setup_block(c.windows)
            d = torch.tensor(c.profs, dtype=torch.float64, device="cuda")
            for kind in c.kinds:
                part, full = engine.cf_partials_dev(d, kind, full=True)
                torch.cuda.synchronize()
                parts[kind].append(part.clone()); fulls[kind].append(full.cpu().numpy())
            rec = engine.cf_records(1)
            assert np.array_equal(rec["coef"], rec_u["coef"]) and rec["kstop"] == rec_u["kstop"] and np.array_equal(rec["rdlp"], rec_u["rdlp"])
            for f, row in enumerate(_tables(c, rec, hi - lo, lo)):
                rows[f] += row
        finally:
            trm.free_memory()
    engine.init(c.tcfg)
    try:
        engine.cf_setup_block(c.windows)
        bands = {kind: engine.cf_combine_dev(torch.stack(parts[kind]).contiguous(), 2).cpu().numpy() for kind in c.kinds}
    finally:
        trm.free_memory()
    col = cx.from_records(orc.OracleEngine(c.tcfg), rec_u, c.cols, wn)
    tau, dtau = cx.depths(col, rule)
    worst = {"band": 0.0, "reduction": 0.0}
    for kind in c.kinds:
        band_u, full_u = uns[kind]
        assert np.array_equal(np.concatenate(fulls[kind], axis=1), full_u), (W, kind)
        v, dv = cx.values(col, tau, dtau, kind)
        b, db, _ = cx.band(col, v, dv, wins, lo=los, nranks=2)
        dev, bnd = cx.absdev(bands[kind][1], b[:, ::-1]), db[:, ::-1]
        assert cx.ratio(dev, bnd) <= 1.0, (W, kind, "band", cx.ratio(dev, bnd))
        worst["band"] = max(worst["band"], cx.ratio(dev[bnd > 1e-300], bnd[bnd > 1e-300]))      # (the clamp rows apart, as above)
        own, dro = cx.reduction_of(full_u[1].T[::-1], rows, rec_u["trapz"], 2)
        r = cx.ratio(np.abs(bands[kind][1] - own[:, ::-1]), dro[:, ::-1])
        worst["reduction"] = max(worst["reduction"], r)
        assert r <= 1.0, (W, kind, "reduction", r)
        own_u, dro_u = cx.reduction_of(full_u[1].T[::-1], rows_u, rec_u["trapz"], 1)
        assert cx.ratio(np.abs(band_u[1] - own_u[:, ::-1]), dro_u[:, ::-1]) <= 1.0, (W, kind)
        assert np.all(np.abs(bands[kind][1] - band_u[1]) <= (dro + dro_u)[:, ::-1]), (W, kind)
        if cut == 64:
            assert np.array_equal(bands[kind], band_u), (W, kind)
    print("blocks, %d samples cut at %d: worst |got - exact| / bound: band %.3f, reduction alone %.3f"
          % (W, cut, worst["band"], worst["reduction"]))


def test_read_back_refusals(cases):
    """bartrt_cf_get_records without a setup, without a call since the setup, for a walker outside the chunk, and for
    the transit arrays on an eclipse engine."""
    from bart_amd import engine, transit_module as trm
    c = cases("layers")[0]
    engine.init(c.tcfg)
    try:
        with pytest.raises(trm.TransitError, match="cf_setup first"):
            engine.cf_launch()
        engine.cf_setup(c.windows)
        assert engine.cf_launch()["nwalkers"] == 0
        with pytest.raises(trm.TransitError, match="no contribution-function call"):
            engine.cf_records(0)
        engine.transmittance(c.profs, c.windows)
        assert engine.cf_records(2)["nwalkers"] == 3 and "rtop" not in engine.cf_records(0)
        for w in (-1, 3):
            with pytest.raises(trm.TransitError, match="outside the latest chunk"):
                engine.cf_records(w)
        r = engine._CfRecords()
        ds = np.zeros((len(c.press_bar),) * 2)
        r.ds = ds.ctypes.data
        assert trm.lib().bartrt_cf_get_records(0, C.byref(r)) == EINVAL and b"transit" in trm.lib().bartrt_last_error()
    finally:
        trm.free_memory()
