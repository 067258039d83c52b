"""GPU: posterior marginals (include/bartrt.h, bartrt_marginals / _dev, bartrt_marginals_range / _dev, bartrt_hpd;
csrc/hist.hip), bart_amd.posterior.marginals and `retrieve --marginals`.  The reference is numpy throughout --
np.histogram, np.histogram2d, np.nanmin / np.nanmax -- and the criterion is equality of integers (of bits, for the
range): there is no tolerance anywhere in this file.  No test but the last initialises an engine: the calls need none."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hist_restate as hr  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1
SLAB = 256
ROWS = {"1": 1, "63": 63, "64": 64, "65": 65, "slab-1": SLAB - 1, "slab": SLAB, "slab+1": SLAB + 1, "2slab+7": 2 * SLAB + 7}
NINE_OF_TWELVE = [7, 2, 11, 0, 5, 9, 3, 10, 6]      # out of order, not adjacent
SELECTIONS = {"one": (3, [1]), "two": (5, [4, 1]), "nine of twelve": (12, NINE_OF_TWELVE)}


@pytest.fixture(scope="module")
def eng():
    from bart_amd import engine
    engine.marginals_set_slab(SLAB)
    assert engine.marginals_slab() == SLAB
    yield engine
    engine.marginals_set_slab(0)
    engine.marginals_set_chunk(0)


def _edges(nsel, nbins):
    """The three families of the CPU test, cycled over the selection."""
    return np.stack([hr.edges_of(hr.FAMILIES[s % 3], nbins) for s in range(nsel)])


def _forms(eng, x, cols, edges, pairs=True, ok=None):
    """Host and device form; both must be the same integers.  -> (h1, out, h2) as uint64."""
    import torch
    host = eng.marginals(x, cols, edges, pairs=pairs, ok=ok)
    d_ok = None if ok is None else torch.from_numpy(np.asarray(ok != 0, np.uint8)).cuda()
    dev = eng.marginals(torch.from_numpy(x).cuda(), cols, edges, pairs=pairs, ok=d_ok)
    for h, d in zip(host, dev):
        assert (h is None and d is None) or np.array_equal(h, d.cpu().numpy().astype(np.uint64))
    return host


def _assert_numpy(got, x, cols, edges, pairs=True, ok=None):
    want = hr.numpy_counts(x, cols, edges, ok, pairs)
    nrows = x.shape[0] if ok is None else int(np.count_nonzero(ok))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.all(got[0].sum(axis=1) + got[1].sum(axis=1) == nrows)
    if pairs:
        assert got[2].shape == want[2].shape and np.array_equal(got[2], want[2])
    else:
        assert got[2] is None


@pytest.mark.parametrize("sel", list(SELECTIONS))
@pytest.mark.parametrize("rows", list(ROWS))
def test_rows_and_selections_against_numpy(eng, rows, sel):
    """The partial wave, the slab seams, more than one workgroup; one column, two, and nine of twelve out of order."""
    nrows, (ld, cols) = ROWS[rows], SELECTIONS[sel]
    edges = _edges(len(cols), 20)
    x = hr.matrix_for(edges, nrows, ld, cols, seed=nrows + ld)
    got = _forms(eng, x, cols, edges)
    _assert_numpy(got, x, cols, edges)
    assert got[2].shape[0] == len(cols) * (len(cols) - 1) // 2
    lohi, nfin = eng.marginals_range(x, cols)
    want, wn = hr.numpy_range(x, cols)
    assert np.array_equal(lohi.view(np.uint64), want.view(np.uint64)) and np.array_equal(nfin, wn)


def test_sixty_four_columns(eng):
    """64 columns, 2 016 pairs at four bins: more pair histograms than one workgroup's LDS holds."""
    cols = [int(c) for c in np.random.default_rng(64).permutation(64)]
    edges = _edges(64, 4)
    x = hr.matrix_for(edges, 2 * SLAB + 7, 64, cols, seed=64)
    got = _forms(eng, x, cols, edges)
    assert got[2].shape == (2016, 4, 4)
    _assert_numpy(got, x, cols, edges)


@pytest.mark.parametrize("nbins", [1, 2, 20, 128])
def test_bins_with_pairs(eng, nbins):
    ld, cols = 7, [5, 0, 3]
    edges = _edges(3, nbins)
    x = hr.matrix_for(edges, 3 * (nbins + 1) + 7 + 2 * SLAB, ld, cols, seed=nbins)
    for s in range(3):                       # every special value is there
        assert all((x[:, cols[s]] == v).any() for v in hr.special_values(edges[s]) if not np.isnan(v))
    got = _forms(eng, x, cols, edges)
    _assert_numpy(got, x, cols, edges)
    assert np.all(got[1] >= 1)


def test_1024_bins_without_pairs(eng):
    ld, cols = 6, [4, 1, 2, 0]               # four columns: more than one column tile of the binning kernel
    edges = _edges(4, 1024)
    x = hr.matrix_for(edges, 3 * 1025 + 7 + SLAB, ld, cols, seed=1024)
    got = _forms(eng, x, cols, edges, pairs=False)
    _assert_numpy(got, x, cols, edges, pairs=False)


@pytest.mark.parametrize("mask", ["drops 30 %", "drops all"])
def test_mask_equals_the_compacted_matrix(eng, mask):
    import torch
    ld, cols = 12, NINE_OF_TWELVE
    nrows = 2 * SLAB + 7
    edges = _edges(9, 20)
    x = hr.matrix_for(edges, nrows, ld, cols, seed=30)
    ok = (np.random.default_rng(30).random(nrows) >= 0.3) if mask == "drops 30 %" else np.zeros(nrows, bool)
    got = _forms(eng, x, cols, edges, ok=ok)
    lohi, nfin = eng.marginals_range(x, cols, ok)
    d_lohi, d_nfin = eng.marginals_range(torch.from_numpy(x).cuda(), cols, torch.from_numpy(ok.astype(np.uint8)).cuda())
    assert np.array_equal(d_lohi.cpu().numpy().view(np.uint64), lohi.view(np.uint64))
    assert np.array_equal(d_nfin.cpu().numpy().astype(np.uint64), nfin)
    if mask == "drops all":
        assert all(not a.any() for a in got) and np.isnan(lohi).all() and not nfin.any()
        return
    assert 0.6 * nrows < ok.sum() < 0.8 * nrows
    _assert_numpy(got, x, cols, edges, ok=ok)
    compact = eng.marginals(np.ascontiguousarray(x[ok]), cols, edges)
    assert all(np.array_equal(g, c) for g, c in zip(got, compact))
    want, wn = hr.numpy_range(x, cols, ok)
    assert np.array_equal(lohi.view(np.uint64), want.view(np.uint64)) and np.array_equal(nfin, wn)


@pytest.mark.parametrize("pattern", ["one cell", "two cells by lane"])
def test_full_contention(eng, pattern):
    """A posterior as narrow as it gets: every lane of every wave adds to the same LDS word (or to one of two)."""
    nrows, ld, cols = 2 * SLAB + 7, 4, [2, 0, 3]
    edges = _edges(3, 20)
    x = np.full((nrows, ld), np.nan)
    for s, c in enumerate(cols):
        mid = 0.5 * (edges[s, 3:5].sum()), 0.5 * (edges[s, 11:13].sum())
        x[:, c] = mid[0] if pattern == "one cell" else np.where(np.arange(nrows) % 2 == 0, mid[0], mid[1])
    got = _forms(eng, x, cols, edges)
    _assert_numpy(got, x, cols, edges)
    ncells = 1 if pattern == "one cell" else 2
    assert np.all((got[2] > 0).sum(axis=(1, 2)) == ncells) and np.all(got[2].sum(axis=(1, 2)) == nrows)
    assert not got[1].any()


def test_same_bytes_twice_and_at_other_slabs(eng):
    ld, cols = 12, NINE_OF_TWELVE
    edges = _edges(9, 20)
    x = hr.matrix_for(edges, 2 * SLAB + 7, ld, cols, seed=77)
    ok = np.random.default_rng(77).random(x.shape[0]) < 0.8
    a = _forms(eng, x, cols, edges, ok=ok)
    b = _forms(eng, x, cols, edges, ok=ok)
    ra = eng.marginals_range(x, cols, ok)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    try:
        for rows in (64, 0):
            eng.marginals_set_slab(rows)
            assert eng.marginals_slab() == rows or (rows == 0 and eng.marginals_slab() >= 1024)
            c = _forms(eng, x, cols, edges, ok=ok)
            assert all(p.tobytes() == q.tobytes() for p, q in zip(a, c)), rows
            rc = eng.marginals_range(x, cols, ok)
            assert all(p.tobytes() == q.tobytes() for p, q in zip(ra, rc)), rows
    finally:
        eng.marginals_set_slab(SLAB)
    _assert_numpy(a, x, cols, edges, ok=ok)


def test_upload_chunks_of_100_rows_equal_the_device_form(eng):
    import torch
    ld, cols = 12, NINE_OF_TWELVE
    edges = _edges(9, 20)
    x = hr.matrix_for(edges, 2 * SLAB + 7, ld, cols, seed=100)
    ok = np.random.default_rng(100).random(x.shape[0]) < 0.9
    d_x, d_ok = torch.from_numpy(x).cuda(), torch.from_numpy(ok.astype(np.uint8)).cuda()
    dev = [t.cpu().numpy().astype(np.uint64) for t in eng.marginals(d_x, cols, edges, ok=d_ok)]
    d_lohi, d_nfin = eng.marginals_range(d_x, cols, d_ok)
    try:
        eng.marginals_set_chunk(100)
        host = eng.marginals(x, cols, edges, ok=ok)
        lohi, nfin = eng.marginals_range(x, cols, ok)
    finally:
        eng.marginals_set_chunk(0)
    assert all(np.array_equal(h, d) for h, d in zip(host, dev))
    assert np.array_equal(lohi.view(np.uint64), d_lohi.cpu().numpy().view(np.uint64))
    assert np.array_equal(nfin, d_nfin.cpu().numpy().astype(np.uint64))
    _assert_numpy(host, x, cols, edges, ok=ok)


@pytest.mark.parametrize("chunk", [0, 100])
def test_host_forms_read_no_further_than_the_last_selected_column(eng, chunk):
    """A padded matrix whose memory ends with the last selected column of its last row; uploaded whole and in chunks of
    100 rows, where only the last chunk ends early."""
    nrows, cols = 257, [4, 1, 6]
    ncols = max(cols) + 1
    ld = ncols + 5
    edges = _edges(3, 20)
    flat = np.full((nrows - 1) * ld + ncols, np.nan)
    x = np.lib.stride_tricks.as_strided(flat, (nrows, ncols), (8 * ld, 8))
    for s, c in enumerate(cols):
        x[:, c] = hr.column_for(edges[s], nrows, 4100 + s)
    try:
        eng.marginals_set_chunk(chunk)
        got = eng.marginals(x, cols, edges)
        lohi, nfin = eng.marginals_range(x, cols)
    finally:
        eng.marginals_set_chunk(0)
    _assert_numpy(got, x, cols, edges)
    want, wn = hr.numpy_range(x, cols)
    assert np.array_equal(lohi.view(np.uint64), want.view(np.uint64)) and np.array_equal(nfin, wn)


def test_device_and_host_calls_alternate_on_the_scratch(eng):
    """marginals on a CUDA tensor and a side stream, marginals_range on the host array, three times over: both entry
    points and both kinds of staging go through the one scratch (csrc/scratch.hpp)."""
    import torch
    cols = [2, 0, 1]
    edges = _edges(3, 20)
    x = hr.matrix_for(edges, 2 * SLAB + 1, 3, cols, seed=55)
    d_x = torch.from_numpy(x).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    want, wn = hr.numpy_range(x, cols)
    for _ in range(3):
        with torch.cuda.stream(side):              # (the results are made and zeroed on the stream the call runs on)
            dev = eng.marginals(d_x, cols, edges)
        lohi, nfin = eng.marginals_range(x, cols)
        assert np.array_equal(lohi.view(np.uint64), want.view(np.uint64)) and np.array_equal(nfin, wn)
        side.synchronize()
        _assert_numpy([t.cpu().numpy().astype(np.uint64) for t in dev], x, cols, edges)


def test_range_special_columns(eng):
    rng = np.random.default_rng(12)
    n = SLAB + 9
    x = rng.normal(size=(n, 5)) * 10.0 ** rng.integers(-300, 300, (n, 5))
    x[::7, 1], x[3::7, 1], x[5::7, 1] = np.inf, -np.inf, np.nan
    x[5::9, 2], x[6::9, 2] = -0.0, 0.0
    x[:, 3] = np.nan
    x[:, 4] = np.where(np.arange(n) % 2 == 0, -0.0, 0.0)
    lohi, nfin = eng.marginals_range(x, [4, 1, 3, 2, 0])
    want, wn = hr.numpy_range(x, [4, 1, 3, 2, 0])
    assert np.array_equal(nfin, wn) and np.array_equal(lohi[1:].view(np.uint64), want[1:].view(np.uint64))
    assert np.array_equal(lohi[0], want[0]) and np.signbit(lohi[0, 0]) and not np.signbit(lohi[0, 1])
    assert np.isnan(lohi[2]).all() and nfin[2] == 0


def test_hpd_is_the_restatement(eng):
    rng = np.random.default_rng(3)
    for counts in ([5, 9, 9, 5, 9, 1], [17], [0, 0, 0], [1, 30, 40, 2, 0, 1, 35, 38, 3, 0], [50, 25, 15, 10],
                   list(rng.integers(0, 1000, 128))):
        for p in (0.5, 0.6827, 0.75, 0.9545, 1.0):
            mask, thr, inc, runs = eng.hpd(counts, p)
            wmask, wthr, winc, wruns = hr.hpd_restate(counts, p)
            assert np.array_equal(mask, wmask) and (thr, inc, runs) == (wthr, winc, wruns), (counts, p)


# ---- refusals ---------------------------------------------------------------------------------------------------
def _raw(dev, nrows=20, ld=4, cols=(1, 3), nbins=5, edges=None, pairs=True, null=(), x=None, fill=7):
    """bartrt_marginals / _dev through ctypes with pre-filled outputs: -> (rc, message, h1, out, h2)."""
    import torch
    from bart_amd import transit_module as trm
    lib = trm.lib()
    nsel = len(cols)
    nb, ns = max(min(nbins, 1025), 1), max(nsel, 1)
    c = np.ascontiguousarray(cols if nsel else [0], np.int32)
    e = np.tile(np.linspace(0.0, 1.0, nb + 1), (ns, 1)) if edges is None else np.ascontiguousarray(edges, np.double)
    x = np.random.default_rng(0).random((20, 4)) if x is None else x
    h1, out = np.full((ns, nb), fill, np.uint64), np.full((ns, 3), fill, np.uint64)
    h2 = np.full((max(ns * (ns - 1) // 2, 1), min(nb, 128), min(nb, 128)), fill, np.uint64)
    if dev:
        keep = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda() for a in (x, h1, out, h2)]
        px, p1, po, p2 = (C.c_void_p(t.data_ptr()) for t in keep)
    else:
        px, p1, po, p2 = (trm._ptr(a) for a in (x, h1, out, h2))
    arg = lambda name, v: None if name in null else v
    args = [arg("x", px), nrows, ld, None, nsel, arg("cols", trm._ptr(c)), nbins, arg("edges", trm._ptr(e)),
            arg("h1", p1), arg("out", po), p2 if pairs else None]
    rc = lib.bartrt_marginals_dev(*args, None) if dev else lib.bartrt_marginals(*args)
    msg = lib.bartrt_last_error().decode()
    if dev:
        torch.cuda.synchronize()
        h1, out, h2 = (t.cpu().numpy().view(np.uint64) for t in keep[1:])
    return rc, msg, h1, out, h2


_bad_edges = lambda i, v: np.tile(np.r_[np.linspace(0.0, 1.0, 6)[:i], v, np.linspace(0.0, 1.0, 6)[i + 1:]], (2, 1))
REFUSALS = {
    "no column": (dict(cols=()), "nsel"),
    "65 columns": (dict(cols=tuple(range(4)) * 16 + (0,)), "nsel"),
    "a negative column": (dict(cols=(1, -1)), "cols[1]"),
    "a column at ld": (dict(cols=(4, 1)), "cols[0]"),
    "ld below the largest column + 1": (dict(ld=3), "ld"),
    "no bin": (dict(nbins=0), "nbins"),
    "1025 bins": (dict(nbins=1025, pairs=False), "nbins"),
    "129 bins with pairs": (dict(nbins=129), "nbins"),
    "edges not increasing": (dict(edges=_bad_edges(3, 0.3)), "edges[0][3]"),
    "an edge repeated": (dict(edges=_bad_edges(2, 0.2)), "edges[0][2]"),
    "an infinite edge": (dict(edges=_bad_edges(5, np.inf)), "edges[0][5]"),
    "a NaN edge": (dict(edges=_bad_edges(0, np.nan)), "edges[0][0]"),
    "no row": (dict(nrows=0), "nrows"),
    "2^31 rows": (dict(nrows=2 ** 31), "nrows"),
    "x is NULL": (dict(null=("x",)), "x"),
    "cols is NULL": (dict(null=("cols",)), "cols"),
    "edges is NULL": (dict(null=("edges",)), "edges"),
    "h1 is NULL": (dict(null=("h1",)), "h1"),
    "out is NULL": (dict(null=("out",)), "out"),
}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_name_the_argument_and_touch_nothing(eng, case, dev):
    kw, name = REFUSALS[case]
    rc, msg, h1, out, h2 = _raw(dev, **kw)
    assert rc == EINVAL and name in msg, msg
    assert msg.startswith("marginals_dev: " if dev else "marginals: ")
    assert np.all(h1 == 7) and np.all(out == 7) and np.all(h2 == 7)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_one_column_with_pairs_wanted_leaves_h2_alone(eng, dev):
    x = hr.matrix_for(_edges(1, 5), 2 * SLAB + 7, 4, [2], seed=1)
    rc, msg, h1, out, h2 = _raw(dev, nrows=x.shape[0], cols=(2,), edges=_edges(1, 5), x=x)
    assert rc == 0, msg
    want = hr.numpy_counts(x, [2], _edges(1, 5), pairs=False)
    assert np.array_equal(h1, want[0]) and np.array_equal(out, want[1]) and np.all(h2 == 7)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_129_bins_without_pairs_are_served(eng, dev):
    x = hr.matrix_for(_edges(2, 129), 500, 4, [1, 3], seed=129)
    rc, msg, h1, out, h2 = _raw(dev, nrows=500, nbins=129, edges=_edges(2, 129), pairs=False, x=x)
    assert rc == 0, msg
    want = hr.numpy_counts(x, [1, 3], _edges(2, 129), pairs=False)
    assert np.array_equal(h1, want[0]) and np.array_equal(out, want[1]) and np.all(h2 == 7)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_range_refusals(eng, dev):
    import torch
    from bart_amd import transit_module as trm
    lib = trm.lib()
    x = np.random.default_rng(0).random((20, 4))
    d_x = torch.from_numpy(x).cuda()
    for kw, name in ((dict(cols=()), "nsel"), (dict(cols=(0,) * 65), "nsel"), (dict(cols=(0, 4)), "cols[1]"),
                     (dict(cols=(-1,)), "cols[0]"), (dict(nrows=0), "nrows"), (dict(nrows=2 ** 31), "nrows"),
                     (dict(null="x"), "x"), (dict(null="cols"), "cols"), (dict(null="lohi"), "lohi")):
        cols = kw.get("cols", (1, 3))
        c = np.ascontiguousarray(cols if cols else [0], np.int32)
        lohi, nfin = np.full((max(len(cols), 1), 2), 7.0), np.full(max(len(cols), 1), 7, np.uint64)
        if dev:
            d_lohi, d_nfin = torch.from_numpy(lohi).cuda(), torch.from_numpy(nfin.view(np.int64)).cuda()
            px, pl, pn = (C.c_void_p(t.data_ptr()) for t in (d_x, d_lohi, d_nfin))
        else:
            px, pl, pn = trm._ptr(x), trm._ptr(lohi), trm._ptr(nfin)
        null = kw.get("null")
        args = [None if null == "x" else px, kw.get("nrows", 20), 4, None, len(cols),
                None if null == "cols" else trm._ptr(c), None if null == "lohi" else pl, pn]
        rc = lib.bartrt_marginals_range_dev(*args, None) if dev else lib.bartrt_marginals_range(*args)
        msg = lib.bartrt_last_error().decode()
        assert rc == EINVAL and name in msg, (kw, msg)
        if dev:
            torch.cuda.synchronize()
            lohi, nfin = d_lohi.cpu().numpy(), d_nfin.cpu().numpy()
        assert np.all(lohi == 7.0) and np.all(nfin == 7)


def test_hpd_refusals(eng):
    from bart_amd import transit_module as trm
    for counts, p, name in (([1, 2], 0.0, "p"), ([1, 2], 1.5, "p"), ([1, 2], float("nan"), "p"), ([], 0.5, "nbins")):
        with pytest.raises(trm.TransitError, match=name):
            eng.hpd(counts, p)


# ---- the posterior layer ----------------------------------------------------------------------------------------
def _chain(nfree, layout, seed):
    """A synthetic output.npy: stepsize with fixed parameters between the free ones; the last free parameter (nfree
    >= 2) never moved.  -> (array, stepsize)."""
    rng = np.random.default_rng(seed)
    nchains, niter = 3, 101
    npars = nfree + 2
    stepsize = np.full(npars, 0.1)
    stepsize[[1, npars - 1]] = 0.0
    free = np.nonzero(stepsize)[0]
    walk = rng.normal(size=(nchains, niter, nfree)) * 10.0 ** rng.integers(-2, 3, nfree) + rng.normal(size=nfree)
    walk[:, :, 0] = 0.1 * rng.normal(size=(nchains, niter)) + np.where(rng.random((nchains, niter)) < 0.5, 0.0, 3.0)   # bimodal
    if nfree >= 2:
        walk[:, :, -1] = 1234.5
    if layout == "mc3":
        return np.ascontiguousarray(walk.transpose(0, 2, 1)), stepsize
    full = np.zeros((nchains, niter, npars))
    full[:, :, free] = walk
    return full, stepsize


@pytest.mark.parametrize("layout", ["mc3", "retrieve"])
@pytest.mark.parametrize("nfree", [1, 2, 5])
def test_posterior_marginals_against_numpy(eng, tmp_path, nfree, layout):
    from bart_amd import posterior
    data, stepsize = _chain(nfree, layout, seed=nfree)
    burnin, thinning, nbins = 11, 3, 20
    path = str(tmp_path / "output.npy")
    np.save(path, data)
    m = posterior.marginals(path, stepsize, burnin, thinning, nbins=nbins, layout=layout)
    kept = data[:, :, burnin::thinning].transpose(0, 2, 1) if layout == "mc3" else data[:, burnin::thinning][:, :, stepsize > 0]
    stacked = kept.reshape(-1, nfree)
    assert m["nsamples"] == stacked.shape[0] == 3 * 30
    assert np.array_equal(m["index"], np.nonzero(stepsize > 0)[0])
    pairs = [(a, b) for a in range(nfree) for b in range(a + 1, nfree)]
    assert np.array_equal(m["pairs"], np.array([(m["index"][a], m["index"][b]) for a, b in pairs]).reshape(-1, 2))
    assert m["hist2d"].shape == (len(pairs), nbins, nbins) and m["hist"].shape == (nfree, nbins)
    for s in range(nfree):
        counts, edges = np.histogram(stacked[:, s], bins=nbins)
        assert np.array_equal(m["hist"][s], counts) and np.array_equal(m["edges"][s], edges)
        assert not m["outside"][s].any()
        for l, p in enumerate((0.6827, 0.9545)):
            mask, _, _, runs = hr.hpd_restate(counts, p)
            inc = np.nonzero(mask)[0]
            assert np.array_equal(m["hpd_mask"][l, s], mask) and m["hpd_runs"][l, s] == runs
            assert m["hpd_lo"][l, s] == edges[inc[0]] and m["hpd_hi"][l, s] == edges[inc[-1] + 1]
    for k, (a, b) in enumerate(pairs):
        assert np.array_equal(m["hist2d"][k], np.histogram2d(stacked[:, a], stacked[:, b], bins=nbins)[0])
    assert m["hpd_runs"][0, 0] == 2                                  # the bimodal parameter
    if nfree >= 2:                                                   # the one that never moved: lo - 0.5, hi + 0.5
        assert m["edges"][-1, 0] == 1234.0 and m["edges"][-1, -1] == 1235.0 and m["hist"][-1, nbins // 2] == 90
    # given ranges, and the .npz
    ranges = np.stack([stacked.min(axis=0) + 0.25 * np.ptp(stacked, axis=0), stacked.max(axis=0) + 1.0], axis=1)
    g = posterior.marginals(data, stepsize, burnin, thinning, nbins=7, ranges=ranges, layout=layout)
    for s in range(nfree):
        want = np.histogram(stacked[:, s], bins=7, range=tuple(ranges[s]))[0]
        assert np.array_equal(g["hist"][s], want)
        assert g["outside"][s, 0] == (stacked[:, s] < ranges[s, 0]).sum() and g["outside"][s, 1] == 0
    posterior.save(str(tmp_path / "m.npz"), m)
    z = np.load(str(tmp_path / "m.npz"))
    assert all(np.array_equal(z[k], m[k]) for k in m)


MARGINAL_KEYS = {"index", "edges", "hist", "outside", "pairs", "hist2d", "levels", "hpd_mask", "hpd_lo", "hpd_hi",
                 "hpd_runs", "nsamples", "burnin"}


def test_retrieve_writes_marginals(tmp_path):
    """`retrieve --resident --marginals m.npz --marginals-bins 12` on the short chain of the T(p)-envelope test: the
    file lies beside output.npy, holds the documented keys, and its counts are numpy's on the written chain."""
    from test_gpu_cf_params import worker_case
    from bart_amd import BARTfunc, cf, retrieve
    case, base, wcfg, pmin, pmax = worker_case(str(tmp_path / "case"), "eclipse")
    params, stepsize = cf._mcmc_vectors(base)
    w = BARTfunc.Worker(wcfg, carry=False)
    try:
        data = w.step(params)[0]
    finally:
        w.close()
    line = lambda v: " ".join(repr(float(x)) for x in v)
    cfg = str(tmp_path / "run.cfg")
    with open(cfg, "w") as f:
        f.write(open(base).read())
        f.write("pmin = %s\npmax = %s\ndata = %s\nuncert = %s\n" % (line(pmin), line(pmax), line(data), line(0.02 * np.abs(data))))
        f.write("nchains = 4\nnumit = 160\nburnin = 10\nwalk = snooker\nseed = 3\n")
    out = str(tmp_path / "o")
    res = retrieve.main(["-c", cfg, "--resident", "--marginals", "m.npz", "--marginals-bins", "12", "--out", out])
    z = np.load(os.path.join(out, "m.npz"))
    assert set(z.files) == MARGINAL_KEYS and int(z["burnin"]) == 10
    chain = np.load(os.path.join(out, "output.npy"))
    free = np.nonzero(stepsize > 0)[0]
    assert np.array_equal(z["index"], free) and z["hist"].shape == (len(free), 12)
    stacked = chain[:, 10:, :].reshape(-1, chain.shape[2])
    assert int(z["nsamples"]) == stacked.shape[0]
    for s, j in enumerate(free):
        assert np.array_equal(z["hist"][s], np.histogram(stacked[:, j], bins=12)[0])
    a, b = z["pairs"][1]
    assert np.array_equal(z["hist2d"][1], np.histogram2d(stacked[:, a], stacked[:, b], bins=12)[0])
    assert all(np.array_equal(res["marginals"][k], z[k]) for k in z.files)
