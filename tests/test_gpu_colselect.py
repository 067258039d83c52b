"""GPU: column-wise multi-rank selection (include/bartrt.h, bartrt_colselect / _dev; csrc/quant.hip).  Every result
is held to np.sort(x[ok], axis=0)[rank] as uint64 views (the two zeros compare equal): order statistics are selected,
not computed, so there is no tolerance anywhere in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quant_restate as qr  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def eng(small_case):
    from bart_amd import engine, transit_module as trm
    engine.init(small_case.tcfg)
    yield engine
    trm.free_memory()


def _matrix(nrows, ncols, seed):
    """The adversarial columns cycled over ncols, with draws in between."""
    adv = qr.adversarial_columns(max(nrows, 2), seed)[:nrows]
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(nrows, ncols)) * 1000.0
    for c in range(0, ncols, 2):
        x[:, c] = adv[:, (c // 2) % adv.shape[1]]
    return x


def _ranks_for(n, seed):
    rng = np.random.default_rng(seed)
    return [[0], [n - 1], [0, n - 1], [n // 2] * 3 + [0], list(rng.integers(0, n, 16))]


def _slab_rows():
    from bart_amd import engine
    s = engine.colselect_slab()
    return [s - 1, s, s + 1, 3 * s + 7]


@pytest.mark.parametrize("ncols", [1, 3, 64, 100])
@pytest.mark.parametrize("nrows", [1, 2, 63, 64, 65, 257, "slab-1", "slab", "slab+1", "3slab+7"])
def test_shapes_against_np_sort(eng, nrows, ncols):
    """The partial wave, the slab seam, the multi-workgroup merge and the padded row, host and device forms."""
    import torch
    if isinstance(nrows, str):
        nrows = dict(zip(["slab-1", "slab", "slab+1", "3slab+7"], _slab_rows()))[nrows]
    x = _matrix(nrows, ncols, seed=nrows * 131 + ncols)
    for pad in (0, 5):
        wide = np.full((nrows, ncols + pad), np.nan)        # (the padding would show at the high ranks)
        wide[:, :ncols] = x
        view = wide[:, :ncols]
        d_wide = torch.from_numpy(wide).cuda()
        for ranks in _ranks_for(nrows, nrows + ncols + pad)[(0 if pad == 0 else 3):]:
            want = qr.sorted_ranks(x, ranks)
            got = eng.colselect(view, ranks)
            assert qr.same_bits(got, want), (nrows, ncols, pad, ranks)
            d_got = eng.colselect(d_wide[:, :ncols], ranks)
            assert qr.same_bits(d_got.cpu().numpy(), want), (nrows, ncols, pad, ranks)


def test_special_values_and_a_nan_column(eng):
    n = 130
    rng = np.random.default_rng(9)
    x = _matrix(n, 9, seed=9)
    x[:, 1] = qr.SPECIALS[:-1][rng.integers(0, 8, n)]
    x[:, 4] = np.where(rng.random(n) < 0.3, np.nan, x[:, 4])
    x[:, 6] = np.nan
    ranks = [n - 1, 0, n - 2, n // 2, n - 1, 1]           # unsorted, with a duplicate
    want = qr.sorted_ranks(x, ranks)
    got = eng.colselect(x, ranks)
    assert qr.same_bits(got, want)
    nn = int(np.isnan(x[:, 4]).sum())
    assert 2 <= nn < n // 2 and np.isnan(got[0, 4]) and np.isnan(got[2, 4]) and not np.isnan(got[3, 4])
    assert np.all(np.isnan(got[:, 6]))
    assert not np.isnan(got[:, [0, 1, 2, 3, 5, 7, 8]]).any()      # the neighbours are untouched


@pytest.mark.parametrize("mask", ["ones", "every other", "one row"])
def test_mask_equals_the_compacted_matrix(eng, mask):
    import torch
    n = eng.colselect_slab() + 70
    x = _matrix(n, 37, seed=4)
    ok = {"ones": np.ones(n, bool), "every other": np.arange(n) % 2 == 1, "one row": np.arange(n) == n - 3}[mask]
    m = int(ok.sum())
    ranks = sorted({0, m - 1, m // 2, m // 3})
    want = qr.sorted_ranks(x, ranks, ok)
    got = eng.colselect(x, ranks, ok)
    assert qr.same_bits(got, want)
    assert got.tobytes() == eng.colselect(np.ascontiguousarray(x[ok]), ranks).tobytes()
    if mask == "ones":
        assert got.tobytes() == eng.colselect(x, ranks).tobytes()
    d_got = eng.colselect(torch.from_numpy(x).cuda(), ranks, torch.from_numpy(ok.astype(np.uint8)).cuda())
    assert d_got.cpu().numpy().tobytes() == got.tobytes()


def test_no_row_left(eng):
    """All rows masked: BARTRT_EINVAL from the host form; the device form cannot look and writes NaN.  So does a rank
    at or above the rows that count, for that rank alone."""
    import torch
    from bart_amd import transit_module as trm
    x = _matrix(40, 5, seed=2)
    with pytest.raises(trm.TransitError, match="no row"):
        eng.colselect(x, [0], np.zeros(40))
    d_x, none = torch.from_numpy(x).cuda(), torch.zeros(40, dtype=torch.uint8, device="cuda")
    assert bool(torch.isnan(eng.colselect(d_x, [0, 3], none)).all())
    ok = np.arange(40) < 10
    with pytest.raises(trm.TransitError, match=r"ranks\[1\]"):
        eng.colselect(x, [9, 10], ok)
    got = eng.colselect(d_x, [9, 10, 0], torch.from_numpy(ok.astype(np.uint8)).cuda()).cpu().numpy()
    assert np.all(np.isnan(got[1])) and qr.same_bits(got[[0, 2]], qr.sorted_ranks(x, [9, 0], ok))


def test_same_bytes_twice_and_at_another_slab(eng):
    n = 3 * eng.colselect_slab() + 7
    x = _matrix(n, 70, seed=6)
    ok = np.random.default_rng(6).random(n) < 0.8
    ranks = list(np.random.default_rng(7).integers(0, int(ok.sum()), 16))
    a = eng.colselect(x, ranks, ok)
    assert a.tobytes() == eng.colselect(x, ranks, ok).tobytes()
    default = eng.colselect_slab()
    try:
        for rows in (1, 100, 2 * default):
            eng.colselect_set_slab(rows)
            assert eng.colselect_slab() == rows
            assert a.tobytes() == eng.colselect(x, ranks, ok).tobytes(), rows
    finally:
        eng.colselect_set_slab(0)
    assert eng.colselect_slab() == default
    assert qr.same_bits(a, qr.sorted_ranks(x, ranks, ok))


# ---- the engine's scratch serves one call at a time (csrc/scratch.hpp) -------------------------------------------
def test_two_streams_share_the_scratch(eng):
    """Two selections back to back on two streams, nothing waited for in between: two slabs and two column tiles each,
    so that the slab merge and the global histogram both go through the scratch the calls share."""
    import torch
    n = eng.colselect_slab() + 1
    xs = [_matrix(n, 65, seed=21), _matrix(n, 65, seed=22)]
    ranks = [[0, n - 1, n // 2, n // 2, 7], [n // 3, 1, n - 2]]
    want = [qr.sorted_ranks(x, r) for x, r in zip(xs, ranks)]
    d_xs = [torch.from_numpy(x).cuda() for x in xs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got = []
    for rep in range(8):
        for i in ((0, 1) if rep % 2 == 0 else (1, 0)):
            got.append((rep, i, eng.colselect(d_xs[i], ranks[i], stream=streams[i])))
    torch.cuda.synchronize()
    for rep, i, g in got:
        assert qr.same_bits(g.cpu().numpy(), want[i]), (rep, i)


def test_scratch_regrows_between_calls(eng, small_case):
    """A new engine's scratch grows with the first call, grows again with a larger one while the first may still run,
    and serves the first matrix again on another stream while the second may still run."""
    import torch
    from bart_amd import transit_module as trm
    trm.free_memory()
    eng.init(small_case.tcfg)                       # (the scratch is the engine's: empty again)
    small, large = _matrix(65, 1, seed=31), _matrix(eng.colselect_slab() + 1, 100, seed=32)
    r_small, r_large = [64, 0, 32], list(np.random.default_rng(33).integers(0, large.shape[0], 16))
    d_small, d_large = torch.from_numpy(small).cuda(), torch.from_numpy(large).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    first = eng.colselect(d_small, r_small)
    second = eng.colselect(d_large, r_large)
    third = eng.colselect(d_small, r_small, stream=side)
    torch.cuda.synchronize()
    first, second, third = (t.cpu().numpy() for t in (first, second, third))
    assert qr.same_bits(first, qr.sorted_ranks(small, r_small)) and qr.same_bits(second, qr.sorted_ranks(large, r_large))
    assert third.tobytes() == first.tobytes()


def test_host_form_reads_no_further_than_the_last_column(eng):
    """A padded matrix whose memory ends with the last column of its last row."""
    nrows, ncols = 257, 7
    ld = ncols + 5
    flat = np.random.default_rng(41).normal(size=(nrows - 1) * ld + ncols)
    x = np.lib.stride_tricks.as_strided(flat, (nrows, ncols), (8 * ld, 8))
    ranks = [0, 256, 128, 1]
    assert qr.same_bits(eng.colselect(x, ranks), qr.sorted_ranks(x, ranks))


# ---- refusals: one test each ------------------------------------------------------------------------------------
def _call(x, nrows, ncols, ld, ranks, dev=False):
    from bart_amd import transit_module as trm
    lib = trm.lib()
    r = np.ascontiguousarray(ranks, np.int64)
    out = np.zeros((max(len(r), 1), max(ncols, 1)))
    if dev:
        import torch
        d_x, d_out = torch.from_numpy(x).cuda(), torch.from_numpy(out).cuda()
        rc = lib.bartrt_colselect_dev(C.c_void_p(d_x.data_ptr()), nrows, ncols, ld, None, len(r), trm._ptr(r),
                                      C.c_void_p(d_out.data_ptr()), None)
    else:
        rc = lib.bartrt_colselect(trm._ptr(x), nrows, ncols, ld, None, len(r), trm._ptr(r), trm._ptr(out))
    return rc, lib.bartrt_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
def test_refuses_too_many_ranks(eng, dev):
    x = np.zeros((20, 4))
    rc, msg = _call(x, 20, 4, 4, list(range(17)), dev)
    assert rc == EINVAL and "nranks" in msg


@pytest.mark.parametrize("dev", [False, True])
def test_refuses_no_ranks(eng, dev):
    rc, msg = _call(np.zeros((20, 4)), 20, 4, 4, [], dev)
    assert rc == EINVAL and "nranks" in msg


@pytest.mark.parametrize("dev", [False, True])
def test_refuses_a_negative_rank(eng, dev):
    rc, msg = _call(np.zeros((20, 4)), 20, 4, 4, [3, -1], dev)
    assert rc == EINVAL and "ranks[1]" in msg


@pytest.mark.parametrize("dev", [False, True])
def test_refuses_ld_below_ncols(eng, dev):
    rc, msg = _call(np.zeros((20, 4)), 20, 4, 3, [0], dev)
    assert rc == EINVAL and "ld" in msg


@pytest.mark.parametrize("dev", [False, True])
def test_refuses_no_rows(eng, dev):
    rc, msg = _call(np.zeros((20, 4)), 0, 4, 4, [0], dev)
    assert rc == EINVAL and "nrows" in msg


def test_host_form_refuses_a_rank_beyond_the_rows(eng):
    rc, msg = _call(np.zeros((20, 4)), 20, 4, 4, [19, 20])
    assert rc == EINVAL and "ranks[1]" in msg and "20" in msg


def test_percentile_rule_needs_no_engine():
    from bart_amd import transit_module as trm
    lib = trm.lib()
    lo, hi, w = C.c_long(), C.c_long(), C.c_double()
    assert lib.bartrt_percentile_rule(10, 50.0, C.byref(lo), C.byref(hi), C.byref(w)) == 0
    assert (lo.value, hi.value, w.value) == (4, 5, 0.5)
    assert lib.bartrt_percentile_rule(0, 50.0, C.byref(lo), C.byref(hi), C.byref(w)) == EINVAL
