"""GPU: Gaussian kernel density estimates (include/bartrt.h, bartrt_kde / _dev, bartrt_hpd_pdf; csrc/kde.hip) and
bart_amd.posterior.marginals_of_samples(kde=True).  The reference is the mpmath restatement of tests/kde_restate.py at a
fixed, named subset of grid indices -- with exp_rt's own formula for the exponential, which is what the 4e-16 of
tests/test_gpu_rt_math.py is measured against; the distance of that formula from exp is computed beside it and is what
the comparison with scipy is allowed on top -- under the bound derived there; between
forms, chunks, leading dimensions, calls and streams the criterion is equality of bits.  The cases are those of
tests/test_kde_core_cpu.py, placed around the rule's tile T = bartrt_kde_tile()."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kde_restate as kr  # noqa: E402

pytestmark = pytest.mark.gpu
CASE_NAMES = list(kr.make_cases(2048))
BITS_CASE = "2T+3 rows x 128 points, masked, inf and NaN in the data"


@pytest.fixture(scope="module")
def eng():
    from bart_amd import engine
    assert engine.kde_tile() >= 256          # (fails on a library without bartrt_kde)
    engine.kde_set_chunk(0)
    yield engine
    engine.kde_set_chunk(0)


@pytest.fixture(scope="module")
def cases(eng):
    return kr.make_cases(eng.kde_tile())


def _bits(result):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in result)


def _host(eng, case, x=None):
    pdf, stat, bad = eng.kde(case["x"] if x is None else x, case["cols"], case["grid"], case["bw"], ok=case["ok"])
    return pdf, stat, bad.astype(np.uint64)


def _dev(eng, case, d_x=None):
    import torch
    if d_x is None:
        d_x = torch.from_numpy(np.ascontiguousarray(case["x"])).cuda()
    d_ok = None if case["ok"] is None else torch.from_numpy(case["ok"].astype(np.uint8)).cuda()
    pdf, stat, bad = eng.kde_dev(d_x, case["cols"], case["grid"], case["bw"], d_ok)
    return pdf.cpu().numpy(), stat.cpu().numpy(), bad.cpu().numpy().astype(np.uint64)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cases_within_the_bound_of_mpmath_and_forms_agree(eng, cases, name):
    """Every shape and content of the list: the host form and the device form give the same bits, the moments and the
    densities at the named indices are within the derived bound of mpmath, non-finite values are counted, degenerate
    columns are NaN beside good ones."""
    case, T = cases[name], eng.kde_tile()
    host = _host(eng, case)
    assert _bits(host) == _bits(_dev(eng, case))
    pdf, stat, bad = host
    for s, c in enumerate(case["cols"]):
        idx = kr.named_indices(case["grid"][s], stat[s, 1])
        ref = kr.exact_column(case["x"], c, case["grid"][s], idx, case["bw"], case["ok"], T, kr.EPS_EXP_DEVICE,
                              device=True)
        kr.assert_column(name, s, ref, pdf[s], stat[s], bad[s], idx)
    if name == "grid points so far out that every term is dropped":
        assert np.all(pdf[0, ::2] == 0.0) and np.all(pdf[0, 1::2] > 0.0)
    if name == "a constant column and an n = 1 column beside a good one":
        assert np.isnan(pdf[:2]).all() and np.isnan(stat[:2, 3]).all() and np.isfinite(pdf[2]).all()
    if name == BITS_CASE:
        assert np.all(bad >= 1)


def test_same_bits_under_chunks_leading_dimensions_calls_and_streams(eng, cases):
    import torch
    case, T = cases[BITS_CASE], eng.kde_tile()
    want = _bits(_host(eng, case))
    try:
        for rows in (T, 2 * T, 0):             # one tile, a multiple of the tile, the default
            eng.kde_set_chunk(rows)
            assert eng.kde_chunk() == rows
            assert _bits(_host(eng, case)) == want, rows
            assert _bits(_dev(eng, case)) == want, rows
        eng.kde_set_chunk(T + 1)               # (rounded up to two tiles)
        assert _bits(_host(eng, case)) == want
    finally:
        eng.kde_set_chunk(0)
    nrows, ld = case["x"].shape
    wide = np.full((nrows, ld + 4), np.nan)
    wide[:, :ld] = case["x"]
    assert _bits(_host(eng, case, x=wide[:, :ld])) == want          # a padded view, read in place at ld + 4
    assert _bits(_dev(eng, case, torch.from_numpy(wide).cuda()[:, :ld])) == want
    # two consecutive calls on one stream, then one on a second stream: the scratch rule
    d_x = torch.from_numpy(case["x"]).cuda()
    d_ok = torch.from_numpy(case["ok"].astype(np.uint8)).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    first = eng.kde_dev(d_x, case["cols"], case["grid"], case["bw"], d_ok)
    second = eng.kde_dev(d_x, case["cols"], case["grid"], case["bw"], d_ok)
    with torch.cuda.stream(side):
        third = eng.kde_dev(d_x, case["cols"], case["grid"], case["bw"], d_ok)
    side.synchronize()
    torch.cuda.synchronize()
    for got in (first, second, third):
        pdf, stat, bad = (t.cpu().numpy() for t in got)
        assert _bits((pdf, stat, bad.astype(np.uint64))) == want


def test_host_form_reads_no_further_than_the_last_selected_column(eng):
    """A padded matrix whose memory ends with the last selected column of its last row."""
    T = eng.kde_tile()
    nrows, cols = T + 5, [4, 1, 6]
    ncols, ld = 7, 12
    flat = np.full((nrows - 1) * ld + ncols, np.nan)
    x = np.lib.stride_tricks.as_strided(flat, (nrows, ncols), (8 * ld, 8))
    rng = np.random.default_rng(3)
    for c in cols:
        x[:, c] = rng.normal(size=nrows)
    grid = np.stack([np.linspace(-3.0, 3.0, 65)] * 3)
    got = eng.kde(x, cols, grid, "scott")
    want = eng.kde(np.ascontiguousarray(x), cols, grid, "scott")
    assert _bits(got) == _bits(want) and np.all(got[1][:, 0] == nrows)


def _chain(seed):
    """Stacked samples [n, npars]: free parameters 0, 2, 3 and 4 among fixed ones; 0 bimodal, 3 radius-like, 4 never
    moved."""
    rng = np.random.default_rng(seed)
    n = 1500
    x = np.zeros((n, 6))
    x[:, 0] = kr._column("bimodal", n, rng)
    x[:, 2] = kr._column("normal", n, rng)
    x[:, 3] = kr._column("radius", n, rng)
    x[:, 4] = 1234.5
    return x, np.array([0, 2, 3, 4])


def test_posterior_marginals_with_kde(eng):
    import torch
    from scipy.stats import gaussian_kde
    from bart_amd import posterior
    x, index = _chain(5)
    base = posterior.marginals_of_samples(x, index, nbins=20)
    m = posterior.marginals_of_samples(x, index, nbins=20, kde=True, kde_points=65, kde_bw="silverman")
    assert set(m) == set(base) | {"kde_x", "kde_pdf", "kde_bw", "mean", "std", "cr_mask", "cr_lo", "cr_hi", "cr_runs"}
    for k in base:                            # every pre-existing key exactly as without kde
        assert np.asarray(m[k]).dtype == np.asarray(base[k]).dtype
        assert np.asarray(m[k]).tobytes() == np.asarray(base[k]).tobytes(), k
    dev = posterior.marginals_of_samples(torch.from_numpy(x).cuda(), index, nbins=20, kde=True, kde_points=65,
                                         kde_bw="silverman")
    assert all(np.asarray(m[k]).tobytes() == np.asarray(dev[k]).tobytes() for k in m)
    assert m["kde_pdf"].shape == m["kde_x"].shape == (4, 65)
    for s in range(4):
        assert np.array_equal(m["kde_x"][s], np.linspace(m["edges"][s, 0], m["edges"][s, -1], 65))
    assert np.isnan(m["kde_pdf"][3]).all() and np.isnan(m["kde_bw"][3]) and m["std"][3] == 0.0 and m["mean"][3] == 1234.5
    T = eng.kde_tile()
    for s in range(3):
        col = x[:, index[s]]
        idx = kr.named_indices(m["kde_x"][s], m["mean"][s])
        ref = kr.exact_column(x, index[s], m["kde_x"][s], idx, "silverman", None, T, kr.EPS_EXP_DEVICE, device=True)
        sp = gaussian_kde(col, bw_method="silverman")(m["kde_x"][s][idx])
        # scipy's own distance from the density with exp, and exp_rt's formula's distance from it
        own = np.abs(sp - ref["pdf_exp"]) + np.abs(ref["pdf"] - ref["pdf_exp"])
        assert np.all(np.abs(m["kde_pdf"][s, idx] - ref["pdf"]) <= ref["pdf_bound"])
        err = np.abs(m["kde_pdf"][s, idx] - sp)
        print("parameter %d: ours from scipy %s, allowed %s" % (index[s], err, ref["pdf_bound"] + own))
        assert np.all(err <= ref["pdf_bound"] + own)
        assert abs(m["kde_bw"][s] - ref["h"]) <= ref["h_bound"] and abs(m["std"][s] - ref["std"]) <= ref["std_bound"]
    for l, p in enumerate(m["levels"]):
        for s in range(4):
            mask, _, _, runs = kr.region_restate(m["kde_pdf"][s], p)
            assert np.array_equal(m["cr_mask"][l, s], mask) and m["cr_runs"][l, s] == runs
            if mask.any():
                assert m["cr_lo"][l, s] == m["kde_x"][s][mask].min() and m["cr_hi"][l, s] == m["kde_x"][s][mask].max()
            else:
                assert np.isnan(m["cr_lo"][l, s]) and np.isnan(m["cr_hi"][l, s])
    assert m["cr_runs"][0, 0] == 2            # the bimodal parameter at 68 %
    with pytest.raises(ValueError, match="kde_points"):
        posterior.marginals_of_samples(x, index, kde=True, kde_points=1025)
