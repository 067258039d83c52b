"""CPU: the display rule of bart_amd/csrc/specenv_core.hpp through a stand-alone host program
(tests/specenv_core_host.cpp, its own main, built here with g++ and the address / undefined-behaviour sanitizers) that
runs the very functions the device kernel runs.  The rule is held to its numpy restatement (tests/specenv_restate.py)
bit for bit and to scipy.ndimage.gaussian_filter1d within the bound derived there."""
import os
import sys

import numpy as np
import pytest
from scipy.ndimage import correlate1d, gaussian_filter1d

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import specenv_restate as sr  # noqa: E402

RPRS = 0.0931


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return sr.build_host(tmp_path_factory.mktemp("specenv_core"))


def _rows(W, nrows=3, seed=0):
    """Non-negative rows of a spectrum's dynamic range, and a stellar flux."""
    rng = np.random.default_rng(1000 * W + seed)
    x = rng.random((nrows, W)) * 10.0 ** rng.integers(-3, 4, (nrows, W))
    sflux = 1e5 * (1.0 + rng.random(W))
    return x, sflux


def test_gauss_half_is_scipys_kernel():
    """bart_amd.posterior.gauss_half, the function that makes the library's weights, against SciPy's own
    _gaussian_kernel1d byte for byte -- radius, weights and normalisation -- and the tests' copy against it."""
    from scipy.ndimage import _filters
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bart_amd import posterior
    for sigma, truncate, radius in ((2.0, 4.0, 8), (0.5, 4.0, 2), (16.0, 4.0, 64), (0.1, 4.0, 0), (1.3, 4.0, 5),
                                    (3.0, 2.5, 8), (7.77, 4.0, 31)):
        half = posterior.gauss_half(sigma, truncate)
        assert half.size == radius + 1 == int(truncate * sigma + 0.5) + 1
        assert sr.same_bytes(half, _filters._gaussian_kernel1d(sigma, 0, radius)[radius:])
        if truncate == 4.0:
            assert sr.same_bytes(half, sr.gauss_half(sigma))
    assert sr.same_bytes(posterior.gauss_half(0.1), [1.0])
    # and through the filter itself: the weights SciPy smooths with at the figure's sigma
    x = np.zeros(41)
    x[20] = 1.0
    assert sr.same_bytes(gaussian_filter1d(x, 2)[20:29], posterior.gauss_half(2.0))
    with pytest.raises(ValueError):
        posterior.gauss_half(0.0)


def test_reflect_index_is_the_half_sample_symmetric_extension(host):
    for W in (1, 2, 3, 7, 8):
        i = np.arange(-5 * W - 3, W + 5 * W + 3)
        want = np.pad(np.arange(W), (5 * W + 3, 5 * W + 3), mode="symmetric")     # numpy's name for d c b a | a b c d
        assert np.array_equal(sr.reflect_index(i, W), want)
        assert np.array_equal(sr.host_reflect(host, i, W), want)


@pytest.mark.parametrize("W", [1, 2, 7, 8, 9, 16, 17, 18, 200])
@pytest.mark.parametrize("star", [True, False])
def test_radius_8_row_lengths(host, W, star):
    """Shorter than the radius (1, 2, 7: the reflection repeats), equal to it, one above it, 2r, 2r + 1, 2r + 2."""
    half = sr.gauss_half(2.0)
    assert half.size == 9
    x, sflux = _rows(W)
    sflux = sflux if star else None
    got = sr.host_display(host, x, sflux, RPRS, half)
    assert sr.same_bytes(got, sr.display_rows(x, sflux, RPRS, half))
    y = x / sflux * RPRS * RPRS if star else x
    want = gaussian_filter1d(y, 2, axis=1)
    print("W = %3d: worst difference from SciPy %.2f units of 2^-53 (bound %.1f)"
          % (W, sr.worst_units(got, want), sr.scipy_bound(8) / sr.U))
    assert sr.within_scipy_bound(got, want, 8)


def test_radius_0_is_the_identity(host):
    x, sflux = _rows(13)
    assert sr.same_bytes(sr.host_display(host, x, None, RPRS, [1.0]), x)
    assert sr.same_bytes(sr.host_display(host, x, sflux, RPRS, [1.0]), x / sflux * RPRS * RPRS)
    # the weight is not read: the identity whatever half[0] says
    assert sr.same_bytes(sr.host_display(host, x, None, RPRS, [0.5]), x)
    assert sr.same_bytes(sr.display_rows(x, None, RPRS, [0.5]), x)


def test_radius_64_on_three_samples(host):
    half = sr.gauss_half(16.0)
    assert half.size == sr.MAX_RADIUS + 1
    x, sflux = _rows(3)
    got = sr.host_display(host, x, sflux, RPRS, half)
    assert sr.same_bytes(got, sr.display_rows(x, sflux, RPRS, half))
    want = correlate1d(x / sflux * RPRS * RPRS, np.r_[half[:0:-1], half], axis=1, mode="reflect")
    assert sr.within_scipy_bound(got, want, 64)
    assert sr.within_scipy_bound(got, gaussian_filter1d(x / sflux * RPRS * RPRS, 16, axis=1), 64)


@pytest.mark.parametrize("W", [17, 199])
def test_strides_keep_every_stride_th_sample(host, W):
    half = sr.gauss_half(2.0)
    x, sflux = _rows(W, seed=2)
    full = sr.host_display(host, x, sflux, RPRS, half, 1)
    for stride in (2, 3):
        assert W % stride != 0
        got = sr.host_display(host, x, sflux, RPRS, half, stride)
        assert got.shape == (3, -(-W // stride))
        assert sr.same_bytes(got, full[:, ::stride])
        assert sr.same_bytes(got, sr.display_rows(x, sflux, RPRS, half, stride))


def test_the_bound_is_the_derived_one():
    """n = 2r + 2 roundings: 36 u at the figure's radius, above the few u observed and far below a wrong weight."""
    assert sr.scipy_bound(8) == pytest.approx(36.0 * sr.U, rel=1e-14)
    assert 3.7 * sr.U < sr.scipy_bound(8) < 1e-14
