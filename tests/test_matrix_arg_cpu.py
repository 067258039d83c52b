"""engine._matrix_arg: the one place where colselect, marginals and marginals_range turn their matrix argument into
(array, nrows, ld, x pointer, ok, ok pointer, is_host).  numpy inputs only: no device and no library are touched."""
import numpy as np
import pytest

from bart_amd import engine


def _arg(x, ok=None, who="colselect"):
    a, nrows, ld, xp, m, mp, host = engine._matrix_arg(x, ok, who)
    assert host and a.dtype == np.double and a.ndim == 2 and nrows == a.shape[0] and xp.value == a.ctypes.data
    assert (m is None and mp is None) or (m.dtype == np.uint8 and m.flags.c_contiguous and mp.value == m.ctypes.data)
    # what the library reads, row by row at ld doubles, is the matrix
    flat = np.lib.stride_tricks.as_strided(a, (nrows, a.shape[1]), (8 * ld, 8))
    assert np.array_equal(flat, a, equal_nan=True)
    return a, ld, m


def test_contiguous_is_taken_as_it_lies():
    x = np.arange(15.0).reshape(5, 3)
    a, ld, m = _arg(x)
    assert a is x and ld == 3 and m is None


def test_padded_view_is_read_in_place():
    wide = np.arange(40.0).reshape(5, 8)
    a, ld, _ = _arg(wide[:, :3])
    assert ld == 8 and a.ctypes.data == wide.ctypes.data and np.shares_memory(a, wide)


def test_transposed_is_copied():
    x = np.arange(15.0).reshape(3, 5).T
    a, ld, _ = _arg(x)
    assert ld == a.shape[1] == 3 and not np.shares_memory(a, x) and np.array_equal(a, x)


def test_column_stride_is_copied():
    wide = np.arange(40.0).reshape(5, 8)
    a, ld, _ = _arg(wide[:, ::2])
    assert ld == 4 and not np.shares_memory(a, wide) and np.array_equal(a, wide[:, ::2])


def test_single_row_with_an_odd_stride():
    buf = np.arange(10.0)
    x = np.lib.stride_tricks.as_strided(buf, (1, 3), (8, 8))      # a row stride below ncols: no second row to reach
    a, ld, _ = _arg(x)
    assert a.shape == (1, 3) and ld == 3 and a.ctypes.data == buf.ctypes.data


def test_float32_is_converted():
    x = np.arange(15, dtype=np.float32).reshape(5, 3)
    a, ld, _ = _arg(x)
    assert ld == 3 and np.array_equal(a, x.astype(np.double))


def test_one_and_three_dimensions_are_reshaped():
    a, ld, _ = _arg(np.arange(4.0))
    assert a.shape == (1, 4) and ld == 4
    x = np.arange(24.0).reshape(2, 3, 4)
    a, ld, _ = _arg(x)
    assert a.shape == (6, 4) and ld == 4 and np.array_equal(a, x.reshape(6, 4))


@pytest.mark.parametrize("who", ["colselect", "marginals", "marginals_range"])
def test_ok_of_wrong_length_names_the_caller(who):
    x = np.zeros((5, 3))
    for ok in (np.ones(4), np.ones(6), np.ones((5, 1))):
        with pytest.raises(ValueError) as err:
            engine._matrix_arg(x, ok, who)
        assert str(err.value) == who + ": ok must have one entry per row"


@pytest.mark.parametrize("ok", [[True, False, True, True, False], [2, 0, -1, 7, 0], [0.5, 0.0, 1.0, np.nan, 0.0]])
def test_ok_becomes_zero_or_one_bytes(ok):
    _, _, m = _arg(np.zeros((5, 3)), ok)
    assert m.shape == (5,) and m.tolist() == [1, 0, 1, 1, 0]
