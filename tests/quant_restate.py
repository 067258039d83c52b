"""Shared by tests/test_quant_core_cpu.py and the GPU tests of the order statistics: the host program's builder, the
adversarial columns, and the comparisons (bart_amd/csrc/quant_core.hpp)."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

PERCENTS = (50.0, 15.87, 84.13, 2.28, 97.72)      # the median and bart_amd.cf.PERCENTILES
DENORM_MIN = float(np.nextafter(0.0, 1.0))
DBL_MAX = float(np.finfo(np.double).max)
SPECIALS = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, DBL_MAX, -DBL_MAX, np.inf, -np.inf, np.nan])


def build_host(tmpdir):
    """tests/quant_core_host.cpp built with g++ and the address / undefined-behaviour sanitizers; returns
    run(mode, words) -> the output file's 64-bit words as doubles (view them as uint64 where the mode says so)."""
    exe = os.path.join(str(tmpdir), "quant_core_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "quant_core_host.cpp"), "-o", exe])
    count = [0]

    def run(mode, words):
        count[0] += 1
        fin, fout = (os.path.join(str(tmpdir), "%s%d.bin" % (k, count[0])) for k in ("in", "out"))
        np.ascontiguousarray(words, np.double).tofile(fin)
        r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        v = np.fromfile(fout)
        os.remove(fin)
        os.remove(fout)
        return v
    return run


def host_select(run, x, ranks, ok=None):
    """quant::select of every column of x [nrows, ncols] -> [nranks, ncols]."""
    x = np.ascontiguousarray(x, np.double)
    head = [x.shape[0], x.shape[1], len(ranks), 0 if ok is None else 1]
    parts = [head, np.asarray(ranks, float)] + ([] if ok is None else [np.asarray(ok, float)]) + [x.ravel()]
    return run("select", np.concatenate(parts)).reshape(len(ranks), x.shape[1])


def adversarial_columns(n, seed=0):
    """[n, 7] (n >= 2): a constant column, two distinct values, values differing only in the lowest byte, only in the
    top byte (sign and high exponent bits), mixed signs, the special values repeated, and plain normal draws."""
    rng = np.random.default_rng(seed)
    base = np.double(1234.5678).view(np.uint64)
    low = ((base & ~np.uint64(0xff)) | rng.integers(0, 256, n).astype(np.uint64)).view(np.double)
    top = ((base & ~np.uint64(0xff << 56)) | (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56))).view(np.double)
    top = np.where(np.isnan(top), 1.0, top)       # (an all-ones exponent with this mantissa would be a NaN: kept out here)
    spec = SPECIALS[:-1][rng.integers(0, len(SPECIALS) - 1, n)]
    cols = [np.full(n, -3.25), np.where(rng.random(n) < 0.5, 2.0, 2.0000000000000004), low, top,
            rng.normal(size=n) * 10.0 ** rng.integers(-300, 300, n), spec, rng.normal(size=n)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def same_bits(a, b):
    """uint64 views equal, except that the two zeros compare equal (np.sort may leave them in either order)."""
    a, b = np.ascontiguousarray(a, np.double), np.ascontiguousarray(b, np.double)
    if a.shape != b.shape:
        return False
    zero = (a == 0.0) & (b == 0.0)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | zero))


def sorted_ranks(x, ranks, ok=None):
    """np.sort(x[ok], axis=0)[ranks]: what every selection is held to."""
    x = np.asarray(x, np.double)
    if ok is not None:
        x = x[np.asarray(ok, bool)]
    return np.sort(x, axis=0)[np.asarray(ranks, np.int64)]


def within_two_ulp(got, want, lo_stat, hi_stat):
    """|got - want| <= 2 ulp of the larger neighbouring order statistic (np.spacing): one rounding in the difference
    and one in the product-and-add."""
    big = np.maximum(np.abs(lo_stat), np.abs(hi_stat))
    return bool(np.all(np.abs(np.asarray(got) - np.asarray(want)) <= 2.0 * np.spacing(big)))
