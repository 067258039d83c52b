"""Shared by tests/test_specenv_core_cpu.py and tests/test_gpu_specenv.py: a numpy restatement of the display rule of
bart_amd/csrc/specenv_core.hpp (the value, reflect_index, the fixed summation order, stride), the host program's
builder, and the bound that holds the rule to scipy.ndimage.gaussian_filter1d.

THE BOUND AGAINST SCIPY.  Both sides are given the same doubles: the same y (numpy's division and multiplications are
correctly rounded, as the header's are) and the same weights (gauss_half below is SciPy's own _gaussian_kernel1d).
They differ in the order in which the 2r + 1 products y[i] w[i] are formed and added.  Write u = 2^-53 and
gamma_n = n u / (1 - n u).  For a row without a negative value every term t_i = y[i] w[i] is non-negative, and a value
computed in ANY order is sum_i t_i (1 + theta_i) with |theta_i| <= gamma_n, n the number of roundings on the longest
path from a term to the result (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2: no
cancellation, so the relative error of the sum is that of its worst term).  Two such values a and b of the same exact
sum S > 0 therefore obey |a - b| <= 2 gamma_n S, and S <= max(a, b) / (1 - gamma_n):

    |a - b| <= 2 gamma_n / (1 - gamma_n) * max(a, b)

The roundings on the longest path.  The header's order: a pair's sum (1), its product (1), and at most r additions to
the running sum -- r + 2.  An order that forms the 2r + 1 products one by one and adds them in sequence: the product
(1) and at most 2r additions -- 2r + 1.  Pairing the terms first adds one more.  n = 2r + 2 covers every order of
pairs or single products, fused multiply-adds included (they only remove roundings).  For the figure's sigma 2
(r = 8): n = 18, and the bound is 36.0 u = 4.0e-15 relative.  (For orientation: the header's order is that of SciPy's
own loop for symmetric kernels, and an x86-64 build of SciPy 1.15.3 agrees with it bit for bit at row lengths 1 to 200;
an order that starts from the innermost pair differs by a few u there.  Another build of SciPy may contract or
reorder, so the bound is what is asserted.)  The bound assumes no product underflows; the tests' values are far from
that."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
MAX_RADIUS = 64


def scipy_bound(r):
    """2 gamma_n / (1 - gamma_n), n = 2r + 2: the relative distance (of the larger value) allowed between two
    summation orders of a non-negative row (the module's docstring)."""
    n = 2 * r + 2
    g = n * U / (1.0 - n * U)
    return 2.0 * g / (1.0 - g)


def within_scipy_bound(got, want, r):
    got, want = np.asarray(got, np.double), np.asarray(want, np.double)
    return bool(np.all(np.abs(got - want) <= scipy_bound(r) * np.maximum(np.abs(got), np.abs(want))))


def worst_units(got, want):
    """The largest relative difference in units of 2^-53, for the printed figures."""
    got, want = np.asarray(got, np.double), np.asarray(want, np.double)
    big = np.maximum(np.abs(got), np.abs(want))
    return float(np.max(np.where(big > 0, np.abs(got - want) / np.where(big > 0, big, 1.0), 0.0)) / U)


def gauss_half(sigma, truncate=4.0):
    """scipy.ndimage's Gaussian weights (_gaussian_kernel1d, order 0), restated: the half k = 0 .. radius."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:])


def reflect_index(i, W):
    """The index in [0, W) of the half-sample-symmetric extension d c b a | a b c d | d c b a at any integer i."""
    m = np.mod(np.asarray(i, np.int64), 2 * W)          # (numpy's mod of a negative number is non-negative)
    return np.where(m < W, m, 2 * W - 1 - m)


def display_value(x, sflux, rprs):
    x = np.asarray(x, np.double)
    return x if sflux is None else x / np.asarray(sflux, np.double) * rprs * rprs


def display_rows(x, sflux, rprs, half, stride=1):
    """x [nrows, W] -> [nrows, ceil(W / stride)]: the rule in the header's order -- the centre term, then the pairs
    from the outermost inwards, every operation a numpy operation on doubles (one rounding each)."""
    x = np.atleast_2d(np.asarray(x, np.double))
    half = np.asarray(half, np.double)
    r, W = half.size - 1, x.shape[1]
    y = display_value(x, sflux, rprs)
    l = np.arange(0, W, stride)
    if r == 0:
        return np.ascontiguousarray(y[:, l])
    acc = y[:, l] * half[0]
    for j in range(r, 0, -1):
        s = y[:, reflect_index(l - j, W)] + y[:, reflect_index(l + j, W)]
        acc = acc + s * half[j]
    return np.ascontiguousarray(acc)


def build_host(tmpdir):
    """tests/specenv_core_host.cpp built with g++ and the address / undefined-behaviour sanitizers (no contraction of
    multiply-adds, whatever the host's default); returns run(mode, words) -> the output file's doubles."""
    exe = os.path.join(str(tmpdir), "specenv_core_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "specenv_core_host.cpp"), "-o", exe])
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


def host_display(run, x, sflux, rprs, half, stride=1):
    """specenv::display_row of every row of x [nrows, W] -> [nrows, ceil(W / stride)]."""
    x = np.atleast_2d(np.ascontiguousarray(x, np.double))
    half = np.asarray(half, np.double)
    nrows, W = x.shape
    head = [nrows, W, half.size - 1, stride, 0 if sflux is None else 1, rprs]
    parts = [head, half] + ([] if sflux is None else [np.asarray(sflux, np.double)]) + [x.ravel()]
    return run("display", np.concatenate(parts)).reshape(nrows, -(-W // stride))


def host_reflect(run, i, W):
    return run("reflect", np.concatenate([[W], np.asarray(i, np.double)])).astype(np.int64)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, np.double), np.ascontiguousarray(b, np.double)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
