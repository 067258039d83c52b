"""Shared by tests/test_hist_core_cpu.py and tests/test_gpu_marginals.py: the host program's builder, the edge families
and the special values every binning test uses, numpy's counts as the reference, and restatements in plain Python of
the highest-density region and of a deliberately WRONG binning (bart_amd/csrc/hist_core.hpp)."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = ("uniform", "log", "narrow")


def build_host(tmpdir):
    """tests/hist_core_host.cpp built with g++ and the address / undefined-behaviour sanitizers; returns
    run(mode, words) -> the output file's 64-bit words as uint64."""
    exe = os.path.join(str(tmpdir), "hist_core_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "hist_core_host.cpp"), "-o", exe])
    count = [0]

    def run(mode, words):
        count[0] += 1
        fin, fout = (os.path.join(str(tmpdir), "%s%d.bin" % (k, count[0])) for k in ("in", "out"))
        np.ascontiguousarray(words, np.double).tofile(fin)
        r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        v = np.fromfile(fout, np.uint64)
        os.remove(fin)
        os.remove(fout)
        return v
    return run


def host_marginals(run, x, cols, edges, ok=None, pairs=True):
    """hist::marginals -> (h1 [nsel, nbins], out [nsel, 3], h2 [npairs, nbins, nbins] or None)."""
    x, edges = np.ascontiguousarray(x, np.double), np.ascontiguousarray(edges, np.double)
    nsel, nbins = len(cols), edges.shape[1] - 1
    head = [x.shape[0], x.shape[1], nsel, nbins, 0 if ok is None else 1, 1 if pairs else 0]
    parts = [head, np.asarray(cols, float), edges.ravel()] + ([] if ok is None else [np.asarray(ok, float)]) + [x.ravel()]
    v = run("bin", np.concatenate(parts))
    n1 = nsel * nbins
    h2 = v[n1 + 3 * nsel:].reshape(-1, nbins, nbins) if pairs else None
    return v[:n1].reshape(nsel, nbins), v[n1:n1 + 3 * nsel].reshape(nsel, 3), h2


def host_range(run, x, cols, ok=None):
    """hist::marginals_range -> (lohi [nsel, 2], nfinite [nsel])."""
    x = np.ascontiguousarray(x, np.double)
    head = [x.shape[0], x.shape[1], len(cols), 0 if ok is None else 1]
    parts = [head, np.asarray(cols, float)] + ([] if ok is None else [np.asarray(ok, float)]) + [x.ravel()]
    v = run("range", np.concatenate(parts))
    return v[:2 * len(cols)].view(np.double).reshape(-1, 2), v[2 * len(cols):]


def host_hpd(run, counts, p):
    v = run("hpd", np.concatenate([[len(counts), p], np.asarray(counts, float)]))
    n = len(counts)
    return v[:n].astype(bool), int(v[n]), int(v[n + 1]), int(v[n + 2])


# ---- edges and values -------------------------------------------------------------------------------------------
def edges_of(family, nbins):
    """nbins + 1 strictly increasing finite edges with 0.0 among them: uniform from np.linspace, log-spaced, and
    uniform with one bin a single ulp wide."""
    if family == "uniform":
        return np.linspace(0.0, 4.0, nbins + 1)
    if family == "log":
        return np.concatenate([[0.0], np.logspace(-5.0, 1.0, nbins)])
    if family == "narrow":
        e = np.linspace(0.0, 4.0, nbins + 1)
        k = nbins // 2
        e[k + 1] = np.nextafter(e[k], np.inf)
        return e
    raise ValueError(family)


def special_values(e):
    """Every edge, its neighbours one ulp to either side, both infinities, NaN, both zeros, a value below and a value
    above the range."""
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                           [np.inf, -np.inf, np.nan, -0.0, 0.0, e[0] - 1.0, e[-1] + 1.0]])


def column_for(e, nrows, seed):
    """nrows values for the edges e: the special values (all of them once nrows allows) and draws over a range a
    little wider than the edges', shuffled."""
    rng = np.random.default_rng(seed)
    pool = special_values(e)
    rng.shuffle(pool)
    w = e[-1] - e[0]
    draws = e[0] - 0.1 * w + 1.2 * w * rng.random(max(nrows - pool.size, 0))
    col = np.concatenate([pool, draws])[:nrows]
    rng.shuffle(col)
    return col


def matrix_for(edges, nrows, ld, cols, seed):
    """x [nrows, ld], NaN where no selected column lies (a read outside the selection would show), column cols[s] made
    for edges[s]."""
    x = np.full((nrows, ld), np.nan)
    for s, c in enumerate(cols):
        x[:, c] = column_for(edges[s], nrows, seed * 1000 + s)
    return x


# ---- the reference: numpy ---------------------------------------------------------------------------------------
def numpy_counts(x, cols, edges, ok=None, pairs=True):
    """(h1, out, h2) by np.histogram, numpy comparisons and np.histogram2d on the rows ok keeps."""
    x = np.asarray(x, np.double)
    if ok is not None:
        x = x[np.asarray(ok, bool)]
    nsel, nbins = len(cols), edges.shape[1] - 1
    h1, out = np.zeros((nsel, nbins), np.uint64), np.zeros((nsel, 3), np.uint64)
    for s, c in enumerate(cols):
        v = x[:, c]
        h1[s] = np.histogram(v[np.isfinite(v)], bins=edges[s])[0]
        out[s] = [(v < edges[s, 0]).sum(), (v > edges[s, -1]).sum(), np.isnan(v).sum()]
    if not pairs:
        return h1, out, None
    h2 = []
    for a in range(nsel):
        for b in range(a + 1, nsel):
            va, vb = x[:, cols[a]], x[:, cols[b]]
            fin = np.isfinite(va) & np.isfinite(vb)
            h2.append(np.histogram2d(va[fin], vb[fin], bins=[edges[a], edges[b]])[0])
    h2 = np.array(h2, np.uint64).reshape(-1, nbins, nbins)
    return h1, out, h2


def numpy_range(x, cols, ok=None):
    x = np.asarray(x, np.double)
    if ok is not None:
        x = x[np.asarray(ok, bool)]
    lohi, n = np.full((len(cols), 2), np.nan), np.zeros(len(cols), np.uint64)
    for s, c in enumerate(cols):
        v = x[:, c][np.isfinite(x[:, c])]
        n[s] = v.size
        if v.size:
            lohi[s] = np.nanmin(v), np.nanmax(v)
    return lohi, n


# ---- restatements in plain Python -------------------------------------------------------------------------------
def hpd_restate(counts, p):
    """The highest-density region on Python integers: -> (mask, threshold, included, nruns)."""
    counts = [int(c) for c in counts]
    n, N = len(counts), sum(counts)
    mask = [False] * n
    if N == 0:
        return np.array(mask), 0, 0, 0
    c = thr = 0
    for i in sorted(range(n), key=lambda i: (-counts[i], i)):
        mask[i] = True
        c += counts[i]
        thr = counts[i]
        if float(c) >= p * float(N):
            break
    runs = sum(1 for i in range(n) if mask[i] and (i == 0 or not mask[i - 1]))
    return np.array(mask), thr, c, runs


def wrong_uniform_only(v, e):
    """A WRONG binning on purpose: the uniform-grid estimate taken as the answer, never compared with the edges.  The
    tests show that they can tell it from the rule."""
    nbins = len(e) - 1
    v = v[np.isfinite(v) & (v >= e[0]) & (v <= e[-1])]
    g = np.minimum(np.floor((v - e[0]) * (nbins / (e[-1] - e[0]))).astype(np.int64), nbins - 1)
    return np.bincount(g, minlength=nbins).astype(np.uint64)
