"""The Gelman-Rubin statistic of bart_amd/csrc/gr_core.hpp restated in plain Python, twice: in doubles, every sum in
the header's order (the bits a build of the header must give), and in exact rationals (what the doubles are measured
against).  Also the chains, the host program (tests/gr_core_host.cpp) and the measured accuracy bound that
tests/test_gr_core_cpu.py and tests/test_gpu_mcmc_converge.py share."""
import math
import os
import subprocess
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 256          # gr::kTile
MIN_ROWS = 4        # gr::kMinRows
THRESHOLD = 1.01    # gr::kThreshold


def leaf(col, lo, hi):
    s = 0.0
    for r in range(lo, hi):
        s += col[r]
    n = float(hi - lo)
    mean = s / n
    m2 = 0.0
    for r in range(lo, hi):
        d = col[r] - mean
        m2 += d * d
    return [n, mean, m2]


def merge(a, b):
    na, nb = a[0], b[0]
    n = na + nb
    d = b[1] - a[1]
    return [n, a[1] + (d * nb) / n, a[2] + (b[2] + (((d * d) * na) * nb) / n)]


def triple(col, r0, r1):
    a = leaf(col, r0, min(r0 + TILE, r1))
    for lo in range(r0 + TILE, r1, TILE):
        a = merge(a, leaf(col, lo, min(lo + TILE, r1)))
    return a


def psrf_of(ts):
    nch, n = len(ts), ts[0][0]
    w = m = 0.0
    for t in ts:
        w += t[2] / (n - 1.0)
        m += t[1]
    w = w / nch
    m = m / nch
    b = 0.0
    for t in ts:
        d = t[1] - m
        b += d * d
    b = n * b / (nch - 1)
    num = (n - 1.0) / n * w + b / n
    if w == 0.0:                                  # what IEEE division gives
        return math.inf if num > 0.0 else math.nan
    return math.sqrt(num / w)


def statistic(chain, stepsize, r0, r1, threshold=0.0):
    """psrf [npars], triples [nch, npars, 3], converged: the header's gr::statistic, operation for operation."""
    nch, nkept, npars = chain.shape
    psrf, triples = np.zeros(npars), np.zeros((nch, npars, 3))
    if nch < 2 or r1 - r0 < MIN_ROWS:
        return psrf, triples, 0
    free = [j for j in range(npars) if stepsize[j] > 0]
    for j in free:
        cols = [chain[i, :, j].tolist() for i in range(nch)]
        ts = [triple(c, r0, r1) for c in cols]
        triples[:, j] = ts
        psrf[j] = psrf_of(ts)
    thr = threshold if threshold != 0.0 else THRESHOLD
    ok = len(free) > 0 and all(math.isfinite(psrf[j]) and psrf[j] < thr for j in free)
    return psrf, triples, int(ok)


def exact(chain, stepsize, r0, r1):
    """R of every free parameter from exact rational arithmetic, as Decimals of 60 digits (None where W = 0);
    0 for the others."""
    nch, _, npars = chain.shape
    n = r1 - r0
    out = []
    for j in range(npars):
        if not stepsize[j] > 0:
            out.append(Decimal(0))
            continue
        means, m2 = [], []
        for i in range(nch):
            x = [Fraction(v) for v in chain[i, r0:r1, j].tolist()]
            mu = sum(x) / n
            means.append(mu)
            m2.append(sum((v - mu) ** 2 for v in x))
        W = sum(v / (n - 1) for v in m2) / nch
        mm = sum(means) / nch
        B = n * sum((v - mm) ** 2 for v in means) / (nch - 1)
        if W == 0:
            out.append(None)
            continue
        R2 = (Fraction(n - 1, n) * W + B / n) / W
        with localcontext() as ctx:
            ctx.prec = 60
            out.append((Decimal(R2.numerator) / Decimal(R2.denominator)).sqrt())
    return out


def deviation(psrf, want):
    """Largest relative deviation of the doubles psrf from the exact values (parameters with a defined R alone)."""
    worst = 0.0
    with localcontext() as ctx:
        ctx.prec = 60
        for got, w in zip(np.asarray(psrf).tolist(), want):
            if w is None or w == 0:
                continue
            assert math.isfinite(got), (got, w)
            worst = max(worst, float(abs(Decimal(got) - w) / w))
    return worst


def stepsizes(npars):
    """Free parameters with fixed (0) and shared (-1: a copy of the first) ones between them; the first is free."""
    return np.array([0.0 if j % 5 == 2 else -1.0 if j % 7 == 3 else 0.05 + 0.01 * (j % 3) for j in range(npars)])


def make_chain(nch, nkept, npars, seed):
    """Random chains whose columns differ in scale: column 1 (where there is one) has mean 1e8 and spread 1, column 4
    a radius of 97 000 with a spread of 3; the chains' means differ by a fraction of the spread."""
    rng = np.random.default_rng(seed)
    centre = np.array([[-2.0, 1e8, 0.0, 0.5, 97000.0, -0.5, 1e-3][j % 7] for j in range(npars)])
    spread = np.array([[0.01, 1.0, 0.1, 0.2, 3.0, 0.05, 1e-5][j % 7] for j in range(npars)])
    shift = 0.3 * rng.normal(size=(nch, 1, npars))
    return np.ascontiguousarray(centre + spread * (rng.normal(size=(nch, nkept, npars)) + shift))


# (rows of the test, chains, parameters, r0): every row count of the issue with every chain count, the parameter
# counts spread over them, and row ranges that do not start at the chain's first row
ROWS = (4, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
SHAPES = [(rows, nch, npars, r0)
          for a, rows in enumerate(ROWS) for b, nch in enumerate((2, 3, 10))
          for npars, r0 in [((1, 7, 64)[(a + b) % 3], (0, 3, 300)[(a + 2 * b) % 3])]]
# the shapes on which accuracy is measured in exact rationals: seven parameters (columns of every scale)
EXACT_SHAPES = [(rows, nch, 7, r0) for rows, nch, r0 in ((4, 2, 0), (TILE - 1, 3, 3), (TILE + 1, 10, 0),
                                                          (3 * TILE + 5, 3, 300), (3 * TILE + 5, 10, 3))]


def case(shape):
    rows, nch, npars, r0 = shape
    nkept = r0 + rows + 2                                        # (rows past r1 exist and must not be read)
    return make_chain(nch, nkept, npars, seed=1000 * rows + 10 * nch + npars), stepsizes(npars), r0, r0 + rows


def build_host(tmpdir):
    """tests/gr_core_host.cpp built with g++ and the address / undefined-behaviour sanitizers; returns
    run(mode, chain, stepsize, r0, r1, threshold) -> psrf, triples, converged."""
    exe = os.path.join(str(tmpdir), "gr_core_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "gr_core_host.cpp"), "-o", exe])
    count = [0]

    def run(mode, chain, stepsize, r0, r1, threshold=0.0):
        nch, nkept, npars = chain.shape
        count[0] += 1
        fin, fout = (os.path.join(str(tmpdir), "%s%d.bin" % (k, count[0])) for k in ("in", "out"))
        np.concatenate([[nch, nkept, npars, r0, r1, threshold], np.asarray(stepsize, float),
                        np.ascontiguousarray(chain, float).ravel()]).tofile(fin)
        r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        v = np.fromfile(fout)
        os.remove(fin)
        os.remove(fout)
        assert v.size == npars + nch * npars * 3 + 2 and v[-1] == 1.0
        return v[:npars], v[npars:-2].reshape(nch, npars, 3), int(v[-2])
    return run


def numpy_psrf(chain, stepsize, r0, r1):
    from bart_amd import sampler
    free = np.where(np.asarray(stepsize) > 0)[0]
    out = np.zeros(chain.shape[2])
    out[free] = sampler.gelman_rubin(chain[:, r0:r1][:, :, free])
    return out


_measured = {}


def measure(host):
    """Deviation from the exact value of the host build and of numpy's sampler.gelman_rubin over EXACT_SHAPES, and the
    bound the tests assert: 8 x the larger, and no less than 8 x 2^-53 (half a unit in the last place of a double:
    what a correctly rounded R itself may deviate)."""
    if not _measured:
        dev = {"host": 0.0, "numpy": 0.0, "onepass": 0.0}
        for shape in EXACT_SHAPES:
            chain, step, r0, r1 = case(shape)
            want = exact(chain, step, r0, r1)
            dev["host"] = max(dev["host"], deviation(host("stat", chain, step, r0, r1)[0], want))
            dev["numpy"] = max(dev["numpy"], deviation(numpy_psrf(chain, step, r0, r1), want))
            one = host("onepass", chain, step, r0, r1)[0]
            one = np.where(np.isfinite(one), one, 1e300)                   # (a negative variance: no digit right)
            dev["onepass"] = max(dev["onepass"], deviation(one[[1]], want[1:2]))       # the 1e8 column alone
        dev["bound"] = 8.0 * max(dev["host"], dev["numpy"], 2.0 ** -53)
        _measured.update(dev)
        print("Gelman-Rubin accuracy against exact rationals: host build %.3g, numpy %.3g, one-pass on the 1e8 "
              "column %.3g; bound %.3g" % (dev["host"], dev["numpy"], dev["onepass"], dev["bound"]))
    return _measured
