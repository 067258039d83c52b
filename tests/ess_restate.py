"""The effective sample size of bart_amd/csrc/ess_core.hpp restated in plain Python doubles, every sum in the header's
order (the bits a build of the header must give), the lagged sums once more in exact rationals, and the chains, the
cases and the host program (tests/ess_core_host.cpp) that tests/test_ess_core_cpu.py and tests/test_gpu_mcmc_ess.py
share.  The mean is gr_restate's: the header takes gr_core.hpp's and does not restate it either."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np

import gr_restate as gr

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_ROWS = gr.MIN_ROWS   # ess::testable
DEFAULT_LAG = 1024       # ess::kDefaultLag
MAX_LAG = 4096           # ess::kMaxLag


def lags(maxlag, n):
    return min(maxlag if maxlag else DEFAULT_LAG, n - 1)


def div(a, b):
    """a / b as IEEE arithmetic gives it (Python raises where b is zero)."""
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def mean(col, r0, r1):
    return gr.triple(col, r0, r1)[1]


def lagged_sums(col, r0, r1, m, K):
    """S_0 .. S_K: one accumulator each, ascending rows, differences first, then the product, then the add."""
    d = [x - m for x in col[r0:r1]]
    out = []
    for k in range(K + 1):
        s = 0.0
        for a, b in zip(d, d[k:]):
            s += a * b
        out.append(s)
    return out


def tau_of(S, K):
    s0, tot, stopped = S[0], 0.0, False
    t = 0
    while 2 * t + 1 <= K:
        p = div(S[2 * t], s0) + div(S[2 * t + 1], s0)
        if p <= 0.0:
            stopped = True
            break
        tot += p
        t += 1
    return -1.0 + 2.0 * tot, int(not stopped)


def reached_of(ess, truncated, stepsize, target):
    free = [j for j in range(len(stepsize)) if stepsize[j] > 0]
    return int(len(free) > 0 and all(math.isfinite(ess[j]) and ess[j] >= target and not truncated[:, j].any()
                                     for j in free))


def statistic(chain, stepsize, r0, r1, maxlag=0, target=0.0):
    """tau [nch, npars], ess [npars], truncated [nch, npars], acf [nch, npars, K + 1], means [nch, npars], reached:
    the header's ess::statistic, operation for operation."""
    nch, nkept, npars = chain.shape
    n = r1 - r0
    K = lags(maxlag, n)
    tau, ess, trunc = np.zeros((nch, npars)), np.zeros(npars), np.zeros((nch, npars), np.int32)
    acf, means = np.zeros((nch, npars, max(K + 1, 0))), np.zeros((nch, npars))
    if n < MIN_ROWS:
        return tau, ess, trunc, acf, means, 0
    for j in range(npars):
        if not stepsize[j] > 0:
            continue
        e = 0.0
        for i in range(nch):
            col = chain[i, :, j].tolist()
            means[i, j] = mean(col, r0, r1)
            S = lagged_sums(col, r0, r1, means[i, j], K)
            acf[i, j] = S
            tau[i, j], trunc[i, j] = tau_of(S, K)
            e += div(float(n), float(tau[i, j]))
        ess[j] = e
    return tau, ess, trunc, acf, means, reached_of(ess, trunc, stepsize, target)


def exact_sums(col, r0, r1, m, K):
    """(S_k, sum_r |d_r d_{r+k}|) for k = 0 .. K in exact rationals, the differences taken about the double m."""
    d = [Fraction(x) - Fraction(m) for x in col[r0:r1]]
    return [(sum(a * b for a, b in zip(d, d[k:])), sum(abs(a * b) for a, b in zip(d, d[k:]))) for k in range(K + 1)]


def make_chain(nch, nkept, npars, seed, phi=0.8):
    """Correlated chains (a first-order autoregression of coefficient phi in every column) whose columns differ in
    scale as gr_restate.make_chain's do: column 4 is a radius of 97 000 with a spread of 3."""
    rng = np.random.default_rng(seed)
    centre = np.array([[-2.0, 1e8, 0.0, 0.5, 97000.0, -0.5, 1e-3][j % 7] for j in range(npars)])
    spread = np.array([[0.01, 1.0, 0.1, 0.2, 3.0, 0.05, 1e-5][j % 7] for j in range(npars)])
    e = rng.normal(size=(nch, nkept, npars))
    z = np.empty_like(e)
    z[:, 0] = e[:, 0]
    for r in range(1, nkept):
        z[:, r] = phi * z[:, r - 1] + math.sqrt(1.0 - phi * phi) * e[:, r]
    return np.ascontiguousarray(centre + spread * z)


def one_free(npars, j):
    step = np.zeros(npars)
    step[j] = 0.05
    return step


# The issue's shapes.  n: below one window of the lags kernel (4, 5), one row past a window (257), several (1 300);
# maxlag: 1, the lane-block edge (255 / 256 / 257) and 4 096, which exceeds n - 1 everywhere and must clamp; one chain
# and three; every range starts past the chain's first row.  Seven parameters carry a fixed (2) and a shared (3) column.
def _cases():
    out = []
    for n in (4, 5, 257, 1300):
        for nch in (1, 3):
            for maxlag in (1, 255, 256, 257, 4096):
                out.append(dict(id="n%d-ch%d-lag%d" % (n, nch, maxlag), n=n, nch=nch, npars=7, r0=3, maxlag=maxlag))
    out.append(dict(id="n257-ch3-lag0-p64-onefree", n=257, nch=3, npars=64, r0=5, maxlag=0, free=37))
    out.append(dict(id="n1300-ch1-lag256-p64-onefree", n=1300, nch=1, npars=64, r0=1, maxlag=256, free=63))
    out.append(dict(id="n257-ch3-lag256-constant", n=257, nch=3, npars=7, r0=3, maxlag=256, constant=4))
    return out


CASES = _cases()


def case(c):
    """chain, stepsize, r0, r1, maxlag of a case; rows past r1 exist and must not be read."""
    nkept = c["r0"] + c["n"] + 2
    chain = make_chain(c["nch"], nkept, c["npars"], seed=7000 + 10 * c["n"] + c["nch"] + c["maxlag"] % 97)
    step = one_free(c["npars"], c["free"]) if "free" in c else gr.stepsizes(c["npars"])
    if "constant" in c:
        chain[:, :, c["constant"]] = 97000.0
    return chain, step, c["r0"], c["r0"] + c["n"], c["maxlag"]


_reference = {}


def reference(host, c):
    """The host build's outputs of a case, computed once and shared by the tests that need them."""
    if c["id"] not in _reference:
        chain, step, r0, r1, maxlag = case(c)
        _reference[c["id"]] = host(chain, step, r0, r1, maxlag, 10.0)
    return _reference[c["id"]]


def same(a, b):
    """Byte for byte, NaNs apart: IEEE 754 leaves the sign and the payload of a NaN that an operation makes to the
    implementation (0 / 0 is the negative "indefinite" on x86, the positive quiet NaN in Python and on the GPU), so NaNs
    are held to lie at the same places and every other value to be the same bytes."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes()


def build_host(tmpdir):
    """tests/ess_core_host.cpp built with g++ and the address / undefined-behaviour sanitizers; returns
    run(chain, stepsize, r0, r1, maxlag, target) -> dict(tau, ess, truncated, acf, mean, reached)."""
    exe = os.path.join(str(tmpdir), "ess_core_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "ess_core_host.cpp"), "-o", exe])
    count = [0]

    def run(chain, stepsize, r0, r1, maxlag=0, target=0.0):
        nch, nkept, npars = chain.shape
        count[0] += 1
        fin, fout = (os.path.join(str(tmpdir), "%s%d.bin" % (k, count[0])) for k in ("in", "out"))
        np.concatenate([[nch, nkept, npars, r0, r1, maxlag, target], np.asarray(stepsize, float),
                        np.ascontiguousarray(chain, float).ravel()]).tofile(fin)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        v = np.fromfile(fout)
        os.remove(fin)
        os.remove(fout)
        pairs, K = nch * npars, lags(maxlag, r1 - r0)
        nacf = pairs * (K + 1) if K >= 0 else 0
        assert v.size == 3 * pairs + npars + nacf + 2 and v[-1] == 1.0
        cut = np.cumsum([pairs, npars, pairs, nacf, pairs])
        tau, ess, trunc, acf, mean_ = np.split(v[:-2], cut)[:5]
        return dict(tau=tau.reshape(nch, npars), ess=ess, truncated=trunc.reshape(nch, npars).astype(np.int32),
                    acf=acf.reshape(nch, npars, max(K + 1, 0)), mean=mean_.reshape(nch, npars), reached=int(v[-2]))
    return run
