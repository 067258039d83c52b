"""Shared by tests/test_kde_core_cpu.py and tests/test_gpu_kde.py: the host program's builder, the cases both files
run, an mpmath restatement of the kernel-density rule of bart_amd/csrc/kde_core.hpp for one column with a running
error bound, and a restatement on Python floats of the credible region of a density.

THE BOUND (u = 2^-53; "1 ulp" of a library routine is taken as 2 u relative; first order in u throughout, the
products of the factors are formed explicitly where they are large).  For one column, the rows that count being i =
1 .. n, ref the column's value in row 0 (0.0 if that is not finite), y_i = x_i - ref, A = max |y_i|, Y2 = sum y_i^2,
sigma = sqrt(M2 / n), Lm = kMomentRows, T = kKdeTileRows, ntiles the tiles of the matrix and K = kLeavesPerTile + ntiles
the merges a triple can go through:

  moments   (a) y_i is rounded once: a perturbation of the data by at most u |y_i|, which moves M2 by at most
                2 u sqrt(M2 Y2) (Cauchy-Schwarz on 2 sum (y_i - mean) delta_i).
            (b) a leaf's mean is a sum of at most Lm values and a division: off by at most (Lm + 1) u A; every merge
                adds at most 7 u A (d, its product, the division and the addition, all on numbers of size <= 2 A):
                every mean is within E = (Lm + 1 + 7 K) u A.  A merge adds d^2 w, w = n_a n_b / n; d is off by at most
                2 E, so the merges together are off by at most 4 E sum |d| w <= 4 E sqrt(sum d^2 w  sum w) <=
                4 E sqrt(M2  2 n) (sum d^2 w is the between-part of M2; sum w <= n per level, two levels).
            (c) the roundings of the accumulation, all on non-negative numbers: 3 u on a leaf's term ((y - mean), its
                square), Lm u for the leaf's sum, 6 u per merge: (3 + Lm + 6 K) u relative.
            eps_M2 = u [2 sqrt(Y2 / M2) + 4 sqrt(2) (Lm + 1 + 7 K) A / sigma + 3 + Lm + 6 K]
            eps_std = eps_M2 / 2 + 3 u        (the division, the square root within 1 ulp)
            |mean' - mean| <= E + u |mean|    (the final ref + mean_y)
  factor    q^(-1/5) for Scott (q = n) and Silverman (q = 3 n / 4, exact) is one Newton step y (6 - q y^5) / 5 from the
            library's pow(q, -0.2) (kde_core.hpp, inv_fifth_root).  A seed off by d relative leaves 3 d^2; the only
            thing assumed of any pow is d <= 1e-10, which leaves 3e-20.  The step's own roundings: y^5 by four products
            (4 u), times q (u): q y^5 = 1 + 5 d is off by at most 5 u (1 + 5 d); 6 minus it, a number near 5, is then off
            by at most 5 u absolute plus its own u 5: 2 u relative; the product with y and the division by 5 add u each:
            eps_factor = 4 u + 3e-20 (with 1e-3 of slack for the second-order terms: 4.004 u).  0 for a scalar.
  h         eps_h = eps_std + eps_factor + u.
  argument  rh = 1 / h' (u), d = g - x (u), their product (u): (g - x) / h is off by eps_h + 3 u relative; the square
            and the exact halving: |a' - a| <= |a| rho, rho = 2 eps_h + 7 u.
  exp       E(a') = F(a) e^(a' - a) (1 + eps_exp), F the function E evaluates: the term t_i = F(a_i) is off by at most
            t_i r_i, r_i = (1 + eps_exp) exp(|a_i| rho (1 + 1e-10)) - 1.
            The host program: F = exp, eps_exp = 2 u (glibc documents 1 ulp for std::exp).
            The device: exp_rt is NOT exp to 4e-16.  tests/test_gpu_rt_math.py holds its fp64 evaluation to 4e-16 of
            its own FORMULA -- n the integer nearest a log2e, r = a - n ln2_d with the header's rounded ln2, a degree-9
            interpolant p(r), 2^n p(r) -- and that formula is off exp by up to 7e-14 (the interpolant) plus 2.3e-17 per
            unit of n (ln2_d).  So for the device F is the formula, restated in mpmath with the header's numbers
            (tests/rtmath_restate.py), eps_exp = 4e-16 against it, and the distance of that reference from the one
            with exp is computed beside it (pdf_exp): it is what a comparison with scipy is allowed on top.  F's
            logarithmic derivative is within 1.4e-11 of 1 inside a piece (kernels.hpp), hence the 1e-10 above; F
            jumps where n steps, by the difference of the two pieces' interpolants: a term whose a_i (1 +- rho)
            straddle a step is allowed the difference |F_n(a_i) - F_n'(a_i)| of the two pieces, computed exactly.
  dropped   a term whose computed argument is below kArgMin is zero.  A row with a_i < kArgMin - 1 is dropped for
            certain and costs t_i, an ABSOLUTE term (at most e^-709 a row); one within 1 of kArgMin may go either way
            and is allowed the larger of the two, which is t_i.
  sum       every computed term passes through at most T additions in its tile and ntiles across the tiles, one
            accumulator, all operands non-negative: a factor within gamma = (T + ntiles) u / (1 - (T + ntiles) u).
  norm      n h' (u), times sqrt(2 pi) rounded (u) and the product (u), the division (u): nu = eps_h + 4 u.
  =>  |pdf' - pdf| <= N [ sum_kept (t_i ((1 + r_i) (1 + gamma) (1 + nu) - 1) + jump_i) + sum_dropped t_i ],
      N = 1 / (n h sqrt(2 pi)), pdf = N sum F(a_i).
The bound is a function of the case -- of the data, the grid point and the tile count -- not one number."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
EPS_EXP_DEVICE = 4e-16          # exp_rt's fp64 evaluation against its own formula: tests/test_gpu_rt_math.py
EPS_EXP_HOST = 2 * U            # glibc: 1 ulp
ARG_MIN = -708.0
MOMENT_ROWS, LEAVES_PER_TILE = 256, 8
SCOTT, SILVERMAN, FACTOR = 0, 1, 2
RULES = {"scott": SCOTT, "silverman": SILVERMAN}


def build_host(tmpdir):
    """tests/kde_core_host.cpp built with g++ and the address / undefined-behaviour sanitizers; returns
    run(mode, words) -> the output file's 64-bit words as uint64."""
    exe = os.path.join(str(tmpdir), "kde_core_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "kde_core_host.cpp"), "-o", exe])
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


def rule_of(bw):
    """'scott' | 'silverman' | a positive scalar -> (bw_rule, bw_factor) of the C ABI."""
    return (RULES[bw], 0.0) if isinstance(bw, str) else (FACTOR, float(bw))


def host_kde(run, x, cols, grid, bw, ok=None):
    """kde::density -> (pdf [nsel, ngrid], stat [nsel, 4], nonfinite [nsel])."""
    x, grid = np.ascontiguousarray(x, np.double), np.ascontiguousarray(grid, np.double)
    nsel, ngrid = grid.shape
    rule, factor = rule_of(bw)
    head = [x.shape[0], x.shape[1], nsel, ngrid, 0 if ok is None else 1, rule, factor]
    parts = [head, np.asarray(cols, float), grid.ravel()] + ([] if ok is None else [np.asarray(ok, float)]) + [x.ravel()]
    v = run("kde", np.concatenate(parts))
    n1 = nsel * ngrid
    return v[:n1].view(np.double).reshape(nsel, ngrid), v[n1:n1 + 4 * nsel].view(np.double).reshape(nsel, 4), v[n1 + 4 * nsel:]


def host_hpd(run, pdf, p):
    v = run("hpd", np.concatenate([[len(pdf), p], np.asarray(pdf, float)]))
    n = len(pdf)
    return v[:n].astype(bool), float(v[n:n + 1].view(np.double)[0]), float(v[n + 1:n + 2].view(np.double)[0]), int(v[n + 2])


# ---- the cases ----------------------------------------------------------------------------------------------------
def named_indices(grid_row, mean):
    """The grid indices at which mpmath values are computed: the first, the last, the 63 / 64 / 65 and 127 / 128 seams
    where they exist, the point nearest the mean and the farthest.  Named before any result is known."""
    n = len(grid_row)
    idx = {0, n - 1} | {i for i in (63, 64, 65, 127, 128) if i < n}
    if np.isfinite(mean):
        d = np.abs(np.asarray(grid_row) - mean)
        idx |= {int(np.argmin(d)), int(np.argmax(d))}
    return sorted(idx)


def _column(kind, n, rng):
    if kind == "normal":
        return 1.5 + 0.7 * rng.normal(size=n)
    if kind == "bimodal":
        return np.where(rng.random(n) < 0.5, 0.0, 3.0) + 0.3 * rng.normal(size=n)
    if kind == "radius":                     # 97 000 km that varies by a few km
        return 9.7e4 + 3.0 * rng.normal(size=n)
    if kind == "constant":
        return np.full(n, 2.5)
    raise ValueError(kind)


def _grid_for(col, ngrid, ok=None):
    v = col[np.isfinite(col) & (np.ones(len(col), bool) if ok is None else np.asarray(ok, bool))]
    if v.size == 0:
        return np.linspace(-1.0, 1.0, ngrid)
    s = np.std(v) if v.size > 1 and np.std(v) > 0 else 1.0
    return np.linspace(v.min() - s, v.max() + s, ngrid)


THREE_OF_SEVEN = (7, [5, 0, 3])              # 3 columns of 5 that hold data, out of order, ld = 7


def _matrix(kinds, nrows, ld, cols, seed):
    """x [nrows, ld], NaN where no selected column lies (a read outside the selection would show)."""
    rng = np.random.default_rng(seed)
    x = np.full((nrows, ld), np.nan)
    for kind, c in zip(kinds, cols):
        x[:, c] = _column(kind, nrows, rng)
    return x


def make_cases(T):
    """name -> dict(x, cols, grid, bw, ok): every shape and content both test files run.  T: the rule's tile."""
    cases = {}

    def add(name, kinds, nrows, ngrid, bw, sel=None, ok=None, seed=0, edit=None, grid=None):
        ld, cols = sel if sel else (1, [0])
        x = _matrix(kinds, nrows, ld, cols, seed)
        if edit:
            edit(x)
        g = np.stack([_grid_for(x[:, c], ngrid, ok) for c in cols]) if grid is None else grid(x)
        cases[name] = dict(x=x, cols=list(cols), grid=g, bw=bw, ok=ok)

    add("1 row x 1 point", ["normal"], 1, 1, "scott", seed=1)
    add("2 rows x 63 points", ["normal"], 2, 63, "silverman", seed=2)
    add("T-1 rows x 64 points, bimodal, factor 0.3", ["bimodal"], T - 1, 64, 0.3, seed=3)
    add("T rows x 1024 points", ["normal"], T, 1024, "scott", seed=4)
    add("T+1 rows x 65 points x out-of-order columns", ["normal", "radius", "bimodal"], T + 1, 65, "scott",
        sel=THREE_OF_SEVEN, seed=5)

    def specials(x):
        x[3::97, 5], x[5::89, 0], x[7::83, 3], x[11::101, 3] = np.inf, -np.inf, np.nan, np.inf
    add("2T+3 rows x 128 points, masked, inf and NaN in the data", ["bimodal", "normal", "radius"], 2 * T + 3, 128,
        "silverman", sel=THREE_OF_SEVEN, ok=np.random.default_rng(6).random(2 * T + 3) < 0.7, seed=6, edit=specials)
    whole = np.ones(2 * T + 3, bool)
    whole[T:2 * T] = False
    add("a mask that removes a whole tile", ["normal"], 2 * T + 3, 64, "scott", ok=whole, seed=7)
    one = np.zeros(T + 1, bool)
    one[T - 3] = True
    add("a mask that removes all but one row", ["normal", "radius", "bimodal"], T + 1, 63, "scott", sel=THREE_OF_SEVEN,
        ok=one, seed=8)

    def lonely(x):
        x[:, 0] = np.nan
        x[T // 2, 0] = 4.25
    add("a constant column and an n = 1 column beside a good one", ["constant", "normal", "normal"], T + 1, 65, "scott",
        sel=THREE_OF_SEVEN, seed=9, edit=lonely)

    def far(x):                              # the even points 60 .. 123 std away: every term is below kArgMin
        g = _grid_for(x[:, 0], 64)
        g[::2] = x[:, 0].mean() + np.std(x[:, 0]) * np.arange(60, 124, 2) * np.where(np.arange(32) % 2, -1.0, 1.0)
        return g[None]
    add("grid points so far out that every term is dropped", ["normal"], T + 1, 64, "scott", seed=10, grid=far)

    def scattered(x):
        rng = np.random.default_rng(11)
        return np.stack([rng.permutation(np.quantile(x[:, c], rng.random(128)) + 0.1 * rng.normal(size=128))
                         for c in THREE_OF_SEVEN[1]])
    add("a non-uniform, unsorted grid", ["bimodal", "normal", "radius"], 2 * T + 3, 128, 0.25, sel=THREE_OF_SEVEN,
        seed=11, grid=scattered)
    return cases


# ---- the restatement in mpmath ------------------------------------------------------------------------------------
def _exp_rt_piece(mp, k, a, n):
    """exp_rt's formula on the piece n at the exact argument a (rtmath_restate.exp_rt_restated, n given)."""
    import rtmath_restate as rr
    return mp.ldexp(rr.horner(mp, k["rt"], a - n * mp.mpf(k["ln2"])), n)


def exact_column(x, col, grid_row, indices, bw, ok, T, eps_exp, device=False):
    """The rule for column ``col`` of x at grid_row[indices], in mpmath: -> dict n, nonfinite, mean, std, h (floats
    of the exact values, NaN where the rule says so), pdf [len(indices)] (``device``: with exp_rt's formula for the
    exponential, else with exp), pdf_exp (with exp), and the bounds mean_bound, std_bound, h_bound, pdf_bound
    [len(indices)] derived in this module's docstring."""
    import mpmath as mp
    mp.mp.dps = 40
    if device:
        import rtmath_restate as rr
        kh = rr.read_kernels_hpp()
        log2e = mp.mpf(kh["log2e"])
    v = np.asarray(x[:, col], np.double)
    lets = np.ones(len(v), bool) if ok is None else np.asarray(ok, bool)
    counts = lets & np.isfinite(v)
    out = dict(n=int(counts.sum()), nonfinite=int((lets & ~np.isfinite(v)).sum()))
    nan = float("nan")
    n = out["n"]
    ref = mp.mpf(float(v[0])) if np.isfinite(v[0]) else mp.mpf(0)
    xs = [mp.mpf(float(t)) for t in v[counts]]
    ys = [t - ref for t in xs]
    ntiles = (len(v) + T - 1) // T
    K = LEAVES_PER_TILE + ntiles
    out.update(mean=nan, std=nan, h=nan, mean_bound=0.0, std_bound=0.0, h_bound=0.0,
               pdf=np.full(len(indices), nan), pdf_exp=np.full(len(indices), nan), pdf_bound=np.zeros(len(indices)))
    if n == 0:
        return out
    mean_y = mp.fsum(ys) / n
    A = float(max(abs(t) for t in ys))
    E = (MOMENT_ROWS + 1 + 7 * K) * U * A
    out["mean"] = float(ref + mean_y)
    out["mean_bound"] = E + U * abs(out["mean"])
    if n < 2:
        return out
    M2 = mp.fsum((t - mean_y) ** 2 for t in ys)
    std = mp.sqrt(M2 / (n - 1))
    out["std"] = float(std)
    if M2 == 0:
        return out
    Y2, sigma = float(mp.fsum(t * t for t in ys)), float(mp.sqrt(M2 / n))
    eps_m2 = U * (2 * np.sqrt(Y2 / float(M2)) + 4 * np.sqrt(2.0) * (MOMENT_ROWS + 1 + 7 * K) * A / sigma
                  + 3 + MOMENT_ROWS + 6 * K)
    eps_std = eps_m2 / 2 + 3 * U
    out["std_bound"] = eps_std * out["std"]
    rule, factor = rule_of(bw)
    if rule == FACTOR:
        f, eps_factor = mp.mpf(factor), 0.0
    else:
        q = mp.mpf(n) if rule == SCOTT else mp.mpf(3 * n) / 4
        f, eps_factor = q ** (mp.mpf(-1) / 5), 4.004 * U
    h = f * std
    eps_h = eps_std + eps_factor + U
    out["h"], out["h_bound"] = float(h), eps_h * float(h)
    rho, nu = 2 * eps_h + 7 * U, eps_h + 4 * U
    gamma = (T + ntiles) * U / (1 - (T + ntiles) * U)
    norm = 1 / (n * h * mp.sqrt(2 * mp.pi))
    for k, j in enumerate(indices):
        g = mp.mpf(float(grid_row[j]))
        args = [-((g - t) / h) ** 2 / 2 for t in xs]
        terms = [mp.exp(a) for a in args]
        out["pdf_exp"][k] = float(norm * mp.fsum(terms))
        jump = mp.mpf(0)
        if device:                           # F is exp_rt's formula wherever a term can be kept
            for i, a in enumerate(args):
                if a < ARG_MIN - 1:
                    continue
                lo, hi = (int(mp.nint(a * (1 + sgn * rho) * log2e)) for sgn in (1, -1))
                n = int(mp.nint(a * log2e))
                terms[i] = _exp_rt_piece(mp, kh, a, n)
                if lo != hi:
                    jump += abs(_exp_rt_piece(mp, kh, a, lo) - _exp_rt_piece(mp, kh, a, hi))
        out["pdf"][k] = float(norm * mp.fsum(terms))
        a, t = np.array([float(s) for s in args]), np.array([float(s) for s in terms])
        kept = a >= ARG_MIN + 1
        r = (1 + eps_exp) * np.exp(np.abs(a[kept]) * rho * (1 + 1e-10)) - 1
        err = np.sum(t[kept] * ((1 + r) * (1 + gamma) * (1 + nu) - 1)) + float(jump) + np.sum(t[~kept])
        out["pdf_bound"][k] = float(norm) * err * (1 + 1e-9)       # (the bound's own float arithmetic)
    return out


def assert_column(name, s, ref, pdf_row, stat_row, nonfinite, indices):
    """One column of a result against exact_column's, every figure printed before it is asserted."""
    n, mean, std, h = stat_row
    print("%s [%d]: n %d  mean err %.3g / %.3g  std err %.3g / %.3g  h err %.3g / %.3g" % (
        name, s, n, abs(mean - ref["mean"]), ref["mean_bound"], abs(std - ref["std"]), ref["std_bound"],
        abs(h - ref["h"]), ref["h_bound"]))
    assert n == ref["n"] and int(nonfinite) == ref["nonfinite"], (name, s)
    for got, key in ((mean, "mean"), (std, "std"), (h, "h")):
        if np.isnan(ref[key]):
            assert np.isnan(got), (name, s, key, got)
        else:
            assert abs(got - ref[key]) <= ref[key + "_bound"], (name, s, key, got, ref[key], ref[key + "_bound"])
    if np.isnan(ref["h"]) or ref["std"] == 0:
        assert np.isnan(h) and np.isnan(pdf_row).all(), (name, s)
        return
    assert np.all(np.isfinite(pdf_row)) and np.all(pdf_row >= 0.0), (name, s)
    err = np.abs(pdf_row[indices] - ref["pdf"])
    print("    pdf err / bound at %s: %s" % (indices, " ".join("%.2g/%.2g" % p for p in zip(err, ref["pdf_bound"]))))
    print("    the reference's distance from the one with exp: %s" % " ".join(
        "%.2g" % v for v in np.abs(ref["pdf"] - ref["pdf_exp"])))
    assert np.all(err <= ref["pdf_bound"]), (name, s, err, ref["pdf_bound"])


# ---- the region on Python floats ------------------------------------------------------------------------------------
def region_restate(pdf, p):
    """The credible region of a density on a grid (kde_core.hpp, REGION): -> (mask, threshold, included, nruns)."""
    pdf = [float(v) for v in pdf]
    n = len(pdf)
    mask = [False] * n
    if any(not (v >= 0.0) for v in pdf):
        return np.array(mask), 0.0, 0.0, 0
    order = sorted(range(n), key=lambda i: (-pdf[i], i))
    total = 0.0
    for i in order:
        total = total + pdf[i]
    if total == 0.0:
        return np.array(mask), 0.0, 0.0, 0
    c = thr = 0.0
    for i in order:
        mask[i] = True
        c = c + pdf[i]
        thr = pdf[i]
        if c >= p * total:
            break
    runs = sum(1 for i in range(n) if mask[i] and (i == 0 or not mask[i - 1]))
    return np.array(mask), thr, c, runs
