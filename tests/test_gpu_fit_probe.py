"""GPU: the fit's kernel alone (bartrt_fit_probe: the solve phase of csrc/fit.hip's fit_advance, no engine) against
the numpy restatement tests/fit_restate.py on synthetic band rows, at the edges of its shapes: one wave per start,
lane q on column q of a 64 x 64 system in LDS.

Tolerance: the bound of fit_restate's docstring, 16 nfree 2^-52 cond2(Ms) |y| / sqrt(M_jj) + 2^-52 |x_j|, computed per
rung from the restatement's own Jacobi-scaled matrix; cases are built with cond2 <= 1e8 and that is asserted first.
The valid masks (which dampings factored) and Marquardt's scaling D must be equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_restate as fr  # noqa: E402

pytestmark = pytest.mark.gpu


def probe(P, x, lam, D, cur, pband, pstatus):
    from bart_amd import transit_module as trm
    from bart_amd.fit import FitOpts
    a = lambda v: np.ascontiguousarray(v, np.double)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    S = len(x)
    opts = FitOpts(size=C.sizeof(FitOpts), nrungs=P.K, fdstep=P.fdstep)
    keep = [a(v) for v in (P.prior, P.priorlow, P.priorup)] if P.prior is not None else None
    if keep:
        opts.prior, opts.priorlow, opts.priorup = (v.ctypes.data for v in keep)
    args = [a(v) for v in (P.pmin, P.pmax, P.stepsize, P.data, P.uncert, x, lam, D, cur, pband)]
    pst = np.ascontiguousarray(pstatus, np.intc)
    trial, valid = np.zeros((S, P.K, P.npars)), np.zeros(S, np.intc)
    trm.check(trm.lib().bartrt_fit_probe(S, P.npars, p(args[0]), p(args[1]), p(args[2]), P.ndata, p(args[3]), p(args[4]),
                                         C.cast(C.byref(opts), C.c_void_p), p(args[5]), p(args[6]), p(args[7]),
                                         p(args[8]), p(args[9]), p(pst), p(trial), p(valid)))
    return trial, valid, args[7]


def case(nfree, ndata, K, S, seed, priors=False, extra=3, reject=(), on_bound=False, shared=False):
    """A random well-conditioned problem: npars = nfree + extra (fixed ones, and one copy when `shared`), a linear
    model with an orthonormal-ish design so that cond2 stays small, random current band rows."""
    rng = np.random.default_rng(seed)
    npars = nfree + extra
    step = np.zeros(npars)
    free = np.sort(rng.choice(npars, nfree, replace=False))
    step[free] = rng.uniform(0.05, 0.2, nfree)
    if shared:
        fixed = [j for j in range(npars) if step[j] == 0]
        step[fixed[0]] = -(free[0] + 1.0)
    pmin, pmax = np.full(npars, -1.0), np.full(npars, 1.0)
    data = rng.normal(size=ndata)
    uncert = rng.uniform(0.5, 2.0, ndata)
    pri = {}
    if priors:
        prior, lo, up = np.zeros(npars), np.zeros(npars), np.zeros(npars)
        for j in free[::2]:
            prior[j], lo[j], up[j] = rng.uniform(-0.5, 0.5), rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
        up[free[0]] = 0.0                                       # a width on one side only
        pri = dict(prior=prior, priorlow=lo, priorup=up)
    P = fr.Problem(pmin, pmax, step, data, uncert, nrungs=K, **pri)
    # the design: independent columns scaled to the data; with fewer rows than columns the damping (and the priors)
    # must carry the system, so lambda is large there
    G = rng.normal(size=(ndata, npars)) / np.sqrt(ndata)
    x = rng.uniform(-0.5, 0.5, (S, npars))
    if on_bound:
        x[:, free[-1]] = 1.0                                    # h flips its sign there
        x[0, free[0]] = -1.0
    x = np.array([P.shared(r) for r in x])
    lam = np.full(S, 10.0 if ndata < nfree else 1e-2) * rng.uniform(0.5, 2.0, S)
    D = np.zeros((S, npars))
    D[:, free] = rng.uniform(0.0, 2.0, (S, nfree)) * (rng.random((S, nfree)) < 0.5)
    if ndata < nfree:
        D[:, free] += 1.0                                       # (rank-deficient A: every column needs its damping)
    model = lambda rows: rows @ G.T + 0.3 * np.sin(rows @ G.T)
    cur = model(x)
    pband = np.array([model(P.jacobian_rows(r)) for r in x])
    pstatus = np.zeros((S, nfree), np.intc)
    for s, q, st in reject:
        if s < S and q < nfree:
            pstatus[s, q] = st
            pband[s, q] = -1.0
    return P, x, lam, D, cur, pband, pstatus


def check(P, x, lam, D, cur, pband, pstatus, cond_max=1e8):
    trial, valid, Dout = probe(P, x, lam, D, cur, pband, pstatus)
    worst, nvalid = 0.0, 0
    for s in range(len(x)):
        sol = P.solve(x[s], lam[s], D[s], cur[s], pband[s], pstatus[s])
        assert int(valid[s]) == sol["valid"], (s, int(valid[s]), sol["valid"])
        assert np.array_equal(Dout[s], sol["D"]), (s, Dout[s], sol["D"])
        for k in range(P.K):
            if sol["valid"] >> k & 1:
                nvalid += 1
                assert sol["cond"][k] <= cond_max, (s, k, sol["cond"][k])
            err = np.abs(trial[s, k] - sol["trial"][k])
            assert np.all(err <= sol["tol"][k]), (s, k, err.max(), sol["tol"][k], sol["cond"][k])
            worst = max(worst, float(np.max(err / np.maximum(sol["tol"][k], 1e-300))))
    print("probe: %d valid rungs, largest error / bound %.3g" % (nvalid, worst))
    return trial, valid, nvalid


@pytest.mark.parametrize("nfree", [1, 2, 31, 32, 33, 63, 64])
def test_columns(nfree):
    _, _, nvalid = check(*case(nfree, 65, 4, 2, seed=nfree, extra=0 if nfree == 64 else 1))
    assert nvalid == 8


@pytest.mark.parametrize("ndata", [1, 3, 64, 65, 300])
def test_rows(ndata):
    _, _, nvalid = check(*case(5, ndata, 4, 2, seed=100 + ndata, priors=ndata == 3))
    assert nvalid == 8


@pytest.mark.parametrize("K", [1, 4, 8])
def test_rungs(K):
    _, _, nvalid = check(*case(6, 20, K, 2, seed=200 + K))
    assert nvalid == 2 * K


@pytest.mark.parametrize("S", [1, 2, 65])
def test_starts(S):
    _, _, nvalid = check(*case(7, 12, 4, S, seed=300 + S, priors=True, shared=True, on_bound=True,
                               reject=((0, 2, 1), (1, 0, 2), (64, 6, 3))))
    assert nvalid == 4 * S


@pytest.mark.parametrize("priors", [False, True])
def test_every_parameter_frozen_but_one(priors):
    P, x, lam, D, cur, pband, pstatus = case(6, 9, 4, 3, seed=400 + priors, priors=priors)
    pstatus[:, 1:] = 1                                          # every column but the first is rejected
    pband[:, 1:] = -1.0
    trial, valid, _ = check(P, x, lam, D, cur, pband, pstatus)
    moved = np.abs(trial - x[:, None, :]) > 0
    assert moved[:, :, P.free[0]].all() and not moved[:, :, P.free[1:]].any() and np.all(valid == 15)


def test_a_column_without_effect_or_damping_makes_every_rung_invalid():
    P, x, lam, D, cur, pband, pstatus = case(4, 10, 4, 2, seed=500)
    pband[1, 2] = cur[1]                                        # start 1: column 2 of J is zero, and its D
    D[1, P.free[2]] = 0.0
    trial, valid, _ = check(P, x, lam, D, cur, pband, pstatus)
    assert valid.tolist() == [15, 0] and np.array_equal(trial[1], np.tile(x[1], (4, 1)))


def test_refusals():
    from bart_amd import transit_module as trm
    P, x, lam, D, cur, pband, pstatus = case(3, 4, 4, 1, seed=600)
    P.K = 9
    with pytest.raises(trm.TransitError, match="nrungs"):
        probe(P, x, lam, D, cur, pband, pstatus)
    P.K = 4
    P.stepsize = np.array([0.1, -1.0, -2.0, 0.1, 0.1, 0.0])[:P.npars]
    with pytest.raises(trm.TransitError, match="shared"):
        probe(P, x, lam, D, cur, pband, pstatus)
