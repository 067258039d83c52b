"""CPU: the optimiser's arithmetic (bart_amd/csrc/fit_core.hpp) through a stand-alone host program
(tests/fit_core_host.cpp, its own main, built here with g++ and the address / undefined-behaviour sanitizers) that
drives the very pick_start / solve_start functions the device kernel runs, over analytic models.  Every iteration of
the program's trace is replayed by tests/fit_restate.py (numpy.linalg.solve, no copy of the Cholesky) from the
program's own previous state; optima are held against scipy.optimize.least_squares."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_restate as fr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fit_core") / "fit_core_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "fit_core_host.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        return r.stdout
    run.exe = exe
    return run


# ---- the program's models, with its order of operations
class Linear:
    mid = 0

    def __init__(self, A):
        self.A = np.array(A, float)
        self.aux = self.A.ravel().tolist()

    def f(self, p):
        out = []
        for row in self.A.tolist():
            v = 0.0
            for a, x in zip(row, p):
                v += a * x
            out.append(v)
        return out


class Decay:
    mid = 1

    def __init__(self, t):
        self.aux = [float(v) for v in t]

    def f(self, p):
        return [p[0] * math.exp(-p[1] * t) + p[2] for t in self.aux]


class Rosenbrock:
    mid, aux = 2, []

    def f(self, p):
        return [10.0 * (p[1] - p[0] * p[0]), 1.0 - p[0]]


def batched(model, nd, reject=(-1, 0.0)):
    """reject = (parameter, threshold) or (parameter, second parameter, threshold): the program's rule."""
    par, par2, above = reject if len(reject) == 3 else (reject[0], -1, reject[1])

    def call(rows):
        band, status = [], []
        for p in np.asarray(rows, float).tolist():
            bad = par >= 0 and p[par] + (p[par2] if par2 >= 0 else 0.0) > above
            status.append(1 if bad else 0)
            band.append([-1.0] * nd if bad else model.f(p))
        return np.array(band), np.array(status)
    return call


def run_case(prog, tmp_path, P, model, starts, reject=(-1, 0.0)):
    starts = np.atleast_2d(np.array(starts, float))
    S, np_, nd, K = len(starts), P.npars, P.ndata, P.K
    reject = reject if len(reject) == 3 else (reject[0], -1, reject[1])
    z = [0.0] * np_
    pri = [P.prior, P.priorlow, P.priorup] if P.prior is not None else [z, z, z]
    rows = [[S, np_, nd, model.mid, P.maxiter, K, P.fdstep, P.ftol, P.xtol, P.lambda0, int(P.prior is not None),
             reject[0], reject[1], reject[2]], P.pmin, P.pmax, P.stepsize, *pri, P.data, P.uncert, starts.ravel(), model.aux]
    with open(tmp_path / "p.txt", "w") as f:
        for r in rows:
            f.write(" ".join(repr(float(v)) if isinstance(v, (float, np.floating)) else str(v) for v in r) + "\n")
    prog("run", tmp_path / "p.txt", tmp_path / "o.bin")
    v = np.fromfile(tmp_path / "o.bin")
    assert v[-1] == 1.0
    made = int(v[0])
    per_it = S * K * np_ + S + S * np_
    sizes = [1, S * (P.maxiter + 1) * (np_ + 4), made * per_it, S * np_, S, S, S, S * 4, 1]
    assert v.size == sum(sizes)
    parts = np.split(v, np.cumsum(sizes)[:-1])
    its = parts[2].reshape(made, per_it)
    return dict(made=made, trace=parts[1].reshape(S, P.maxiter + 1, np_ + 4),
                trial=its[:, :S * K * np_].reshape(made, S, K, np_),
                valid=its[:, S * K * np_:S * K * np_ + S].astype(int), D=its[:, S * K * np_ + S:].reshape(made, S, np_),
                best=parts[3].reshape(S, np_), chisq=parts[4], status=parts[5].astype(int), niter=parts[6].astype(int),
                nbad=parts[7].reshape(S, 4).astype(int), starts=starts)


def replay(P, call, res):
    """Every iteration of every start rebuilt from the program's own previous state.  Returns per-start lists of the
    frozen sets met, for the caller's own assertions."""
    S, np_ = len(res["starts"]), P.npars
    tr = res["trace"]
    frozen_seen = [[] for _ in range(S)]
    worst = 0.0
    for s in range(S):
        band, status = call([P.shared(res["starts"][s])])
        st = P.pick0(res["starts"][s], band[0], status[0])
        nbad = [0, 0, 0, 0]
        if 1 <= int(status[0]) <= 3:
            nbad[int(status[0])] += 1
        assert np.array_equal(tr[s, 0, :np_], st["x"]) and tr[s, 0, np_ + 3] == st["status"]
        assert tr[s, 0, np_] == st["chisq"] and tr[s, 0, np_ + 1] == P.lambda0 and tr[s, 0, np_ + 2] == -1
        it = 0
        while st["status"] == fr.RUNNING:
            it += 1
            assert it <= res["made"]
            D = np.zeros(np_) if it == 1 else res["D"][it - 2, s]
            pband, pstatus = call(P.jacobian_rows(st["x"]))
            sol = P.solve(st["x"], st["lam"], D, st["cur"], pband, pstatus)
            assert sol["valid"] == res["valid"][it - 1, s], (s, it, sol["valid"], res["valid"][it - 1, s])
            assert np.array_equal(sol["D"], res["D"][it - 1, s]), (s, it)
            for k in range(P.K):
                if sol["valid"] >> k & 1:
                    assert sol["cond"][k] <= 1e8, (s, it, k, sol["cond"][k])
                err = np.abs(res["trial"][it - 1, s, k] - sol["trial"][k])
                assert np.all(err <= sol["tol"][k]), (s, it, k, err, sol["tol"][k])
                worst = max(worst, float(np.max(err / np.maximum(sol["tol"][k], 1e-300))))
            frozen_seen[s].append(list(sol["frozen"]))
            trial = res["trial"][it - 1, s]
            tband, tstatus = call(trial)
            st, nb, _ = P.pick(st, it, trial, res["valid"][it - 1, s], tband, tstatus)
            nbad = [a + b + c for a, b, c in zip(nbad, sol["nbad"], nb)]
            rec = tr[s, it]
            assert rec[np_ + 2] == st["rung"] and rec[np_ + 3] == st["status"], (s, it, rec[np_ + 2:], st)
            assert np.array_equal(rec[:np_], st["x"]) and rec[np_] == st["chisq"], (s, it)
            assert abs(rec[np_ + 1] - st["lam"]) <= 4 * fr.EPS * st["lam"], (s, it)
            st["lam"] = rec[np_ + 1]
        assert it == res["niter"][s] and st["status"] == res["status"][s], (s, it, res["niter"][s], res["status"][s])
        assert nbad == res["nbad"][s].tolist(), (s, nbad, res["nbad"][s])
        for later in range(it + 1, P.maxiter + 1):        # a finished start does not change
            assert np.array_equal(tr[s, later, :np_ + 2], tr[s, it, :np_ + 2]) and tr[s, later, np_ + 3] == st["status"]
    print("replay: largest trial-point error / its bound %.3g" % worst)
    return frozen_seen


X5 = np.linspace(0.0, 1.0, 7)
A3 = np.stack([np.ones(7), X5, X5 ** 2], axis=1)


def linear_problem(**kw):
    truth = np.array([1.0, -2.0, 0.5])
    data = A3 @ truth + 0.01 * np.array([1, -1, 2, 0, -2, 1, -1.0])
    args = dict(pmin=[-10.0] * 3, pmax=[10.0] * 3, stepsize=[0.1, 0.1, 0.1], data=data, uncert=np.full(7, 0.01))
    args.update(kw)
    return fr.Problem(**args)


def test_linear_first_accepted_step_is_the_normal_equations_solution(prog, tmp_path):
    P = linear_problem(lambda0=1e-12)
    res = run_case(prog, tmp_path, P, Linear(A3), [[0.0, 0.0, 0.0], [3.0, 1.0, -1.0]])
    replay(P, batched(Linear(A3), 7), res)
    want = np.linalg.lstsq(A3 / 0.01, P.data / 0.01, rcond=None)[0]
    for s in range(2):
        assert res["trace"][s, 1, 3 + 2] >= 0                        # the first step is accepted
        np.testing.assert_allclose(res["trace"][s, 1, :3], want, rtol=0, atol=1e-8)
        assert res["status"][s] == fr.CONVERGED


def scipy_fit(model, P, start):
    from scipy.optimize import least_squares
    free = P.free

    def res(v):
        p = np.array(start, float)
        p[free] = v
        return P.residuals(model.f(P.shared(p).tolist()), P.shared(p))
    r = least_squares(res, np.array(start, float)[free], method="trf", bounds=(P.pmin[free], P.pmax[free]),
                      xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return r.x, 2.0 * r.cost, r


def decay_problem(**kw):
    t = np.linspace(0.0, 4.0, 12)
    noise = 1e-3 * np.array([1, -2, 0.5, 1.5, -1, 0, 2, -0.5, -1.5, 1, 0.5, -1.0])
    data = 2.0 * np.exp(-1.3 * t) + 0.5 + noise
    args = dict(pmin=[0.0, 0.0, 0.0], pmax=[10.0, 5.0, 2.0], stepsize=[1e-3] * 3, data=data, uncert=np.full(12, 1e-2),
                fdstep=1e-3, maxiter=200)
    args.update(kw)
    return fr.Problem(**args), Decay(t)


@pytest.mark.parametrize("case", ["decay", "rosenbrock", "rosenbrock_on_bound"])
def test_optimum_agrees_with_scipy_trf(prog, tmp_path, case):
    if case == "decay":
        (P, model), start = decay_problem(), [1.0, 0.5, 0.2]
    else:
        # the bounded case cuts the valley: the optimum lies on p0 = 0.8
        pmax = [0.8, 3.0] if case == "rosenbrock_on_bound" else [3.0, 3.0]
        P = fr.Problem(pmin=[-2.0, -2.0], pmax=pmax, stepsize=[1e-3, 1e-3], data=[0.0, 0.0], uncert=[1.0, 1.0],
                       fdstep=1e-3, maxiter=300)
        model, start = Rosenbrock(), [-1.2, 1.0]
    sx, schisq, r = scipy_fit(model, P, start)          # scipy first, alone
    assert r.status > 0, r.message
    res = run_case(prog, tmp_path, P, model, [start])
    replay(P, batched(model, P.ndata), res)
    c0 = res["trace"][0, 0, P.npars]
    print("%s: %d iterations, chisq %.6g (scipy %.6g), x %r (scipy %r)" % (
        case, res["niter"][0], res["chisq"][0], schisq, res["best"][0].tolist(), sx.tolist()))
    # (on the bound the one remaining parameter sees a quadratic: the first full step lands on its minimum, nothing
    # after it lowers chisq, and the start ends stalled there -- the optimum is the same)
    assert res["status"][0] in ((fr.CONVERGED, fr.STALLED) if case == "rosenbrock_on_bound" else (fr.CONVERGED,))
    assert np.all(np.abs(res["best"][0] - sx) <= 1e-6 * (P.pmax - P.pmin))
    assert res["chisq"][0] <= schisq + 1e-9 * c0
    if case == "rosenbrock_on_bound":
        assert res["best"][0][0] == 0.8


def test_one_free_parameter(prog, tmp_path):
    P = linear_problem(stepsize=[0.0, 0.1, 0.0])
    res = run_case(prog, tmp_path, P, Linear(A3), [[1.0, 0.0, 0.5]])
    replay(P, batched(Linear(A3), 7), res)
    assert res["status"][0] == fr.CONVERGED and abs(res["best"][0][1] + 2.0) < 0.05
    assert res["best"][0][0] == 1.0 and res["best"][0][2] == 0.5


def test_parameter_on_a_bound_with_outward_gradient_stays_frozen(prog, tmp_path):
    # the unconstrained optimum has p1 = -2 or so; the box stops at -1 and the start sits on it
    P = linear_problem(pmin=[-10.0, -1.0, -10.0])
    res = run_case(prog, tmp_path, P, Linear(A3), [[1.0, -1.0, 0.5]])
    frozen = replay(P, batched(Linear(A3), 7), res)[0]
    assert frozen and all(f == [False, True, False] for f in frozen)
    assert res["status"][0] == fr.CONVERGED and np.all(res["trace"][0, :, 1] == -1.0)
    sub = np.linalg.lstsq(A3[:, [0, 2]] / 0.01, (P.data + A3[:, 1]) / 0.01, rcond=None)[0]
    np.testing.assert_allclose(res["best"][0][[0, 2]], sub, atol=1e-7)


def test_shared_parameter_follows_its_source(prog, tmp_path):
    P = linear_problem(stepsize=[0.1, 0.1, -1.0])
    res = run_case(prog, tmp_path, P, Linear(A3), [[0.3, 0.0, 9.0]])
    replay(P, batched(Linear(A3), 7), res)
    assert np.array_equal(res["trace"][0, :, 2], res["trace"][0, :, 0]) and np.ptp(res["trace"][0, :, 0]) > 0
    assert np.array_equal(res["trial"][:, 0, :, 2], res["trial"][:, 0, :, 0])
    assert res["status"][0] == fr.CONVERGED


def test_prior_with_a_width_on_one_side_only(prog, tmp_path):
    # the data want p0 near 1; a prior at 0.5 that only holds from above pulls it down, one that only holds from
    # below does not act
    up = linear_problem(prior=[0.5, 0, 0], priorlow=[0.0, 0, 0], priorup=[0.002, 0, 0])
    low = linear_problem(prior=[0.5, 0, 0], priorlow=[0.002, 0, 0], priorup=[0.0, 0, 0])
    plain = linear_problem()
    out = {}
    for name, P in (("up", up), ("low", low), ("plain", plain)):
        res = run_case(prog, tmp_path, P, Linear(A3), [[0.9, -1.5, 0.0]])
        replay(P, batched(Linear(A3), 7), res)
        assert res["status"][0] == fr.CONVERGED
        out[name] = res
    assert 0.5 < out["up"]["best"][0][0] < out["plain"]["best"][0][0] - 0.05
    assert out["up"]["chisq"][0] > out["plain"]["chisq"][0]
    np.testing.assert_allclose(out["low"]["best"][0], out["plain"]["best"][0], atol=1e-7)


def test_rejected_perturbed_row_freezes_its_parameter_for_that_iteration(prog, tmp_path):
    # the model rejects p1 > 0.0005: from p1 = 0 the forward-difference row of p1 (h = 0.001) is rejected, the others'
    # are not.  The freeze is decided anew in every iteration and carries no memory: the second start, whose p1 is
    # below the threshold by more than h, never meets it; the first keeps its p1 (a frozen parameter does not move, so
    # its next perturbed row is the same rejected one) while its other parameters converge
    P = linear_problem()
    res = run_case(prog, tmp_path, P, Linear(A3), [[0.0, 0.0, 0.0], [0.0, -0.5, 0.0]], reject=(1, 0.0005))
    frozen = replay(P, batched(Linear(A3), 7, (1, 0.0005)), res)
    assert all(f == [False, True, False] for f in frozen[0]) and all(f == [False, False, False] for f in frozen[1])
    assert np.all(res["trace"][0, :, 1] == 0.0) and res["trace"][0, 1, 0] != 0.0
    assert res["nbad"].tolist() == [[0, res["niter"][0], 0, 0], [0, 0, 0, 0]]
    assert res["status"].tolist() == [fr.CONVERGED, fr.CONVERGED] and abs(res["best"][1][1] + 2.0) < 0.1


def test_a_row_rejected_once_freezes_its_parameter_once(prog, tmp_path):
    # the model rejects p0 + p1 > 3.0005.  From (3, 0, 0) the forward-difference row of p1 (h = 0.001) crosses that
    # line, the one of p0 (h = 0.0001) does not: p1 is frozen in iteration 1 while p0 moves down towards 1.  From
    # there p1's row is accepted, and p1 is free from iteration 2 on
    P = linear_problem(stepsize=[0.01, 0.1, 0.1])
    reject = (0, 1, 3.0005)
    res = run_case(prog, tmp_path, P, Linear(A3), [[3.0, 0.0, 0.0]], reject=reject)
    frozen = replay(P, batched(Linear(A3), 7, reject), res)[0]
    assert frozen[0] == [False, True, False] and all(f == [False, False, False] for f in frozen[1:]) and len(frozen) > 2
    tr = res["trace"][0]
    assert tr[1, 1] == 0.0 and tr[1, 0] < 2.9 and tr[2, 1] != 0.0
    assert res["nbad"][0].tolist() == [0, 1, 0, 0] and res["status"][0] == fr.CONVERGED
    assert abs(res["best"][0][1] + 2.0) < 0.1


def test_start_on_a_rejected_model_does_not_disturb_the_others(prog, tmp_path):
    P = linear_problem()
    starts = [[0.0, 0.0, 0.0], [0.0, 5.0, 0.0], [3.0, 1.0, -1.0]]
    res = run_case(prog, tmp_path, P, Linear(A3), starts, reject=(1, 4.0))
    replay(P, batched(Linear(A3), 7, (1, 4.0)), res)
    assert res["status"].tolist() == [fr.CONVERGED, fr.NO_START, fr.CONVERGED]
    assert np.isinf(res["chisq"][1]) and res["niter"][1] == 0 and res["nbad"][1].tolist() == [0, 1, 0, 0]
    assert np.array_equal(res["best"][1], starts[1])
    for s, start in ((0, starts[0]), (2, starts[2])):
        alone = run_case(prog, tmp_path, P, Linear(A3), [start], reject=(1, 4.0))
        assert np.array_equal(alone["best"][0], res["best"][s]) and alone["chisq"][0] == res["chisq"][s]
        n = alone["niter"][0]
        assert np.array_equal(alone["trace"][0, :n + 1], res["trace"][s, :n + 1])


def test_all_rungs_invalid_ends_stalled(prog, tmp_path):
    # the third parameter has no effect on the model: its column of A is zero, so is its D, and every rung's pivot
    A = A3.copy()
    A[:, 2] = 0.0
    P = linear_problem()
    res = run_case(prog, tmp_path, P, Linear(A), [[0.0, 0.0, 0.0]])
    replay(P, batched(Linear(A), 7), res)
    assert res["status"][0] == fr.STALLED and np.all(res["valid"][:, 0] == 0)
    assert np.array_equal(res["best"][0], [0.0, 0.0, 0.0]) and res["niter"][0] == 4      # 1e-3 (1e4)^4 > 1e12


def test_iteration_limit(prog, tmp_path):
    P = fr.Problem(pmin=[-2.0, -2.0], pmax=[3.0, 3.0], stepsize=[1e-3, 1e-3], data=[0.0, 0.0], uncert=[1.0, 1.0],
                   fdstep=1e-3, maxiter=3)
    res = run_case(prog, tmp_path, P, Rosenbrock(), [[-1.2, 1.0]])
    replay(P, batched(Rosenbrock(), 2), res)
    assert res["status"][0] == fr.ITER_LIMIT and res["niter"][0] == 3 and res["made"] == 3


def test_stepsize_validation_is_check_stepsize(prog, tmp_path):
    assert prog("check", 3, 0.1, -1, 0.0).strip() == "0"
    assert prog("check", 3, 0.1, -3, -1).strip() == "2"          # shared with a shared one
    assert prog("check", 3, 0.1, 0.2, -4).strip() == "3"         # k > npars
    assert prog("check", 2, 0.1, -1.5).strip() == "2"            # not an integer
    # and the loop refuses what it refuses (exit status 3), and a problem without a free parameter
    for step in ([0.1, -3.0, -1.0], [0.1, 0.2, -4.0], [0.0, 0.0, 0.0]):
        P = linear_problem(stepsize=step)
        with open(tmp_path / "bad.txt", "w") as f:
            z = "0 0 0"
            f.write("1 3 7 0 5 4 0.01 1e-10 1e-10 0.001 0 -1 -1 0\n-1 -1 -1\n1 1 1\n%s\n%s\n%s\n%s\n%s\n%s\n0 0 0\n%s\n" % (
                " ".join(map(str, step)), z, z, z, " ".join(map(repr, P.data.tolist())), "1 1 1 1 1 1 1",
                " ".join(map(repr, A3.ravel().tolist()))))
        r = subprocess.run([prog.exe, "run", str(tmp_path / "bad.txt"), str(tmp_path / "bad.bin")], capture_output=True)
        assert r.returncode == 3, (step, r.returncode, r.stderr[-2000:])
