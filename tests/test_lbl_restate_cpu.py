"""CPU: the exact restatement of the line-by-line extinction (tests/lbl_restate.py) held to closed forms, to the numpy
oracle, and to a list of mutants of itself, on the cases of tests/lbl_cases.py (no GPU).

  closed forms   an isolated Doppler line is the Gaussian; an isolated Lorentz-dominated line is the Lorentzian to its
                 first correction; down-sampling a constant gives the constant
  oracle         oracle/lbl_oracle.py lies inside the bound plus its own stated accuracy (scipy's wofz 1e-13, numpy's
                 exp and the double arithmetic of its strengths 1e-14) on every decided point; prints the undecided
                 share (at most 2 %), the pairs (at most 15 000) and the bound relative to max e(nu) per case
  mutants        each deliberately wrong restatement leaves the bound on at least one decided point of a named case.
                 The last group, K scaled by 1 + 1e-10 on one branch at a time, is the point of the exercise: a relative
                 error of 1e-10 on any branch is caught."""
import numpy as np
import pytest

import lbl_cases as LC
import lbl_restate as X

ORACLE_EPS = 1e-13 + 1e-14
CPU_CASES = [n for n in LC.CASES]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("lbl_exact_cpu"))
    return lambda name: LC.get(name, root)


def test_isolated_lines_are_the_gaussian_and_the_lorentzian():
    mp, mpf = X.mp, X.mpf
    fad = X.Faddeeva()
    for x in (0.0, 0.5, 3.0, 7.0, 12.0):
        assert abs(fad(mpf(x), mpf(0))[0] / mp.exp(-mpf(x) ** 2) - 1) < mpf("1e-30")
    # y >> 1: K = y / (sqrt(pi) (x^2 + y^2)) (1 + (3 x^2 - y^2) / (2 (x^2 + y^2)^2) + O(|z|^-4))
    for x, y in ((0.0, 300.0), (500.0, 300.0), (3000.0, 1000.0)):
        x_, y_ = mpf(x), mpf(y)
        r2 = x_ * x_ + y_ * y_
        lor = y_ / (mp.sqrt(mp.pi) * r2)
        K = fad(x_, y_)[0]
        assert abs(K / (lor * (1 + (3 * x_ * x_ - y_ * y_) / (2 * r2 * r2))) - 1) < 10 / r2 ** 2
        assert abs(K / lor - 1) < 2 / r2
    # the derivatives that carry the arguments' roundings: against a difference quotient
    K, Kx, Ky = fad(mpf(2.5), mpf(0.3))
    h = mpf("1e-12")
    assert abs((fad(mpf(2.5) + h, mpf(0.3))[0] - K) / h / Kx - 1) < 1e-10
    assert abs((fad(mpf(2.5), mpf(0.3) + h)[0] - K) / h / Ky - 1) < 1e-10


def test_downsampling_a_constant_gives_the_constant(case):
    cs = case("osamp")
    rs = X.Restatement(cs.su)
    for dv in (2, 3, 4, 12):
        ka, pts = rs.fine_points(dv)
        n = len(pts)
        val, bnd, _, _ = rs.reduce(ka, dv, [X.mpf(7)] * n, [0.0] * n, [0.0] * n, [0.0] * n)
        assert len(val) == cs.W and all(v == 7 for v in val)
        assert max(bnd) <= (dv + 2) * X.U * 7


def test_tiny_real_parts_keep_their_digits():
    """w's real part far below its modulus (small y, large x): the working precision follows it."""
    fad = X.Faddeeva()
    for x, y in ((16.9, 1e-300), (20.0, 1e-50), (100.0, 1e-12), (12.0, 1e-30)):
        K = fad(X.mpf(x), X.mpf(y))[0]
        lead = X.mp.exp(-X.mpf(x) ** 2) + X.mpf(y) / (X.mp.sqrt(X.mp.pi) * X.mpf(x) ** 2)
        assert abs(K / lead - 1) < 2 / x ** 2, (x, y, K, lead)


@pytest.mark.parametrize("name", CPU_CASES)
def test_oracle_inside_the_bound(case, name):
    cs = case(name)
    cs.sharp()
    res = cs.restated()
    pairs = sum(r.pairs for r in res.values())
    und = np.concatenate([r.undecided for r in res.values()])
    v = np.concatenate([r.v for r in res.values()])
    b = np.concatenate([r.bound for r in res.values()])
    print("%s: %d pairs, %.2f %% of the points undecided, bound / max e = %.3g, largest bound / value %.3g, branches %s"
          % (name, pairs, 100 * und.mean(), b.max() / v.max(), (b[v > 0] / v[v > 0]).max(),
             {k: sum(r.by_branch.get(k, 0) for r in res.values()) for k in X.BRANCHES}))
    assert pairs <= LC.MAX_PAIRS
    assert und.mean() <= LC.MAX_UNDECIDED
    if cs.per_gram:
        tab = cs.o.opacity_table([1000.0])
        ref = np.concatenate([tab[l, 0, g] for (l, g) in res])
    else:
        ext = cs.o.extinction(cs.prof)
        ref = np.concatenate([ext[l] for l in res])
        dvs = [cs.o.layer_dv(*s) for s in cs.states()]
        assert dvs == [s["dv"] for s in cs.restated_states()]
        if name == "osamp":
            assert any(d > 1 and d % 2 for d in dvs) and any(d > 1 and d % 2 == 0 for d in dvs)
    lo = np.concatenate([r.lo for r in res.values()])
    hi = np.concatenate([r.hi for r in res.values()])
    slack = ORACLE_EPS * v
    assert np.all((ref >= lo - slack) & (ref <= hi + slack))
    assert np.array_equal(ref[~und] == 0, v[~und] == 0)


def test_all_five_owners_and_the_edges_occur(case):
    owners = set()
    for name in LC.CASES:
        cs = case(name)
        if cs.claims:
            owners |= set(int(o) for o in np.unique(cs.owners))
    assert owners == {0, 1, 2, 3, 4}
    rs = case("doppler").restated_states()
    assert len(case("doppler").su.dbs[1]["temps"]) == 1
    # the strongest H2O line of `doppler` reaches no point, yet it sets the threshold
    cs = case("doppler")
    X_ = X.Restatement(cs.su)
    lines, smax = X_.kept(rs[0])
    S = X_.strengths(rs[0], 0)
    j = int(np.argmax([float(s) for s, _ in S]))
    assert cs.su.dbs[0]["wn"][j] > cs.su.wn[-1] + 20.0 and S[j][0] == smax[0]
    # a line under kExpMin: its strength is positive and far below every threshold
    j = int(np.argmax(cs.su.dbs[0]["elow"]))
    assert 0 < S[j][0] < X.mpf("1e-290") * smax[0]
    assert all(float(st["lor"][0]) == 0.0 for st in case("y0").restated_states())


# mutant -> the case it has to leave the bound on
MUTANT_CASE = dict(no_stim="doppler", no_ln2="doppler", z_nearest="mixed", thresh_all="doppler", ends_full="osamp",
                   odd_for_even="osamp", nearest_linear="grid", kc_floor="grid", reach_short="grid", y_lowend="mixed",
                   k_taylor="doppler", k_weideman="mixed", k_asym11="doppler", k_asym6="pressure", k_far="pressure")


@pytest.mark.parametrize("mutant", X.MUTANTS)
def test_mutant_leaves_the_bound(case, mutant):
    cs = case(MUTANT_CASE[mutant])
    good = cs.restated()
    bad = cs.restated(mutant=mutant)
    out = 0
    for key, r in good.items():
        m = ~r.undecided
        out += int(np.sum(np.abs(bad[key].v - r.v)[m] > r.bound[m]))
    print("%s on %s: %d decided points outside the bound" % (mutant, cs.name, out))
    assert out >= 1
