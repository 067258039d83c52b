"""CPU: the exact restatement of the transit column (tests/transit_restate.py) against closed forms in exact
arithmetic and against oracle/rt_oracle.c, and the conditions that make tests/test_gpu_transit_matrix.py able to fail,
on exactly its cases (tests/transit_cases.py): every mutation of the column moves M by more than 100 bounds
(sensitivity), no chord at or above a cut lies within 1000 bounds of `toomuch` (decidability), and the `toomuch` sweep
puts the cut on every row position and row tile (coverage)."""
import mpmath
import numpy as np
import pytest

import transit_cases as tc
import transit_restate as tr

mp = mpmath.mpf


def _uniform(L, e0, toomuch=1e30, transparent=False, kend=None, rstar=8e10):
    r = np.linspace(7.5e9, 7.0e9, L)
    ch = tr.Chords(r)
    with mpmath.workdps(tr.DPS):
        e = np.empty((L, 1), object)
        e[:] = mp(e0)
    z = np.zeros((L, 1))
    return r, ch, tr.columns(e, z, z, ch, L - 1 if kend is None else kend, toomuch, transparent, rstar)


def test_closed_forms_in_exact_arithmetic():
    with mpmath.workdps(tr.DPS):
        tol = mp(10) ** -40
        # a uniform shell: tau(b) = 2 e sqrt(r_top^2 - b^2)
        r, ch, col = _uniform(23, 3e-9)
        for k in range(23):
            want = 2 * mp(3e-9) * mpmath.sqrt(mp(r[0]) ** 2 - mp(r[k]) ** 2)
            assert abs(col.tau[k, 0] - want) <= tol * max(want, 1), k
        # no absorber: M = (r_bottom / R*)^2; with `transparent` 0 exactly
        r, ch, col = _uniform(23, 0.0)
        assert abs(col.M[0] - (mp(r[-1]) / mp(8e10)) ** 2) < tol and col.last[0] == 22
        r, ch, col = _uniform(23, 0.0, transparent=True)
        assert col.M[0] == 0
        # kend = 0: M = (r_top / R*)^2; 0 under `transparent`
        r, ch, col = _uniform(23, 3e-9, kend=0)
        assert abs(col.M[0] - (mp(r[0]) / mp(8e10)) ** 2) < tol and col.last[0] == 0
        r, ch, col = _uniform(23, 3e-9, kend=0, transparent=True)
        assert col.M[0] == 0
        # an opaque first chord
        r, ch, col = _uniform(23, 1.0, toomuch=10.0)
        assert col.last[0] == 1
        g1 = mpmath.exp(-col.tau[1, 0]) * mp(r[1])
        want = (mp(r[0]) ** 2 - (mp(r[0]) + g1) * (mp(r[0]) - mp(r[1]))) / mp(8e10) ** 2
        assert abs(col.M[0] - want) < tol


def test_chord_table_bound_is_the_cancellation():
    """The entry's bound in ulps of the entry grows with the distance from the diagonal, as s_{j-1} + s_j over
    s_{j-1} - s_j does; on the diagonal (no second root) it is under five ulps' halves."""
    ch = tr.Chords(np.linspace(7.5e9, 7.49e9, 40))
    d, b = ch.dense()
    ratio = b[39, 1:] / (tr.U * d[39, 1:])
    assert ratio[-1] < 5 and np.all(np.diff(ratio) < 0) and ratio[0] > 100


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("transit_cases"))
    out = {"sweep": [tc.sweep_case(root)], "zero": tc.zero_cases(root), "short": tc.short_cases(root),
           "off": tc.off_list_cases(root)}
    for L in tc.DEPTHS:
        out["L%d" % L] = tc.matrix_cases(root, L)
    return out


GROUPS = ["L37", "L150", "L260", "off", "sweep", "zero", "short"]


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_agreement_sensitivity_and_decidability(cases, group):
    worst, blind = {"tau": 0.0, "M": 0.0}, []
    for c in cases[group]:
        if group in ("L150", "L260") and not tc.exact_here(c):
            continue
        seen, chords = set(), None
        for v in c.variants:
            col, o, chords = tc.oracle_column(c, v, chords=chords)
            what = "%s %s" % (c.dir, v)
            # ---- the oracle, within the fp64 bound of its own evaluation
            spec, tau, last = o.run(c.profs[1], want_tau=True)
            assert np.array_equal(last[c.checked], col.last), what
            worst["M"] = max(worst["M"], (tr.absdev(spec[c.checked], col.M) / col.dM).max())
            for n, i in enumerate(c.checked):
                k = int(col.last[n]) + 1
                dev = tr.absdev(tau[i, :k], col.tau[:k, n])
                assert dev[0] == 0.0 and np.all(dev[1:] <= col.dtau[1:k, n]), (what, i)
                nz = dev[1:] > 0
                worst["tau"] = max(worst["tau"], (dev[1:][nz] / col.dtau[1:k, n][nz]).max() if nz.any() else 0.0)
            # ---- decidability
            assert tr.undecided(col) == [], what
            # ---- sensitivity: each mutation shows on some checked column of the case, under the wider of the two
            # kernels' bounds (the matrix-tile kernel's, with exp_rt's interpolant)
            col = tr.with_exp_rt(col)
            for n in range(len(c.checked)):
                for name, m in tr.mutants(col, n).items():
                    if abs(float(m - col.M[n])) > 100 * col.dM[n]:
                        seen.add(name[0])
        want = {"a", "b"} if len(c.press_bar) > 2 else {"b"}       # (two layers: one chord, the cut has one place)
        if any(v[2] for v in c.variants):
            want.add("d")
        if len(c.press_bar) > 17:
            want.add("c")
        if getattr(c, "tag", "") == "all":
            want = {"a", "d"}              # no extinction at all: only the cut's place and the core show
        if not want <= seen:
            blind.append((c.dir, sorted(want - seen)))
    assert not blind, blind         # a case that cannot show a mutation is a bad case: change its inputs
    print("%s: worst oracle |tau - exact| / bound %.3f, |M - exact| / bound %.3f" % (group, worst["tau"], worst["M"]))
    assert worst["tau"] <= 1.0 and worst["M"] <= 1.0


def sweep_coverage(c, lasts):
    """lasts: {variant index: last[W]}.  Every value of last % 16 and every row tile of the case; one aligned
    16-wavenumber group with three distinct cuts inside one row tile."""
    L = len(c.press_bar)
    allk = np.concatenate([l[l >= 1] for l in lasts.values()])
    assert set(allk % 16) == set(range(16)), sorted(set(allk % 16))
    assert set(allk // 16) == set(range((L + 15) // 16)), sorted(set(allk // 16))
    best = 0
    for l in lasts.values():
        for g in range(0, len(l) - 15, 16):
            grp = l[g:g + 16]
            for t in set(grp // 16):
                best = max(best, len(set(grp[grp // 16 == t])))
    assert best >= 3, best
    return best


def test_cut_sweep_covers_every_row_and_tile(cases):
    c = cases["sweep"][0]
    lasts = {}
    for n, v in enumerate(c.variants):
        o = tc.oracle_inputs(c, v)[0]
        lasts[n] = np.array(o.run(c.profs[1], want_tau=True)[2])
    print("most distinct cuts of one 16-wavenumber group in one row tile: %d" % sweep_coverage(c, lasts))
