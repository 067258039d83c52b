"""CPU: the exact restatement of the contribution-function kernels (tests/cf_exact.py) against closed forms in exact
arithmetic and against oracle/rt_oracle.c's optical depth passed through tests/cf_restate.py, and the conditions that
make tests/test_gpu_cf_exact.py able to fail, on exactly its cases (tests/cf_cases.py): the derived bound is at most
1e-11 of the row's largest |value| on every checked row of every ordinary case (the thin and all-zero cases: the bound
printed and held in absolute terms), and every deliberate mistake (cf_exact.MUTANTS) leaves the bound by a factor of
ten on a named case.  The inputs here are the ORACLE's extinction, radii and temperatures taken exactly
(cf_exact.from_oracle, as eclipse_cases.oracle_columns does it): the device's own records need the device.  cf_setup's
weight arithmetic is not reachable on the host: the weights are held in the GPU file, through the read-back."""
import mpmath
import numpy as np
import pytest

import cf_cases as cc
import cf_exact as cx
import cf_restate
import transit_restate as tr

mp = mpmath.mpf
ORACLE_TOL = 1e-9           # tests/test_gpu_cf.py's TOL: what the suite holds the oracle path to, of the row's maximum
ROW_SHARE = 1e-11


def test_closed_forms_in_exact_arithmetic():
    """An isothermal grey column: tau_k = k e dr, tr_k = exp(-k e dr), cf_k = B (x^(k-1) - x^k) rdlp, x = exp(-e dr);
    a box response: the band value of a constant is the constant, of a ramp its midpoint."""
    with mpmath.workdps(tr.DPS):
        tol = mp(10) ** -40
        L, e0, dr, T, nu = 20, 2.0 ** -22, 2.0 ** 20, 1500.0, 2000.0
        for kend in (L - 1, 7):
            c = cx.Columns()
            c.e = np.empty((L, 1), object); c.e[:] = mp(e0)
            c.de, c.A = np.zeros((L, 1)), np.full((L, 1), e0)
            c.dr = np.concatenate([[0.0], np.full(L - 1, dr)])
            c.c1 = np.full(L, 1.4387769 / T * 1.0)
            c.nu, c.cols, c.L, c.kend, c.ch = np.array([nu]), [0], L, kend, None
            c.rdlp = np.concatenate([[0.0], 1.0 / np.arange(1, L)])
            for rule in (0, 1):
                tau, dtau = cx.depths(c, rule)
                assert all(abs(tau[k, 0] - k * mp(e0) * mp(dr)) <= tol for k in range(L))
                trv, _ = cx.values(c, tau, dtau, cx.KIND_TR)
                cfv, _ = cx.values(c, tau, dtau, cx.KIND_CF)
                x = mpmath.exp(-mp(e0) * mp(dr))
                B = 2 * mp(6.6260755e-27) * mp(nu) ** 3 * mp(2.99792458e10) ** 2 / (mpmath.exp(mp(float(c.c1[0])) * mp(nu)) - 1)
                for k in range(L):
                    kk = min(k, kend)
                    assert abs(trv[k, 0] - x ** kk) <= tol
                    want = B * (x ** (k - 1) - x ** k) * mp(float(c.rdlp[k])) if 0 < k <= kend else mp(0)
                    assert abs(cfv[k, 0] - want) <= tol * B, (k, kend)
        # the band: a box response over nine samples
        c = cx.Columns()
        c.cols = list(range(9))
        v = np.empty((2, 9), object)
        v[0], v[1] = [mp(3)] * 9, [mp(i) for i in range(9)]
        b, db, dred = cx.band(c, v, np.zeros((2, 9)), [(0, 9, np.ones(9))])
        assert abs(b[0, 0] - 3) <= tol and abs(b[0, 1] - 4) <= tol and np.all(db > 0) and np.all(dred <= db)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("cf_cases"))


def exact_of(c, o, prof, rule, kind, cache, mutant=None):
    """(full[L, ncols] from the top, dfull, band[nf, L], dband, dred) of one walker; the depths cached per rule 1 / not."""
    key = (c.dir, id(prof), o.c.has_cloud and o.c.cloudtop, rule == 1)
    if key not in cache:
        col = cx.from_oracle(o, prof, c.cols)
        cache[key] = (col,) + cx.depths(col, rule, transit=col.ch is not None)
    col, tau, dtau = cache[key]
    v, dv = cx.values(col, tau, dtau, kind, mutant=mutant)
    b, db, dred = cx.band(col, v, dv, cc.window_list(c.windows), mutant=mutant)
    return col, v, dv, b, db, dred


def oracle_rows(c, o, prof, kind):
    """The suite's oracle path on every grid sample, layers from the top: [L, W]."""
    _, tau, _ = o.run(prof, want_tau=True)
    L = len(c.press_bar)
    return cf_restate.contribution(prof[:L], c.press_bar, tau.T, o.wn) if kind == cc.CF else np.exp(-tau.T)


@pytest.mark.parametrize("group", list(cc.GROUPS))
def test_oracle_inside_the_bound_and_the_bound_small(root, group):
    """Walker 1 of every case under every rule, kind and deck the GPU tests run: the oracle path within the bound plus
    its own tolerance of the exact value on every checked row; the bound at most 1e-11 of the row's largest |value|
    (full output: per column over the layers; band: per filter over the layers) -- every row, none skipped.  On the
    thin and all-zero cases the bound is printed and held to an absolute figure: the transmittances' own 2 (7.5e-14 +
    4e-16) relative to B rdlp at the most."""
    from oracle import rt_oracle as orc
    worst, share, absolute = 0.0, 0.0, {}
    for c in cc.GROUPS[group](root):
        if getattr(c, "form", "x") is None:
            continue                                # (the refused depth: no result to hold)
        prof = np.asarray(c.profs[1], float)
        for deck in c.decks:
            cache = {}
            for rule in c.rules:
                o = orc.OracleEngine(cc.inf_cfg(c), integ=rule)
                if deck is not None:
                    o.set_cloudtop(deck)
                if c.tag == "thin":
                    assert o.run(prof, want_tau=True)[1].max() < cc.THIN_TAU
                if c.tag == "thick":
                    t = o.run(prof, want_tau=True)[1]
                    assert (t[c.checked][:, :-1].max(axis=1) > cc.CLAMP_TAU).all(), t[c.checked][:, -2]
                for kind in c.kinds:
                    col, v, dv, b, db, _ = exact_of(c, o, prof, rule, kind, cache)
                    ref = oracle_rows(c, o, prof, kind)
                    pos = [col.cols.index(i) for i in c.checked]
                    vf = np.abs(tr.to_float(v[:, pos]))
                    rowmax = vf.max(axis=0)
                    dev = cx.absdev(ref[:, c.checked], v[:, pos])
                    allow = dv[:, pos] + ORACLE_TOL * rowmax[None, :]
                    assert np.all(dev <= allow), (c.tag, deck, rule, kind, cx.ratio(dev, allow))
                    worst = max(worst, cx.ratio(dev, allow))
                    bmax = np.abs(tr.to_float(b)).max(axis=1)
                    if c.tag in cc.ABSOLUTE:
                        scale = 1.0 if kind == cc.TR else max(float(cx.er.planck(mp(float(col.c1[k])) * mp(float(nu)), float(nu))[0]) * col.rdlp[k]
                                                              for k in range(1, col.L) for nu in col.nu[pos])
                        absolute[c.tag, kind] = max(absolute.get((c.tag, kind), 0.0), float(dv[:, pos].max() / scale))
                        assert dv[:, pos].max() <= 2.2 * (7.5e-14 + 4e-16 + 1e-15) * scale, (c.tag, kind, dv[:, pos].max() / scale)
                        continue
                    # (a row that is exactly zero -- the contribution under a deck on the top layer -- has a zero bound)
                    r = max(cx.ratio(dv[:, pos].max(axis=0), rowmax), cx.ratio(db.max(axis=1), bmax))
                    share = max(share, r)
                    assert r <= ROW_SHARE, (c.tag, deck, rule, kind, r, (dv[:, pos].max(axis=0) / rowmax), db.max(axis=1) / bmax)
    print("%s: largest bound / row max %.2e (at most %.0e); oracle |dev| / (bound + %.0e row max) at most %.3f; "
          "absolute cases, bound / (B rdlp): %s" % (group, share, ROW_SHARE, ORACLE_TOL, worst, absolute))


def test_each_mutant_leaves_the_bound(root):
    """On the 33-layer case with a deck on row 16 (a partial last block, a frozen depth) and on the 48-layer case: each
    mistake moves a band row or a checked column of the full output by at least ten bounds.  The factor is printed per
    mutant; a mutant that no case tells apart is reported by the assertion."""
    from oracle import rt_oracle as orc
    deckc = cc.deck_cases(root)[0]
    picks = [(deckc, deckc.decks[1]), (deckc, None), ([c for c in cc.layer_cases(root) if c.tag == "L48"][0], None),
             ([c for c in cc.layer_cases(root) if c.tag == "L33"][0], None)]      # (a partial last block on an ordinary column)
    best = {m: (0.0, None) for m in cx.MUTANTS}
    finite = {m: 0.0 for m in cx.MUTANTS}       # ... over rows whose bound is above 1e-300 (not exactly-zero or clamp rows)
    for c, deck in picks:
        prof = np.asarray(c.profs[1], float)
        o = orc.OracleEngine(cc.inf_cfg(c), integ=1)
        if deck is not None:
            o.set_cloudtop(deck)
        cache = {}
        for kind in (cc.CF, cc.TR):
            col, v, dv, b, db, _ = exact_of(c, o, prof, 1, kind, cache)
            pos = [col.cols.index(i) for i in c.checked]
            for m in cx.MUTANTS:
                _, vm, _, bm, _, _ = exact_of(c, o, prof, 1, kind, cache, mutant=m)
                f = cx.ratio(cx.absdev(tr.to_float(cx.atm(vm, m)[:, pos]), cx.atm(v)[:, pos]), cx.atm(dv)[:, pos])
                g = cx.ratio(cx.absdev(tr.to_float(bm), b), db)
                # (the mutant's values are rounded to doubles first, as a device's would be: half an ulp against the bound)
                dfull, bfull = cx.absdev(tr.to_float(cx.atm(vm, m)[:, pos]), cx.atm(v)[:, pos]), cx.atm(dv)[:, pos]
                dband = cx.absdev(tr.to_float(bm), b)
                finite[m] = max(finite[m], cx.ratio(dfull[bfull > 1e-300], bfull[bfull > 1e-300]), cx.ratio(dband[db > 1e-300], db[db > 1e-300]))
                if max(f, g) > best[m][0]:
                    best[m] = (max(f, g), "%s deck %s kind %d" % (c.tag, deck, kind))
    for m in cx.MUTANTS:
        print("mutant %-18s leaves the bound by a factor of %.3g on %s; on rows with a bound above 1e-300: %.3g"
              % (m, best[m][0], best[m][1], finite[m]))
    # cf0_nonzero is the one mistake the arithmetic itself cannot show: tau_0 = 0 on every column, so B (1 - E_0) rdlp_1
    # IS 0 (a finding, stated in the commit message; the GPU tests hold row 0 of the contribution to exactly 0 all the same)
    blind = [m for m in cx.MUTANTS if best[m][0] < 10.0]
    assert blind == ["cf0_nonzero"], blind
