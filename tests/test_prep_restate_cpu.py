"""CPU: the mpmath restatement of the layer preparation (tests/prep_restate.py) held to the C oracle
(oracle/rt_oracle.c: orc_radpress, bracket, orc_extinction) on every case of tests/test_gpu_prep_edges.py.  The two
share no code and no arithmetic (50 digits against plain doubles; makeatm's g-chain in both, written independently):
their agreement is the evidence that the GPU test's reference is right.

Bounds, from counting the oracle's roundings (worst case, every rounding the same way; the measured figures,
printed with -s, are a random walk far inside them):
  radii ........ the reference layer: 2 ulp (its increment is below 1e-2 r).  Each step away from it rounds the new
                 radius (half an ulp of r) and adds an increment d_i = |r_i - r_i-1| of ten roundings of its own plus
                 three more per step already taken (the gravity chain g r^2 / r^2): layer n steps away is bounded by
                 2 + sum_{i <= n} (1/2 + (5 + 1.5 i) d_i / r_i) ulp of r, the d_i and r_i the restated ones;
  extinction ... a term is at most eight roundings and up to 3 + 2 M + 4 C = 27 terms are added, a rounding each:
                 35 roundings of half an EPS, doubled for the compounding as in the GPU test: 40 EPS (EPS = 2^-52) of
                 the SUM OF THE TERMS' MAGNITUDES (where the table extrapolates, 1 - f and f have opposite signs and
                 the sum itself may be much smaller than its terms)."""
import mpmath
import numpy as np
import pytest

import prep_cases as pc
import prep_restate as pr


def _oracle(case, **kw):
    from oracle import rt_oracle as orc
    return orc.OracleEngine(case.tcfg, **kw)


EPS = 2.0 ** -52


def _radius_bound(r):
    ref, ix = pr.mag(r["radius"]), r["ref_idx"]
    step = np.abs(np.diff(ref)) / ref[1:]                 # d / r of the step between layers l and l + 1
    out = np.full(len(ref), 2.0)
    for l in range(ix + 1, len(ref)):
        out[l] = out[l - 1] + 0.5 + (5.0 + 1.5 * (l - ix)) * step[l - 1]
    for l in range(ix - 1, -1, -1):
        out[l] = out[l + 1] + 0.5 + (5.0 + 1.5 * (ix - l)) * step[l]
    return out * pr.ulp(ref)


def restated_extinction(su, o, r):
    """-> (ext[L][W], the sum of the terms' magnitudes [L][W]) at 50 digits, from the dense weights and the oracle's
    own reading of the tables (o.kappa [L][Nt][M][W], o.cia_alpha / o.cia_y2 [planes][W])."""
    mp = mpmath.mpf
    L, W = len(su.press), len(o.wn)
    ext, mags = np.empty((L, W), object), np.empty((L, W), object)
    with mpmath.workdps(pr.DPS):
        wn4 = [mp(float(w)) ** 4 for w in o.wn]
        for l in range(L):
            terms = [[r["grey"][l]] for _ in range(W)]
            tw = r["table_weight"][l]
            for j in range(tw.shape[0]):
                for m in range(len(su.opmol)):
                    if tw[j, m] != 0:
                        for i in range(W):
                            terms[i].append(tw[j, m] * mp(float(o.kappa[l, j, m, i])))
            off, nfile = 0, -1
            for cc, (s1, s2, temps, kind) in enumerate(su.cia):
                if kind == 0:
                    nfile += 1
                    base = off
                    off += len(temps)
                planes = o.cia_alpha if kind == 0 else o.cia_y2
                for j in range(len(temps)):
                    wgt = r["cia_weight"][cc][l, j]
                    if wgt != 0:
                        for i in range(W):
                            terms[i].append(wgt * mp(float(planes[base + j, i])))
            for i in range(W):
                terms[i].append(r["rayleigh"][l] * wn4[i])
                ext[l, i] = sum(terms[i])
                mags[l, i] = sum(abs(t) for t in terms[i])
    return ext, mags


def _hold(su, o, prof, label, **own):
    """own: a walker's own overrides, as prep_restate.restate takes them (the oracle has been set to the same)."""
    ext_o, rad_o = o.extinction(prof)
    r = pr.restate(su, prof, **own)
    dr = pr.absdev(rad_o, r["radius"])
    bound = _radius_bound(r)
    ext, mags = restated_extinction(su, o, r)
    de = pr.absdev(ext_o, ext)
    print("%s: oracle radii off the restatement by %.3g ulp at the most, %.2f of the bound; extinction by %.3g EPS of "
          "its terms' magnitudes" % (label, (dr / pr.ulp(rad_o)).max(), (dr / bound).max(), (de / pr.mag(mags)).max() / EPS))
    assert np.all(dr <= bound), (label, dr / pr.ulp(rad_o))
    # (the grey ramp is evaluated on radii that differ by dr: its slope times dr, where there is a ramp)
    slack = su.cloud_ext * (dr + pr.ulp(rad_o)) / (su.cloud_rup - su.cloud_rdown) if su.cloud_ext > 0.0 else np.zeros(len(dr))
    assert np.all(de <= 40 * EPS * pr.mag(mags) + slack[:, None]), (label, (de / pr.mag(mags)).max() / EPS)
    return r, rad_o, ext_o


@pytest.mark.parametrize("label,L,k,variant", pc.REF_CASES, ids=[c[0] for c in pc.REF_CASES])
def test_reference_layer_cases(tmp_path, label, L, k, variant):
    c = pc.ref_case(tmp_path, L, k, variant)
    o = _oracle(c)
    su = pr.setup_from_oracle(o)
    ix, exact = pr.reference_layer(su)
    if variant in ("on", "off"):
        assert ix == k and exact == (variant == "on")
    else:
        assert ix == (0 if variant == "below" else L - 1) and not exact
    for n, prof in enumerate(pc.profiles(c, 3, seed=L + (k or 0))):
        r, rad_o, _ = _hold(su, o, prof, "%s profile %d" % (label, n))
        if exact:
            assert rad_o[ix] == su.refradius and r["radius"][ix] == su.refradius
        else:
            assert rad_o[ix] != su.refradius


def test_temperature_edges(tmp_path):
    """Both cia_interp readings; the extrapolating profiles' extinction is positive at every sample (with the
    overshoot pc.ramp_overshoot settles on: 150 K unless the synthetic table turns negative there)."""
    for interp in ("linear", "spline"):
        c = pc.temp_edge_case(tmp_path / interp, extra_keys={"cia_interp": interp})
        o = _oracle(c)
        su = pr.setup_from_oracle(o)
        assert len(su.cia) == (2 if interp == "linear" else 4)
        over = pc.ramp_overshoot(c, o)
        print("cia_interp %s: ramp overshoot %g K" % (interp, over))
        profs = pc.temp_edge_profiles(c, over)
        assert profs["ramp"][0] == 400.0 - over and profs["ramp"][23] == 3000.0 + over
        for name, prof in profs.items():
            r, _, ext_o = _hold(su, o, prof, "%s %s" % (interp, name))
            assert np.all(ext_o > 0.0), name
            if name in ("on-nodes", "first-node", "last-node"):
                # on a node the whole weight sits on that node's plane
                tw = pr.mag(r["table_weight"])
                assert np.all((tw > 0).sum(axis=1) == 1)


@pytest.mark.parametrize("which,interp,solution", pc.SINGLE_CASES, ids=["-".join(c) for c in pc.SINGLE_CASES])
def test_single_temperature_cross_sections(tmp_path, which, interp, solution):
    """The oracle's nt == 1 branch against the dense weights; the file moves the spectrum by more than 1e-4."""
    c = pc.single_temp_case(tmp_path / "a", which, interp, solution)
    o = _oracle(c)
    su = pr.setup_from_oracle(o)
    profs = pc.profiles(c, 3, seed=5)
    for n, prof in enumerate(profs):
        _hold(su, o, prof, "single %s %s %s profile %d" % (which, interp, solution, n))
    bare = _oracle(pc.single_temp_case(tmp_path / "b", which, interp, solution, with_file=False))
    for prof in profs:
        assert np.max(np.abs(o.run(prof) / bare.run(prof) - 1.0)) > 1e-4


def test_small_terms_and_stop_layer(tmp_path):
    """Rayleigh under both flags with H2 or He absent, the grey ramp with a layer exactly on either end of it, kstop
    with the cloud top on a layer's pressure, just below it, above the top and below the bottom."""
    for species, abund in ((("He", "H2", "CO", "CO2", "CH4", "H2O"), (0.15, 0.85, 1e-4, 1e-4, 1e-4, 1e-4)),
                           (("H2", "CO", "CH4", "H2O"), (0.9997, 1e-4, 1e-4, 1e-4)),
                           (("He", "CO", "CH4", "H2O"), (0.9997, 1e-4, 1e-4, 1e-4))):
        c = pc.ref_case(tmp_path / "-".join(species[:2]), 24, 9, "off", species=species, abund=abund)
        o = _oracle(c)
        prof = pc.profiles(c, 2, seed=7)[1]
        for flag in (1, 2):
            o.set_scattering(flag, -1.5)
            su = pr.setup_from_oracle(o)
            r, _, _ = _hold(su, o, prof, "%s flag %d" % (species[:2], flag))
            lit = (flag == 1 and "H2" in species) or flag == 2
            assert np.all(pr.mag(r["rayleigh"]) > 0) == lit
        if "H2" in species and "He" in species:
            # a walker's own scattering values (the GPU test's fused step launch), the engine's setting left at -1.5
            o.set_scattering(1, -1.5)
            su = pr.setup_from_oracle(o)
            for v in pc.OWN_SCATTERING:
                o.set_scattering(1, v)
                r, _, _ = _hold(su, o, pc.iso_profile(c, 1234.5), "own scattering value %g" % v, scat_value=v)
                assert np.all(pr.mag(r["rayleigh"]) > 0)
    c = pc.ref_case(tmp_path / "grey", 24, 9, "off")
    o = _oracle(c)
    su = pr.setup_from_oracle(o)
    prof = pc.profiles(c, 2, seed=8)[1]
    rad = [float(x) for x in pr.restate(su, prof)["radius"]]
    rad_o = o.extinction(prof)[1]
    # a layer's radius on either end of the ramp, from the ORACLE's doubles here (what its own comparison sees)
    o.c.cloud_rup, o.c.cloud_rdown, o.c.cloud_ext = rad_o[15], rad_o[6], 3e-9
    su = pr.setup_from_oracle(o)
    r, _, _ = _hold(su, o, prof, "grey ramp")
    g = pr.mag(r["grey"])
    assert abs(rad[15] - rad_o[15]) <= 64 * np.spacing(rad[15])
    assert np.all(g[:6] == 3e-9) and np.all(g[16:] == 0.0) and np.all((g[7:15] > 0) & (g[7:15] < 3e-9))
    for ctop, want in ((su.press[10], (23 - 10) | pr.DECK_BIT), (np.nextafter(su.press[10], 0.0), (23 - 10) | pr.DECK_BIT),
                       (np.nextafter(su.press[10], np.inf), (23 - 9) | pr.DECK_BIT),
                       (0.5 * su.press[-1], 0 | pr.DECK_BIT), (2.0 * su.press[0], 23)):
        assert pr.restate(su, prof, cloudtop=ctop)["kstop"] == want, (ctop, want)


def test_ok_rule():
    su = pr.Setup(press=np.array([3.0, 2.0, 1.0]), mass=np.array([2.0, 4.0]), refpress=2.0, refradius=1.0, gsurf=1.0,
                  tgrid=np.array([1.0, 2.0]), opmol=[])
    good = np.array([[500.0, 600.0, 700.0], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]])
    assert pr.is_ok(su, good)
    for T, want in ((0.0, False), (-1.0, False), (np.inf, False), (1e30, False), (9.9e29, True), (np.nan, False)):
        p = good.copy()
        p[0, 1] = T
        assert pr.is_ok(su, p) == want, T
    p = good.copy()
    p[2, 2] = np.nan
    assert not pr.is_ok(su, p)
    p = good.copy()
    p[1:, 0] = 0.0
    assert not pr.is_ok(su, p)


def test_cloud_tops_through_the_cfg(tmp_path):
    """The GPU test's four cloud tops, written as logarithms: the restated stop layer is the expected one, and it is
    the oracle's: with the deck on layer k every column of the oracle ends where it ends without a cloud, or on k,
    whichever comes first -- and some column is cut short by it."""
    c0 = pc.ref_case(tmp_path / "bare", 24, 9, "off")
    o0 = _oracle(c0)
    l, v_below, cases = pc.stop_layer_cases(o0.press)
    prof = pc.profiles(c0, 2, seed=9)[1]
    free = o0.run(prof, want_tau=True)[2]
    for name, x, want in cases:
        c = pc.ref_case(tmp_path / name.replace(" ", "-"), 24, 9, "off", extra_keys={"cloudtop": repr(x)})
        o = _oracle(c)
        su = pr.setup_from_oracle(o)
        if name == "on the layer":
            assert su.cloudtop == o0.press[l]
        if name == "just below it":
            assert o0.press[l + 1] < su.cloudtop == v_below < o0.press[l]
        r, _, _ = _hold(su, o, prof, "cloud top " + name)
        assert r["kstop"] == want
        last = o.run(prof, want_tau=True)[2]
        kend = want & ~pc.DECK_BIT
        assert np.array_equal(last, np.minimum(free, kend))
        assert (want & pc.DECK_BIT == 0) or np.any(free > kend) or kend == 23
