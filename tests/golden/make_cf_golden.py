"""What the reference's OWN contribution-function code (code/cf.py) computes on a small synthetic
case: Planck, cf_eq, filter_cf (with and without normalize), transmittance(plot=False) and
cf(plot=False).  The module is IMPORTED from a reference checkout (read-only; nothing is copied);
its results and the inputs -- a seeded tau / p / T set on a 1 cm-1 grid, and the filter files
in cf_filters/ (written here) -- go into cf_golden.npz, which tests/test_cf_host.py holds
bart_amd.cf and the tests' restatement (tests/cf_restate.py) to.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cf_golden.py <reference checkout>

The filters: fcf1 and fcf2 overlap, fcf3 runs past the grid's upper edge, fcf4 lies inside one
64-sample tile.  numpy >= 1.24 removed np.float (cf.py:89 uses it), so it is aliased before the
import; matplotlib is stubbed where it is not installed.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FILT = os.path.join(HERE, "cf_filters")

# (wavenumber range cm-1, response shape) of the four filters
FILTERS = {"fcf1": (1020.0, 1085.0, "hat"), "fcf2": (1060.0, 1150.5, "ramp"),
           "fcf3": (1190.0, 1300.0, "hat"), "fcf4": (1130.3, 1150.7, "ramp")}


def write_filters():
    from bart_amd import synth
    os.makedirs(FILT, exist_ok=True)
    paths = []
    for name, (lo, hi, shape) in FILTERS.items():
        wl = np.linspace(1e4 / hi, 1e4 / lo, 41)           # microns, ascending (wavenumber descending)
        x = np.linspace(0.0, 1.0, wl.size)
        resp = np.sin(np.pi * x) ** 2 if shape == "hat" else 0.2 + 0.8 * x
        p = os.path.join(FILT, name + ".dat")
        synth.write_filter(p, wl, resp)
        paths.append(p)
    return paths


def case(nlayers=24, nwave=240, seed=20261016):
    """tau [L][W] from the top (non-decreasing in depth, below layer 17 it repeats as under a cloud
    deck), p [bar] and T [K] in atm order (bottom first), the grid wns [cm-1]."""
    rng = np.random.default_rng(seed)
    wns = 1000.0 + np.arange(nwave, dtype=float)
    p = np.logspace(2, -5, nlayers)
    t = 900.0 + 600.0 * (np.log10(p) + 5.0) / 7.0 + rng.normal(0, 20, nlayers)
    ext = np.exp(rng.normal(0, 1.5, (nlayers, nwave))) * np.logspace(-3, 1, nlayers)[:, None]
    tau = np.cumsum(ext, axis=0)
    tau[0] = 0.0
    tau[17:] = tau[17]
    return wns, p, t, tau


def main(ref):
    np.float = float  # noqa
    np.int = int      # noqa
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        mpl = types.ModuleType("matplotlib")
        mpl.use = lambda *a, **k: None
        for sub in ("pyplot", "gridspec"):
            m = types.ModuleType("matplotlib." + sub)
            setattr(mpl, sub, m)
            sys.modules["matplotlib." + sub] = m
        sys.modules["matplotlib"] = mpl
    sys.dont_write_bytecode = True       # nothing is written into the (read-only) reference tree
    sys.path.insert(0, os.path.join(ref, "code"))
    sys.path.insert(0, ROOT)
    import cf
    from bart_amd import synth
    filters = write_filters()
    wns, p, t, tau = case()
    L = len(p)
    with tempfile.TemporaryDirectory() as d:
        # the reference's two drivers read the atm file and tau.dat from date_dir; every array below is
        # computed from what they read back (the atm file rounds p and T)
        synth.write_atm(os.path.join(d, "case.atm"), ["H2", "He"], p, t, np.tile([0.85, 0.15], (L, 1)),
                        np.linspace(7.0e4, 7.2e4, L))
        with open(os.path.join(d, "tau.dat"), "w") as f:
            f.write("# optical depth per wavenumber; layers from the top of the atmosphere\n")
            for i, w in enumerate(wns):
                f.write("wavenumber[cm-1]: %.12g\n" % w)
                f.write(" ".join("%.17e" % v for v in tau[:, i]) + " \n")
                f.write("last: %d\n" % (L - 1))
        _, p_atm, t_atm, _ = cf.mat.readatm(os.path.join(d, "case.atm"))
        tau_rd, wns_rd = cf.readTauDat(os.path.join(d, "tau.dat"), L)
        assert np.array_equal(tau_rd, tau) and np.array_equal(wns_rd, wns)
        tr_out = cf.transmittance(d + "/", "case.atm", filters, plot=False)
        cf_out, cf_norm_out = cf.cf(d + "/", "case.atm", filters, plot=False)
    p_atm, t_atm = np.asarray(p_atm, float), np.asarray(t_atm, float)
    ptd, ttd = p_atm[::-1], t_atm[::-1]   # cf.cf's order: top to bottom
    bb = cf.Planck(ttd, wns)
    cfa = cf.cf_eq(bb, ptd, tau, L, wns)
    filt_cf = cf.filter_cf(filters, L, wns, cfa, normalize=False)
    filt_cf_n, filt_cf_norm = cf.filter_cf(filters, L, wns, cfa, normalize=True)
    transmit = np.exp(-tau)
    filt_tr = cf.filter_cf(filters, L, wns, transmit)
    np.savez_compressed(os.path.join(HERE, "cf_golden.npz"),
                        wns=wns, p_bar=p_atm, temp=t_atm, tau=tau,
                        filters=np.array([os.path.basename(x) for x in filters]),
                        planck=bb, cf=cfa, filt_cf=filt_cf, filt_cf_n=filt_cf_n, filt_cf_norm=filt_cf_norm,
                        transmit=transmit, filt_tr=filt_tr,
                        transmittance=np.asarray(tr_out, float), cf_cf=np.asarray(cf_out, float),
                        cf_cf_norm=np.asarray(cf_norm_out, float))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
