"""What the reference's OWN readers return on the product's output files in cli_outputs/:
code/readtransit.py `readspectrum` on spec.dat and intens.dat, code/cf.py `readTauDat` on
tau.dat.  The modules are IMPORTED from a reference checkout (read-only; nothing is copied)
and their results stored in cli_outputs/reference_readers.npz, which
tests/test_cli.py::test_reference_readers_on_product_files holds the files to.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reader_golden.py <reference checkout>

numpy >= 1.24 removed np.float (cf.py:89 uses it), so it is aliased before the import;
matplotlib (imported by both modules for their plots) is stubbed where it is not installed.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "cli_outputs")


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
    import cf
    import readtransit
    nlayers = int(np.load(os.path.join(G, "expected.npz"))["nlayers"])
    wn, spec = readtransit.readspectrum(os.path.join(G, "spec.dat"), wn=True)
    tau, wns = cf.readTauDat(os.path.join(G, "tau.dat"), nlayers)
    iwn, inten = readtransit.readspectrum(os.path.join(G, "intens.dat"), wn=True)
    np.savez(os.path.join(G, "reference_readers.npz"), spec_wn=np.asarray(wn, float), spectrum=np.asarray(spec, float),
             tau=np.asarray(tau, float), tau_wn=np.asarray(wns, float), intens_wn=np.asarray(iwn, float),
             intens=np.asarray(inten, float))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
