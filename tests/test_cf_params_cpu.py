"""CPU: the posterior contribution-function calls (include/bartrt.h, bartrt_cf_batch_over / bartrt_cf_params and
their _dev forms) are exported with the declared signatures and refuse to run without an engine; the host half of
bart_amd.cf.posterior (layout sniffing, burn-in and thinning, free-to-full expansion, the shared-parameter error,
the percentile envelopes) with the engine calls stubbed out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -3

SIGNATURES = {
    "bartrt_cf_batch_over": "const double *, int, int, const double *, int, double *, double *, unsigned char *",
    "bartrt_cf_batch_over_dev": "const double *, int, const double *, int, double *, double *, unsigned char *, void *",
    "bartrt_cf_params": "const double *, int, int, int, double *, double *, int *",
    "bartrt_cf_params_dev": "const double *, int, int, int, double *, double *, int *, void *",
}


@pytest.fixture(scope="module")
def lib():
    from bart_amd import build, transit_module as trm
    build.build()
    return trm.lib()


def test_the_four_symbols_have_the_declared_signatures(lib, tmp_path):
    """A strict C compiler accepts each entry point as a function pointer of the type the issue declares (a
    mismatch between the header and that type is an error), and the library exports it."""
    tu = tmp_path / "sig.c"
    lines = ['#include "bartrt.h"']
    lines += ["int (*p_%s)(%s) = %s;" % (n, args, n) for n, args in SIGNATURES.items()]
    lines.append("int main(void) { return p_bartrt_cf_params == 0; }")
    tu.write_text("\n".join(lines) + "\n")
    libdir = os.path.join(ROOT, "bart_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tu),
                           "-L" + libdir, "-lbartrt", "-Wl,-rpath," + libdir, "-o", str(tmp_path / "sig")])
    for n, args in SIGNATURES.items():
        fn = getattr(lib, n)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args.split(",")), n


def test_without_an_engine_the_calls_fail_and_do_not_crash(lib, tmp_path):
    from bart_amd import synth, transit_module as trm
    trm.free_memory()
    x, band = np.zeros((2, 8)), np.zeros((2, 4, 10))
    over, st, ok = np.full((2, 3), np.nan), np.zeros(2, np.int32), np.zeros(2, np.uint8)
    p = trm._ptr

    def every_call():
        return [lib.bartrt_cf_batch_over(p(x), 2, 8, p(over), 1, p(band), None, p(ok)),
                lib.bartrt_cf_batch_over_dev(p(x), 2, p(over), 1, p(band), None, None, None),
                lib.bartrt_cf_params(p(x), 2, 8, 1, p(band), None, p(st)),
                lib.bartrt_cf_params_dev(p(x), 2, 8, 1, p(band), None, p(st), None),
                lib.bartrt_cf_params(None, 0, 0, 7, None, None, None)]

    assert every_call() == [EINVAL] * 5 and b"not initialised" in lib.bartrt_last_error()
    import torch
    if not torch.cuda.is_available():
        # a valid configuration on a machine without a GPU: the init fails, the calls still answer
        case = synth.make_case(str(tmp_path), nwave=16, nlayers=10)
        assert lib.bartrt_init(3, (C.c_char_p * 3)(b"transit", b"-c", case.tcfg.encode())) == ENODEV
        assert set(every_call()) <= {EINVAL, ENODEV}
    with pytest.raises(trm.TransitError):
        from bart_amd import engine
        engine.transmittance_from_params(np.zeros((2, 8)), (np.zeros(1, np.int32), np.full(1, 2, np.int32), np.ones(2), np.ones(1)))


# ---- cf.posterior's host half ------------------------------------------------------------------------------
PARAMS = np.array([-2.0, 0.0, 1.0, 0.0, 0.98, -2.0, 1.0, -0.5])
STEP = np.array([0.01, 0.01, 0.0, 0.01, 0.01, 0.1, 0.0, 0.1])
FREE = np.nonzero(STEP)[0]


def mc3_output(nchains=3, niter=10, seed=1):
    return np.random.default_rng(seed).normal(size=(nchains, len(FREE), niter))


def test_samples_from_the_mc3_layout_burnin_and_thinning():
    from bart_amd import cf
    data = mc3_output()
    got = cf.posterior_samples(data, PARAMS, STEP, burnin=4)
    assert got.shape == (3 * 6, 8)
    # bestFit.py:436-438 and 449-456, literally
    stack = data[0, :, 4:]
    for c in (1, 2):
        stack = np.hstack((stack, data[c, :, 4:]))
    for k in range(stack.shape[1]):
        cur, j = PARAMS.copy(), 0
        for i in range(len(PARAMS)):
            if STEP[i] != 0.0:
                cur[i] = stack[j, k]
                j += 1
        assert np.array_equal(got[k], cur)
    thin = cf.posterior_samples(data, PARAMS, STEP, burnin=1, thinning=4)
    assert np.array_equal(thin[:, FREE], np.concatenate([data[c][:, 1::4].T for c in range(3)]))
    assert np.array_equal(thin[:, 2], np.full(9, PARAMS[2])) and thin.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError, match="no sample is left"):
        cf.posterior_samples(data, PARAMS, STEP, burnin=10)


def test_samples_from_the_retrieve_layout_and_sniffing():
    from bart_amd import cf
    own = np.random.default_rng(2).normal(size=(3, 10, 8))
    got = cf.posterior_samples(own, PARAMS, STEP, burnin=2, thinning=2)
    want = own[:, 2::2].reshape(-1, 8).copy()
    want[:, STEP == 0] = PARAMS[STEP == 0]
    assert np.array_equal(got, want)
    # both layouts of one posterior give the same samples
    mc3 = np.ascontiguousarray(own[:, :, FREE].transpose(0, 2, 1))
    assert np.array_equal(cf.posterior_samples(mc3, PARAMS, STEP, 2, 2), got)
    with pytest.raises(ValueError, match="neither"):
        cf.posterior_samples(np.zeros((3, 5, 9)), PARAMS, STEP, 0)
    with pytest.raises(ValueError, match="three-dimensional"):
        cf.posterior_samples(np.zeros((3, 8)), PARAMS, STEP, 0)
    both = np.random.default_rng(3).normal(size=(2, 6, 8))       # six free of eight, eight iterations
    with pytest.raises(ValueError, match="layout="):
        cf.posterior_samples(both, PARAMS, STEP, 0)
    assert cf.posterior_samples(both, PARAMS, STEP, 0, layout="mc3").shape == (16, 8)
    assert cf.posterior_samples(both, PARAMS, STEP, 0, layout="retrieve").shape == (12, 8)


def test_a_shared_parameter_raises_the_samplers_error():
    from bart_amd import cf, sampler
    step = STEP.copy()
    step[1] = -1.0
    with pytest.raises(ValueError) as a:
        cf.posterior_samples(mc3_output(), PARAMS, step, 0)
    with pytest.raises(ValueError) as b:
        sampler._check_stepsize(step)
    assert str(a.value) == str(b.value) and "shared" in str(a.value)


def test_posterior_with_the_engine_stubbed_out(tmp_path, monkeypatch):
    from bart_amd import cf
    cfg = tmp_path / "BART.cfg"
    cfg.write_text("[MCMC]\nparams = %s\nstepsize = %s\nsolution = transit\n"
                   % (" ".join(repr(float(x)) for x in PARAMS), " ".join(repr(float(x)) for x in STEP)))
    data = mc3_output(nchains=2, niter=30, seed=5)
    np.save(str(tmp_path / "output.npy"), data)
    seen = {}

    def stub(cfg_path, samples, filters, kind, chunk):
        seen.update(cfg=cfg_path, samples=samples.copy(), filters=filters, kind=kind, chunk=chunk)
        rng = np.random.default_rng(9)
        band = rng.random((len(samples), 2, 5))
        status = (np.arange(len(samples)) % 7 == 3).astype(np.int32)
        band[status != 0] = np.nan
        return band, status, kind or "transmittance"

    monkeypatch.setattr(cf, "_run_samples", stub)
    res = cf.posterior(str(tmp_path / "output.npy"), str(cfg), ["f.dat"], burnin=10, thinning=2, chunk=16)
    assert np.array_equal(seen["samples"], cf.posterior_samples(data, PARAMS, STEP, 10, 2))
    assert seen["chunk"] == 16 and seen["kind"] is None and seen["filters"] == ["f.dat"]
    assert res["kind"] == "transmittance" and res["band"].shape == (20, 2, 5)
    good = res["band"][res["status"] == 0]
    assert len(good) == 17 and np.all(np.isfinite(good))
    assert np.array_equal(res["median"], np.median(good, axis=0))
    for k, q in (("lo1", 15.87), ("hi1", 84.13), ("lo2", 2.28), ("hi2", 97.72)):
        assert np.array_equal(res[k], np.percentile(good, q, axis=0))
    assert np.all(res["lo2"] <= res["lo1"]) and np.all(res["lo1"] <= res["median"]) and np.all(res["hi1"] <= res["hi2"])
    # no accepted sample: NaN envelopes, not an exception
    monkeypatch.setattr(cf, "_run_samples", lambda c, s, f, k, ch: (np.full((len(s), 2, 5), np.nan),
                                                                    np.ones(len(s), np.int32), "contribution"))
    res = cf.posterior(data, str(cfg), None, burnin=0)
    assert res["median"].shape == (2, 5) and np.all(np.isnan(res["median"])) and np.all(np.isnan(res["hi2"]))
    cfg.write_text("[MCMC]\nparams = 1.0 2.0\n")
    with pytest.raises(ValueError, match="stepsize"):
        cf.posterior(data, str(cfg), None, burnin=0)
