"""GPU: posterior T(p) envelopes (include/bartrt.h, bartrt_posterior_tp; bart_amd/posterior.py), the device envelopes
of cf.posterior and `retrieve --tp-envelopes`.  Order statistics are held to np.sort bit for bit; interpolated values
to np.percentile within 2 ulp of the larger neighbouring order statistic (tests/quant_restate.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quant_restate as qr  # noqa: E402
from test_gpu_cf_params import draw_rows, worker_case  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Q = list(qr.PERCENTS)


def _assert_envelope(env, order, ranks, good_rows):
    """env [nq, ncols] against np.percentile of good_rows [n, ncols]; order / ranks the statistics behind it."""
    s = np.sort(good_rows, axis=0)
    assert qr.same_bits(order, s[ranks])
    for i, q in enumerate(Q):
        want = np.percentile(good_rows, q, axis=0)
        err = np.abs(env[i] - want) / np.spacing(np.maximum(np.abs(order[2 * i]), np.abs(order[2 * i + 1])))
        print("percent %5.2f: worst error %.2f ulp of the larger neighbour" % (q, float(err.max())))
        assert qr.within_two_ulp(env[i], want, order[2 * i], order[2 * i + 1])


@pytest.fixture(scope="module")
def W(tmp_path_factory):
    from bart_amd import BARTfunc
    case, cfg, wcfg, pmin, pmax = worker_case(str(tmp_path_factory.mktemp("ptp")), "eclipse")
    d = dict(case=case, cfg=cfg, wcfg=wcfg, pmin=pmin, pmax=pmax, worker=BARTfunc.Worker(wcfg, carry=False))
    yield d
    d["worker"].close()          # (two tests below rebuild it)


def _rows(W, n=300, seed=3):
    rows = draw_rows(W["pmin"], W["pmax"], n=n, seed=seed)
    rows[::17, 4] = 3.5          # beta far above the box: temperatures beyond Tmax, status 1
    return rows


def test_against_the_converter(W):
    import torch
    from bart_amd import engine
    rows = _rows(W)
    L = engine.nlayers()
    prof, st = engine.step_profiles_dev(torch.from_numpy(rows).cuda())
    torch.cuda.synchronize()
    T, st = prof.cpu().numpy()[:, :L], st.cpu().numpy()
    assert (st == 1).any() and (st == 0).sum() > 100
    env, status, ngood, ranks, order = engine.posterior_tp(rows, Q, want_order=True)
    assert np.array_equal(status, st) and ngood == int((st == 0).sum())
    assert env.shape == (len(Q), L) and order.shape == (2 * len(Q), L)
    for i, q in enumerate(Q):
        assert tuple(ranks[2 * i:2 * i + 2]) == engine.percentile_rule(ngood, q)[:2]
    _assert_envelope(env, order, ranks, T[st == 0])
    # the carry-over setting has no effect
    engine.step_set_carry(True)
    try:
        env2, status2, _ = engine.posterior_tp(rows, Q)
    finally:
        engine.step_set_carry(False)
    assert env2.tobytes() == env.tobytes() and np.array_equal(status2, status)


def test_chunks_give_identical_bytes(W):
    from bart_amd import engine
    rows = _rows(W, n=60, seed=5)
    ref = engine.posterior_tp(rows, Q, chunk=len(rows))
    for chunk in (1, 7):
        got = engine.posterior_tp(rows, Q, chunk=chunk)
        assert got[0].tobytes() == ref[0].tobytes() and np.array_equal(got[1], ref[1]) and got[2] == ref[2]


def test_all_rejected_and_refusals(W):
    from bart_amd import engine, transit_module as trm
    rows = _rows(W, n=20, seed=7)
    rows[:, 4] = 3.5
    env, status, ngood, ranks, order = engine.posterior_tp(rows, Q, want_order=True)
    assert ngood == 0 and np.all(status == 1) and np.all(np.isnan(env)) and ranks is None
    with pytest.raises(trm.TransitError, match="nq"):
        engine.posterior_tp(rows, [50.0] * 9)
    with pytest.raises(trm.TransitError, match="npars"):
        engine.posterior_tp(rows[:, :-1], Q)
    with pytest.raises(trm.TransitError, match=r"q\[1\]"):
        engine.posterior_tp(rows, [50.0, 101.0])


def test_cf_posterior_device_envelopes(W, tmp_path):
    """cf.posterior(envelopes='device') against the host envelopes on a small posterior: band and status bit for bit,
    the envelopes within the 2-ulp bound; NaN envelopes when nothing is accepted.  (cf.posterior makes workers of its
    own; the module's worker is rebuilt afterwards.)"""
    from bart_amd import BARTfunc, cf
    params, stepsize = cf._mcmc_vectors(W["cfg"])
    free = np.nonzero(stepsize)[0]
    nchains, niter, burnin = 3, 15, 4
    rng = np.random.default_rng(21)
    pmin, pmax = W["pmin"], W["pmax"]
    chains = pmin[free, None] + (pmax - pmin)[free, None] * rng.random((nchains, len(free), niter))
    W["worker"].close()
    try:
        host = cf.posterior(chains, W["cfg"], W["wcfg"].filters, burnin, chunk=7)
        dev = cf.posterior(chains, W["cfg"], W["wcfg"].filters, burnin, chunk=7, envelopes="device")
        assert set(host) == set(dev) and dev["kind"] == host["kind"]
        assert np.array_equal(dev["band"], host["band"], equal_nan=True) and np.array_equal(dev["status"], host["status"])
        good = host["band"][host["status"] == 0]
        n = len(good)
        assert 0 < n < len(host["band"])
        flat = np.sort(good.reshape(n, -1), axis=0)
        for k, q in (("median", 50.0), *cf.PERCENTILES.items()):
            lo, hi = int(np.floor((n - 1) * (q / 100.0))), min(int(np.floor((n - 1) * (q / 100.0))) + 1, n - 1)
            assert dev[k].shape == host[k].shape
            assert qr.within_two_ulp(dev[k].ravel(), host[k].ravel(), flat[lo], flat[hi]), k
        bad = chains.copy()
        bad[:, list(free).index(4)] = 3.5
        none = cf.posterior(bad, W["cfg"], W["wcfg"].filters, burnin, envelopes="device")
        assert np.all(none["status"] != 0) and all(np.all(np.isnan(none[k])) for k in ("median", *cf.PERCENTILES))
        with pytest.raises(ValueError):
            cf.posterior(chains, W["cfg"], W["wcfg"].filters, burnin, envelopes="gpu")
    finally:
        W["worker"] = BARTfunc.Worker(W["wcfg"], carry=False)


def test_retrieve_writes_tp_envelopes(W, tmp_path):
    """`retrieve --resident --tp-envelopes` on a short chain: tp_envelopes.npz beside output.npy, its arrays those of
    posterior.tp_envelopes on the written output.npy.  Without the flag no such file."""
    from bart_amd import BARTfunc, cf, posterior, retrieve
    w = W["worker"]
    params, stepsize = cf._mcmc_vectors(W["cfg"])
    data = w.step(params)[0]
    line = lambda v: " ".join(repr(float(x)) for x in v)
    cfg = str(tmp_path / "run.cfg")
    with open(cfg, "w") as f:
        f.write(open(W["cfg"]).read())
        f.write("pmin = %s\npmax = %s\ndata = %s\nuncert = %s\n" % (line(W["pmin"]), line(W["pmax"]), line(data),
                                                                   line(0.02 * np.abs(data))))
        f.write("nchains = 4\nnumit = 160\nburnin = 10\nwalk = snooker\nseed = 3\n")
    w.close()
    try:
        out = str(tmp_path / "o")
        res = retrieve.main(["-c", cfg, "--resident", "--tp-envelopes", "--out", out])
        z = np.load(os.path.join(out, "tp_envelopes.npz"))
        env = posterior.tp_envelopes(os.path.join(out, "output.npy"), cfg, int(z["burnin"]))
        assert int(z["burnin"]) == 10 and env["ngood"] == int(z["ngood"]) > 0
        for k in ("median", "lo1", "hi1", "lo2", "hi2", "status", "pressure"):
            assert z[k].tobytes() == env[k].tobytes(), k
            assert np.array_equal(res["tp_envelopes"][k], env[k], equal_nan=True)
        assert np.all(z["lo2"] <= z["lo1"]) and np.all(z["lo1"] <= z["median"]) and np.all(z["median"] <= z["hi1"])
        out2 = str(tmp_path / "o2")
        retrieve.main(["-c", cfg, "--resident", "--out", out2])
        assert not os.path.exists(os.path.join(out2, "tp_envelopes.npz"))
        assert open(os.path.join(out2, "output.npy"), "rb").read() == open(os.path.join(out, "output.npy"), "rb").read()
    finally:
        W["worker"] = BARTfunc.Worker(W["wcfg"], carry=False)


@pytest.mark.parametrize("model,pttype", [("line", "line"), ("noinv", "madhu_noinv")])
def test_against_the_reference_envelopes(W, tmp_path, model, pttype):
    """tests/golden/tp_envelopes.npz (make_tp_envelope_golden.py: the reference's PT_generator on every stacked sample,
    np.percentile as bestFit.py:461-465): posterior.tp_envelopes on the same output.npy-shaped array, at the rtol = 1e-13
    tests/test_golden.py grants these T(p) models.  The fixture's layers run top to bottom, the engine's the other way."""
    from bart_amd import BARTfunc, posterior, synthcfg
    g = np.load(os.path.join(G, "tp_envelopes.npz"))
    params, stepsize = g[model + "_params"], g[model + "_stepsize"]
    case, cfg = synthcfg.make_worker_case(str(tmp_path), nwave=601, nlayers=60, params=list(params))
    assert np.array_equal(case.press_bar[::-1], g["p"])
    text = open(cfg).read().replace("PTtype = line", "PTtype = " + pttype)
    assert ("Tmin = %.1f" % g["Tmin"]) in text and ("Tmax = %.1f" % g["Tmax"]) in text
    with open(cfg, "w") as f:
        f.write(text + "stepsize = " + " ".join(repr(float(s)) for s in stepsize) + "\n")
    W["worker"].close()
    try:
        env = posterior.tp_envelopes(g[model + "_chain"], cfg, int(g[model + "_burnin"]), chunk=64)
    finally:
        W["worker"] = BARTfunc.Worker(W["wcfg"], carry=False)
    assert np.array_equal(env["pressure"][::-1], g["p"] * 1e6) or np.allclose(env["pressure"][::-1], g["p"] * 1e6, rtol=1e-12)
    assert np.array_equal(env["status"] == 0, g[model + "_accepted"] == 1) and env["ngood"] == int(g[model + "_accepted"].sum())
    for k in ("median", "lo1", "hi1", "lo2", "hi2"):
        got, want = env[k][::-1], g[model + "_" + k]
        print("%s %s: worst relative difference %.3g" % (model, k, float(np.max(np.abs(got - want) / np.abs(want)))))
    for k in ("median", "lo1", "hi1", "lo2", "hi2"):
        np.testing.assert_allclose(env[k][::-1], g[model + "_" + k], rtol=1e-13)
