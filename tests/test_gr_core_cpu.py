"""CPU: the Gelman-Rubin statistic of the resident sampler (bart_amd/csrc/gr_core.hpp) through a stand-alone host
program (tests/gr_core_host.cpp, its own main, built here with g++ and the address / undefined-behaviour sanitizers)
that runs the very leaf / merge / psrf functions the device kernels run.  Held against tests/gr_restate.py: the
header's order restated in plain Python doubles, and exact rationals.

Accuracy as measured (x86-64, g++; relative deviation of R from the exact value over gr_restate.EXACT_SHAPES): host
build 1.07e-08, numpy's sampler.gelman_rubin 4.41e-09, so the bound the tests assert is 8 x 1.07e-08 = 8.55e-08.  Both
come from the column of mean 1e8 and spread 1 alone: a chain's mean is a double near 1e8, known to 1.5e-8, and the
variance of those means enters R; on every other column both stay below 2e-12 (the radius of 97 000 +- 3) and below
3e-14 elsewhere.  A one-pass sum-of-squares variant gives R = inf or values 2 to 8 % off on the 1e8 column: six
orders of magnitude past the bound."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gr_restate as gr  # noqa: E402


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return gr.build_host(tmp_path_factory.mktemp("gr_core"))


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


@pytest.mark.parametrize("shape", gr.SHAPES, ids=lambda s: "rows%d-ch%d-p%d-r%d" % s)
def test_host_build_is_the_restatement(host, shape):
    """Triples bit for bit; R to the last bit or one ulp (the square root and the divisions are correctly rounded on
    both sides: one ulp is the issue's allowance, none is expected)."""
    chain, step, r0, r1 = gr.case(shape)
    psrf, triples, conv = host("stat", chain, step, r0, r1)
    rp, rt, rc = gr.statistic(chain, step, r0, r1)
    assert triples.tobytes() == rt.tobytes()
    free = step > 0
    assert free.any() and np.all(psrf[~free] == 0.0) and np.all(triples[:, ~free] == 0.0)
    assert np.all(np.isfinite(psrf[free])) and np.all(psrf[free] > 0.86)      # (R >= sqrt(3 / 4) at four rows)
    assert np.all(triples[:, free, 0] == r1 - r0)
    assert float(ulps(psrf[free], rp[free]).max()) <= 1.0
    assert conv == rc
    # the threshold decides: just above the largest R converges, just below does not
    top = float(psrf[free].max())
    assert host("stat", chain, step, r0, r1, top * (1 + 1e-12))[2] == 1
    assert host("stat", chain, step, r0, r1, top * (1 - 1e-12))[2] == 0


def test_accuracy_against_exact_rationals(host):
    """The measured deviations (module docstring, MEASUREMENTS.md) and the bound: the host build lies within it on
    every exact shape, and a one-pass implementation fails it on the 1e8 column."""
    m = gr.measure(host)
    assert m["bound"] == 8.0 * max(m["host"], m["numpy"], 2.0 ** -53) and m["bound"] > 0.0
    assert m["host"] <= m["bound"] and m["numpy"] <= m["bound"]
    assert m["onepass"] > 1e3 * m["bound"], m
    for shape in gr.EXACT_SHAPES:
        chain, step, r0, r1 = gr.case(shape)
        want = gr.exact(chain, step, r0, r1)
        assert gr.deviation(host("stat", chain, step, r0, r1)[0], want) <= m["bound"]


def test_constant_column_and_no_test(host):
    chain, step, r0, r1 = gr.case((gr.TILE + 1, 3, 7, 3))
    # a free parameter that never moved: W = 0 and B = 0 give NaN; chains stuck at different values: inf
    flat = chain.copy()
    flat[:, :, 4] = 97000.0
    psrf, triples, conv = host("stat", flat, step, r0, r1, 1e9)
    assert math.isnan(psrf[4]) and conv == 0 and np.all(triples[:, 4, 2] == 0.0)
    rp, rt, rc = gr.statistic(flat, step, r0, r1, 1e9)
    assert math.isnan(rp[4]) and rc == 0 and triples.tobytes() == rt.tobytes()
    flat[:, :, 4] += np.arange(3)[:, None]
    psrf, _, conv = host("stat", flat, step, r0, r1, 1e9)
    assert math.isinf(psrf[4]) and conv == 0
    assert math.isinf(gr.statistic(flat, step, r0, r1, 1e9)[0][4])
    assert host("stat", chain, step, r0, r1, 1e9)[2] == 1          # (the same chains without the stuck column)
    # fewer than four rows, or one chain: no test, every output zero
    for ch, a, b in ((chain, 3, 6), (chain[:1], 3, 200)):
        psrf, triples, conv = host("stat", ch, step, a, b, 1e9)
        assert not psrf.any() and not triples.any() and conv == 0
        assert gr.statistic(ch, step, a, b, 1e9)[2] == 0
    # no free parameter: nothing to converge
    assert host("stat", chain, np.zeros(7), r0, r1, 1e9)[2] == 0


def test_configuration_reads_grexit(tmp_path):
    from bart_amd import sampler
    keys = "params = 1 2\npmin = 0 0\npmax = 3 3\nstepsize = 0.1 0.1\ndata = 1\nuncert = 0.1\n"
    (tmp_path / "a.cfg").write_text("[MCMC]\n" + keys + "grtest = True\ngrexit = True\ngrcheck = 512\ngrthreshold = 1.05\n")
    (tmp_path / "b.cfg").write_text("[MCMC]\n" + keys)
    a, b = (sampler.SamplerConfig.from_cfg(str(tmp_path / n)) for n in ("a.cfg", "b.cfg"))
    assert (a.grexit, a.grcheck, a.grthreshold) == (True, 512, 1.05)
    assert (b.grexit, b.grcheck, b.grthreshold) == (False, None, 1.01)
    # the loops that do not stop on convergence say so, once
    lines = []
    a.numit, a.nchains = 8, 2
    sampler.run(lambda p: np.ones((len(p), 1)), a, log=lines.append)
    assert sum("grexit" in l for l in lines) == 1
