"""The engines and profiles of tests/test_prep_restate_cpu.py and tests/test_gpu_prep_edges.py, built once for both:
what the CPU test holds the restatement to the oracle on is what the GPU test feeds the device."""
from __future__ import annotations

import os

import numpy as np

# layers below (k) and above (39 - k) both take 0, 1, 7, 8, 9, 15, 16, 17: either walk of the hydrostatic chain runs
# empty, as remainder only, as exactly one block of eight, with a prefetched second block, and as block + remainder
REF_K = (0, 1, 7, 8, 9, 15, 16, 17, 22, 23, 24, 30, 31, 32, 38, 39)
REF_CASES = [("L40-k%02d-%s" % (k, v), 40, k, v) for k in REF_K for v in ("on", "off")] + \
            [("L40-below-bottom", 40, None, "below"), ("L40-above-top", 40, None, "above"),
             ("L130-off", 130, 43, "off"), ("L257-off", 257, 85, "off")]


def _mk(path, **kw):
    from bart_amd import synth
    kw.setdefault("opmol", ("CH4",))
    kw.setdefault("tempdelt", 650.0)
    kw.setdefault("nwave", 32)
    kw.setdefault("cia", False)
    return synth.make_case(str(path), **kw)


def ref_case(path, L, k, variant, **kw):
    """refpress on layer k ("on": the layer's own %.4e string), a third of the way in log p towards a neighbour
    ("off": the upper one for even k, the lower one for odd k; layer k stays the closest in |p - p0| either way: the
    grid's ratio is 1.5 at 40 layers and the step a factor 1.15), twice the bottom pressure, half the top pressure."""
    press = _mk(path, nlayers=L, write=False).press_bar
    if variant == "on":
        text = "%.4e" % press[k]
    elif variant == "off":
        n = k + 1 if (k % 2 == 0 and k + 1 < L) or k == 0 else k - 1
        text = repr(float(10.0 ** (np.log10(press[k]) + (np.log10(press[n]) - np.log10(press[k])) / 3.0)))
    else:
        text = repr(float(2.0 * press[0] if variant == "below" else 0.5 * press[-1]))
    extra = dict(kw.pop("extra_keys", {}) or {})
    extra["refpress"] = text
    c = _mk(path, nlayers=L, refpress=float(text), extra_keys=extra, **kw)
    if variant in ("on", "off"):
        assert int(np.argmin(np.abs(c.press_bar - float(text)))) == k
        assert (c.press_bar[k] == float(text)) == (variant == "on")
    return c


def profiles(case, n, seed):
    """n profiles [n][(S+1) L]: the atmosphere file's own first, then seeded ones -- temperatures anywhere inside the
    table's grid, trace abundances scaled by up to 100 either way (He and H2 fill the rest, when both are there)."""
    rng = np.random.default_rng(seed)
    L = len(case.press_bar)
    out = [case.profiles().ravel()]
    for _ in range(n - 1):
        t = case.temp0 + rng.uniform(-600, 1200) + 250 * np.sin(np.linspace(0, rng.uniform(1, 9), L) + rng.uniform(0, 6))
        t = np.clip(t, case.tgrid[0] + 1.0, case.tgrid[-1] - 1.0)
        ab = case.abund0.copy()
        for s in range(2, ab.shape[1]):
            ab[:, s] *= 10 ** rng.uniform(-2, 1)
        if case.species[:2] == ["He", "H2"]:
            q = 1 - ab[:, 2:].sum(1)
            ab[:, 1] = 0.85 * q
            ab[:, 0] = 0.15 * q
        out.append(case.profiles(t, ab).ravel())
    return np.array(out)


OWN_SCATTERING = (-3.0, 0.25, 2.0)     # a walker's own scattering values (path (c) with step_set_extras)


def iso_profile(case, T):
    return case.profiles(np.full(len(case.press_bar), float(T))).ravel()


# ---- temperature edges ------------------------------------------------------------------------------------------------
CIA_T1 = (450.0, 700.0, 1250.0, 1500.0, 2600.0, 2900.0)      # H2-H2: uneven, first node above the table's
CIA_T2 = (620.0, 980.0, 1730.0, 2950.0)                      # H2-He
EDGE_NODES = (400.0, 1700.0, 3000.0)                         # the nodes approached to one ulp


def _cia_file(path, s1, s2, temps, wn, seed, scale=1e-7):
    from bart_amd import synth
    rng = np.random.default_rng(seed)
    cw = np.arange(wn[0] - 20.0, wn[-1] + 20.1, 7.0)
    base = scale * (1.0 + 0.5 * np.sin(cw / 9.0)) * np.exp(0.2 * rng.normal(size=len(cw)))
    t = np.asarray(temps, float)
    al = base[None, :] * (1.0 + 0.4 * (t[:, None] - 400.0) / 2600.0 + 0.1 * np.sin(t[:, None] / 300.0))
    synth.write_cia(path, s1, s2, t, cw, al)
    return path


def temp_edge_case(path, **kw):
    """L = 24, four table molecules on the default 100 K grid, two cross-section files on CIA_T1 / CIA_T2."""
    from bart_amd import synth
    os.makedirs(str(path), exist_ok=True)
    wn = 1000.0 + np.arange(32)
    files = [_cia_file(os.path.join(str(path), "cs_H2H2.dat"), "H2", "H2", CIA_T1, wn, 11),
             _cia_file(os.path.join(str(path), "cs_H2He.dat"), "H2", "He", CIA_T2, wn, 12)]
    extra = dict(kw.pop("extra_keys", {}) or {})
    extra["csfile"] = ",".join(files)
    return synth.make_case(str(path), nlayers=24, nwave=32, cia=False, extra_keys=extra, **kw)


def temp_edge_profiles(case, overshoot=150.0):
    """The six hand-made profiles, by name."""
    g, L = case.tgrid, len(case.press_bar)
    near = []
    for n in EDGE_NODES:
        near += [np.nextafter(n, -np.inf), n, np.nextafter(n, np.inf)]
    on_cia = [t for t in CIA_T1 + CIA_T2 if t % 100.0 != 0.0]
    temps = {
        "on-nodes": g[np.round(np.linspace(0, len(g) - 1, L)).astype(int)],
        "first-node": np.full(L, g[0]),
        "last-node": np.full(L, g[-1]),
        "one-ulp": np.array([near[l % len(near)] for l in range(L)]),
        "ramp": np.linspace(g[0] - overshoot, g[-1] + overshoot, L),
        "on-cia-nodes": np.array([on_cia[l % len(on_cia)] for l in range(L)]),
    }
    return {k: case.profiles(np.asarray(t, float)).ravel() for k, t in temps.items()}


def ramp_overshoot(case, oracle):
    """The largest overshoot of the ramp (150 K, then shorter) at which the oracle's extinction is positive at every
    sample of the two profiles that leave the table's grid (the ramp, and the one that steps one ulp outside it)."""
    for over in (150.0, 100.0, 50.0, 20.0, 5.0):
        p = temp_edge_profiles(case, over)
        if all(np.all(oracle.extinction(p[k])[0] > 0.0) for k in ("ramp", "one-ulp")):
            return over
    raise AssertionError("the synthetic table extrapolates to a negative extinction within 5 K of its grid")


# ---- single-temperature cross sections -----------------------------------------------------------------------------
SINGLE_CASES = [(n, interp, sol) for n in ("alone", "with-seven") for interp in ("linear", "spline")
                for sol in ("eclipse", "transit")]


def single_temp_case(path, which, interp, solution, with_file=True):
    """One H2-H2 file with the single temperature 1000 K; "with-seven": next to an H2-He file of seven.
    with_file = False: the same engine without the single-temperature file."""
    os.makedirs(str(path), exist_ok=True)
    wn = 1000.0 + np.arange(32)
    files = []
    if with_file:
        files.append(_cia_file(os.path.join(str(path), "cs_one.dat"), "H2", "H2", (1000.0,), wn, 21, scale=3e-6))
    if which == "with-seven":
        files.append(_cia_file(os.path.join(str(path), "cs_seven.dat"), "H2", "He", np.arange(400.0, 2801.0, 400.0), wn, 22))
    extra = {"cia_interp": interp, "solution": solution}
    if files:
        extra["csfile"] = ",".join(files)
    if solution == "transit":
        extra["starrad"] = 1.0
    return _mk(path, nlayers=24, extra_keys=extra)


# ---- the stop layer ------------------------------------------------------------------------------------------------------
DECK_BIT = 1 << 30


def cloudtop_logs(p_barye):
    """-> (x_on, x_below, v_below): a log10(bar) value whose 10^x 1e6 is the pressure exactly (None if no double
    gives it), and the largest pressure below it reachable that way with its logarithm (the cfg holds the cloud top as
    a logarithm); found among the doubles around log10 p."""
    x0 = float(np.log10(p_barye / 1e6))
    xs = [x0]
    for _ in range(64):
        xs = [np.nextafter(xs[0], -np.inf)] + xs + [np.nextafter(xs[-1], np.inf)]
    vals = [(10.0 ** float(x)) * 1e6 for x in xs]
    on = [x for x, v in zip(xs, vals) if v == p_barye]
    below = max((v, x) for x, v in zip(xs, vals) if v < p_barye)
    return (float(on[0]) if on else None), float(below[1]), below[0]


def stop_layer_cases(press):
    """-> (l, v_below, [(name, cfg cloudtop, expected kstop)]) on a 24-layer grid (press: barye, atm order): layer l is
    the first of layers 4 .. 19 whose pressure a logarithm reaches exactly."""
    found = [(l, cloudtop_logs(press[l])) for l in range(4, 20)]
    l, (x_on, x_below, v_below) = next((l, f) for l, f in found if f[0] is not None)
    L = len(press)
    return l, v_below, [("on the layer", x_on, (L - 1 - l) | DECK_BIT), ("just below it", x_below, (L - 1 - l) | DECK_BIT),
                        ("above the top", float(np.log10(press[-1] / 1e6)) - 1.0, 0 | DECK_BIT),
                        ("below the bottom", float(np.log10(press[0] / 1e6)) + 1.0, L - 1)]
