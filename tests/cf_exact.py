"""The contribution-function kernels (csrc/contrib.hip) restated in mpmath at 50 digits -- TEST INFRASTRUCTURE ONLY.

Written from the definitions in the header comment of csrc/contrib.hip; it shares no code with the kernels, with
oracle/rt_oracle.c or with tests/cf_restate.py.  The optical depth is NOT restated here: the vertical depth under the
three integration rules is eclipse_restate.taus, the chord depth transit_restate.columns, each with the bound its module
derives.  Inputs are the doubles the kernels read, each taken exactly: the walker's layer records, rdlp, the radii and
the filter tables (engine.cf_records), the table values at the records' offsets (transit_restate.table_inputs /
.extinction, with their error term de), the wavenumbers.  Layers count FROM THE TOP (k = 0 the top layer); the
outputs' atm order (bottom first) is applied last (atm()).

    tau[k]   the rule's depth for k <= kend, tau[kend] below it (a cloud deck: the depth repeats); no toomuch cut
    tr[k]  = exp(-tau[k])
    cf[0]  = 0,  cf[k] = B(T_k, nu) (exp(-tau[k-1]) - exp(-tau[k])) rdlp[k],  B = 2 h c^2 nu^3 / (exp(c1_k nu) - 1)
    band_f[k] = sum_i h_i resp_i v_i[k] / trapz(resp_f),  trapz = sum_s (resp_s + resp_{s+1}) / 2,
             i over the window's samples, h = 1/2 at the window's two ends and 1 between them

RUNNING ERROR BOUNDS: what a correct fp64 evaluation in the kernels' order of operations may differ by; first order in
u = 2^-53, every count rounded up, 1e-6 of slack.  DERIVED from the arithmetic, never fitted to a device result.  The
documented figures: exp_rt within EXP_REL = 4e-16 of its interpolant and the interpolant within 7.5e-14 + 2.4e-17 |n|
of exp, |n| <= 1.4427 |x| + 1 (csrc/kernels.hpp); rcp_n1 2.3e-15; the Planck term as eclipse_restate.planck states it.

  transmittance.  The argument -tau is exact (a sign), fmax(., kExpMin) replaces exp(-tau) < exp(-708) by exp(-708):
      an ABSOLUTE allowance of 3.4e-308.   dE_k = E_k (4e-16 + 7.5e-14 + 2.4e-17 (1.4427 tau_k + 1) + dtau_k) + 3.4e-308.
      Below kend the device evaluates the SAME tau again: the same bits, so tr repeats to the bit and the difference of
      two such values is exactly 0 (dv = 0 there, asserted as equality by the GPU tests).
  difference.  D_k = E_{k-1} - E_k rounds once: dD_k = dE_{k-1} + dE_k + u |D_k|.  This is where the bound stops being
      relative: on an optically thin column E_{k-1} and E_k agree to many digits while each carries exp_rt's 7.5e-14 ON
      ITS VALUE, so dD ~ 1.5e-13 whatever D is.  The bound is small against the ROW's largest value exactly where some
      layer of the row has D ~ 0.01 or more; the thin cases are held in absolute terms (tests/test_cf_exact_cpu.py).
  contribution.  B (relB of eclipse_restate.planck: the exponent's product, exp_rt, the subtraction, rcp_n1, the
      numerator's products), the product B D and the product with rdlp (read back: an input) round once each:
      dcf_k = |cf_k| (relB_k + 2 u) + B_k rdlp_k dD_k.
  band, the reduction's part (dred).  Per tile and filter: lane (j, q) runs a 16-term fma chain (16 roundings on any
      term), two butterflies add the quarters (2); cf_block_sums adds the filter's T_f tiles in tile order from 0 (T_f);
      cf_combine adds the R ranks' slots from 0 (R; one rank: 0 + s is exact, counted all the same) and divides (1, on
      the result):      dred = (16 + 2 + T_f + R) u sum_i |w_i v_i| / |trapz| + u |band|.
  band, the whole (dband).  The weights w_i = h_i resp_i are exact (a half of a double).  trapz(resp) is summed on the
      host in window order, each term a rounded sum halved exactly: dtrapz = (n + 1) u sum_s |resp_s + resp_{s+1}| / 2.
      dband = sum_i |w_i| dv_i / |trapz| + dred + |band| dtrapz / |trapz|.

MUTANTS: deliberate mistakes, each a switch below; tests/test_cf_exact_cpu.py holds that each leaves the bound."""
from __future__ import annotations

import mpmath
import numpy as np

import eclipse_restate as er
import transit_restate as tr
from transit_restate import DPS, EXP_REL, EXP_RT_FIT, EXP_RT_LN2, SLACK, U

mpf = mpmath.mpf
EXP_MIN_ABS = er.EXP_MIN_ABS
KIND_CF, KIND_TR = 0, 1
ROWS = 16          # kCfRows

LAYER_MUTANTS = ("tau_next", "rdlp_next", "planck_prev", "freeze_late", "freeze_early", "cf0_nonzero", "block_row_reused",
                 "full_reversed")
BAND_MUTANTS = ("half_inward", "lane63_dropped", "lane64_dropped", "tile_missing")
MUTANTS = LAYER_MUTANTS + BAND_MUTANTS


class Columns:
    """The exact inputs of one walker on the grid samples `cols`: e[L, nc] mpf with de[L, nc], A[L, nc]; dr[L], c1[L],
    rdlp[L] doubles; nu[nc]; kend; transit: ch (transit_restate.Chords of the radii)."""


def from_records(o, rec, cols, wn):
    """rec: engine.cf_records(walker); o: the oracle engine of the case (its readers of the tables)."""
    c = Columns()
    cf, v, allow = tr.table_inputs(o, rec["coef"], rec["idx"], cols, wn=wn)
    c.e, c.de, c.A = tr.extinction(cf, v, allow)
    c.cols = list(int(i) for i in cols)
    c.nu = np.asarray(wn, float)[c.cols]
    c.dr, c.c1 = np.asarray(rec["coef"][:, 0], float), np.asarray(rec["coef"][:, 1], float)
    c.rdlp = np.asarray(rec["rdlp"], float)
    c.L, c.kend = len(c.dr), tr.kend_of(rec["kstop"])
    c.ch = tr.Chords(rec["rtop"]) if "rtop" in rec else None
    return c


def from_oracle(o, prof, cols, deck_logp=None):
    """No GPU: the ORACLE's own extinction, radii and temperatures as the exact inputs (de = 0), rdlp with cf_setup's
    arithmetic on the oracle's pressures.  deck_logp: the cloud top (log10 bar) the oracle has been given, or None."""
    c = Columns()
    prof = np.asarray(prof, float).ravel()
    ext, rad = o.extinction(prof)
    L = len(rad)
    c.cols = list(int(i) for i in cols)
    with mpmath.workdps(DPS):
        c.e = tr.mp_array(ext[::-1][:, c.cols])
    c.de, c.A = np.zeros(c.e.shape), np.abs(ext[::-1][:, c.cols])
    r = rad[::-1]
    c.dr = np.concatenate([[0.0], r[:-1] - r[1:]])
    c.c1 = (er.K_H * er.K_LS / er.K_KB) / prof[:L][::-1]
    c.nu = np.asarray(o.wn, float)[c.cols]
    p = np.asarray(o.press, float)          # atm order
    c.rdlp = np.zeros(L)
    for k in range(1, L):
        c.rdlp[k] = 1.0 / (np.log(p[L - 1 - k]) - np.log(p[L - k]))
    c.L, c.kend = L, L - 1
    if o.c.has_cloud:
        for k in range(L):
            if p[L - 1 - k] >= o.c.cloudtop:
                c.kend = k
                break
    c.ch = tr.Chords(r) if o.c.solution == 1 else None
    return c


def depths(c: Columns, rule, transit=False):
    """-> (tau[L][nc] mpf, dtau[L, nc]) down to the BOTTOM layer (no deck: values() freezes)."""
    with mpmath.workdps(DPS):
        L, nc = c.e.shape
        if transit:
            col = tr.columns(c.e, c.de, c.A, c.ch, L - 1, 1e300, False, 1.0, exp_rt=True)
            return col.tau, col.dtau
        drm = [mpf(float(x)) for x in c.dr]
        tau, dtau = np.empty((L, nc), object), np.zeros((L, nc))
        for i in range(nc):
            t, dt, _ = er.taus(list(c.e[:, i]), list(c.de[:, i]), drm, L - 1, rule == 1)
            tau[:, i], dtau[:, i] = t, dt
        return tau, dtau


def values(c: Columns, tau, dtau, kind, mutant=None):
    """-> (v[L, nc] mpf, dv[L, nc]) from the top: tr (kind 1) or cf (kind 0)."""
    with mpmath.workdps(DPS):
        L, nc = tau.shape
        kf = c.kend + (1 if mutant == "freeze_late" else -1 if mutant == "freeze_early" else 0)
        kf = min(max(kf, 0), L - 1)
        v, dv = np.empty((L, nc), object), np.zeros((L, nc))
        for i in range(nc):
            t = [tau[min(k, kf), i] for k in range(L)]
            dt = [dtau[min(k, kf), i] for k in range(L)]
            E = [mpmath.exp(-x) for x in t]
            dE = [float(E[k]) * (EXP_REL + EXP_RT_FIT + EXP_RT_LN2 * (1.4427 * float(t[k]) + 1.0) + dt[k]) * SLACK + EXP_MIN_ABS
                  for k in range(L)]
            if kind == KIND_TR:
                v[:, i], dv[:, i] = E, dE
                continue
            nu = float(c.nu[i])
            Bs = [er.planck(mpf(float(c.c1[k])) * mpf(nu), nu) for k in range(L)]
            v[0, i] = mpf(0)
            for k in range(1, L):
                a, b = (k, min(k + 1, L - 1)) if mutant == "tau_next" else (k - 1, k)
                B, relB = Bs[k - 1] if mutant == "planck_prev" else Bs[k]
                rd = float(c.rdlp[min(k + 1, L - 1)] if mutant == "rdlp_next" else c.rdlp[k])
                D = E[a] - E[b]
                if min(a, kf) == min(b, kf):       # the same depth evaluated twice: the same bits, exactly 0
                    v[k, i] = mpf(0)
                    continue
                dD = dE[a] + dE[b] + U * abs(float(D))
                v[k, i] = B * D * mpf(rd)
                dv[k, i] = (abs(float(v[k, i])) * (relB + 2 * U) + float(B) * abs(rd) * dD) * SLACK
            if mutant == "cf0_nonzero" and L > 1:
                v[0, i] = Bs[0][0] * (1 - E[0]) * mpf(float(c.rdlp[1]))
        if mutant == "block_row_reused" and L % ROWS and L > ROWS:
            v[L - 1] = v[L - 1 - ROWS]
    return v, dv


def atm(v, mutant=None):
    """Layers from the top -> the outputs' atm order along axis 0 (the mutant: not for the full output)."""
    return v if mutant == "full_reversed" else v[::-1]


def exact_weights(idx0, npts, resp, mutant=None):
    """-> (w[npts] mpf, trapz mpf, dtrapz): the weights on the window's samples and the divisor."""
    with mpmath.workdps(DPS):
        r = [mpf(float(x)) for x in resp]
        h = [mpf(1)] * npts
        h[0] = h[-1] = mpf(1) / 2
        if mutant == "half_inward" and npts >= 4:
            h[0], h[1], h[-1], h[-2] = mpf(1), mpf(1) / 2, mpf(1), mpf(1) / 2
        w = [a * b for a, b in zip(h, r)]
        for s in range(npts):
            lane = (idx0 + s) % 64
            if (mutant == "lane63_dropped" and lane == 63) or (mutant == "lane64_dropped" and lane == 0 and idx0 + s > 0):
                w[s] = mpf(0)
        t = sum(((r[s] + r[s + 1]) / 2 for s in range(npts - 1)), mpf(0))
        dt = (npts + 1) * U * sum(abs(float(r[s] + r[s + 1])) / 2 for s in range(npts - 1)) * SLACK
    return w, t, dt


def band(c: Columns, v, dv, windows, lo=0, nranks=1, mutant=None):
    """The band rows of v[L, nc] (from the top) -> (band[nf, L] mpf, dband[nf, L], dred[nf, L]), layers from the top.
    windows: [(idx0, npts, resp)] on the full grid, every sample among c.cols; lo: the first sample of each rank's
    block, ascending (0: one engine on the whole grid) -- tiles count from a block's start; nranks: the slots added."""
    pos = {g: n for n, g in enumerate(c.cols)}
    los = list(lo) if isinstance(lo, (list, tuple)) else [lo]
    with mpmath.workdps(DPS):
        L = v.shape[0]
        out, dout, dred = np.empty((len(windows), L), object), np.zeros((len(windows), L)), np.zeros((len(windows), L))
        for f, (idx0, npts, resp) in enumerate(windows):
            w, t, dt = exact_weights(idx0, npts, resp, mutant)
            sel = [pos[idx0 + s] for s in range(npts)]
            # the tiles the window meets, per rank block (the blocks' starts `los`, ascending; the last runs to the end)
            tiles = set()
            for s in range(npts):
                g = idx0 + s
                b = max(n for n, x in enumerate(los) if x <= g)
                tiles.add((b, (g - los[b]) // 64))
            if mutant == "tile_missing" and len(tiles) > 1:
                gone = max(tiles)
                for s in range(npts):
                    g = idx0 + s
                    b = max(n for n, x in enumerate(los) if x <= g)
                    if (b, (g - los[b]) // 64) == gone:
                        w[s] = mpf(0)
            nred = ROWS + 2 + len(tiles) + nranks
            wf = np.array([abs(float(x)) for x in w])
            tf = abs(float(t))
            for k in range(L):
                out[f, k] = sum((w[s] * v[k, sel[s]] for s in range(npts)), mpf(0)) / t
                mag = float(np.sum(wf * np.abs(tr.to_float(v[k, sel]))))
                bf = abs(float(out[f, k]))
                dred[f, k] = (nred * U * mag / tf + U * bf) * SLACK
                dout[f, k] = (float(np.sum(wf * dv[k, sel])) / tf + bf * dt / tf) * SLACK + dred[f, k]
    return out, dout, dred


def reduction_of(full_top, wt_rows, trapz, tile_lists):
    """The reduction on its own, from the device's OWN full output: full_top[L, W] doubles (layers from the top),
    wt_rows[f] = [(first sample, weights[<= 64])] the read-back entries of filter f in tile order, trapz[f] the
    read-back divisors -> (band[nf, L] floats by math.fsum, the exactly rounded sum; dred[nf, L])."""
    import math
    L = full_top.shape[0]
    nf = len(wt_rows)
    out, dred = np.zeros((nf, L)), np.zeros((nf, L))
    for f in range(nf):
        nred = ROWS + 2 + len(wt_rows[f]) + tile_lists
        for k in range(L):
            terms = [float(x) * float(y) for first, wts in wt_rows[f] for x, y in zip(wts, full_top[k, first:first + len(wts)])]
            # (the products are rounded here and fused on the device: one more rounding on every term)
            s = math.fsum(terms)
            out[f, k] = s / trapz[f]
            dred[f, k] = ((nred + 1) * U * math.fsum(abs(x) for x in terms) / abs(trapz[f]) + 2 * U * abs(out[f, k])) * SLACK
    return out, dred


def absdev(got, ref):
    return tr.absdev(got, ref)


def ratio(dev, bound):
    """max over the array of dev / bound (0 / 0 = 0, x / 0 = inf)."""
    dev, bound = np.asarray(dev, float), np.asarray(bound, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, dev / bound, np.where(dev == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0
