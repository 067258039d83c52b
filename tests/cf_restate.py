"""The tests' numpy restatement of BART's contribution-function arithmetic (reference code/cf.py:
Planck :98-111, cf_eq :114-134), vectorised; the band average is bart_amd.cf.band_average.
Layers from the top (index 0 = top), as tau.dat and cf.cf hold them."""
import numpy as np

H, LS, KB = 6.6260755e-27, 2.99792458e10, 1.380658e-16   # code/constants.py:14-16


def planck(temp, wns):
    """B[L][W] = 2 h nu^3 c^2 / (exp(h nu c / (k T)) - 1), erg s-1 cm-2 sr-1 cm."""
    t = np.asarray(temp, float)[:, None]
    w = np.asarray(wns, float)[None, :]
    return (2.0 * H * w ** 3.0 * LS ** 2.0) / (np.exp((H * w * LS) / (KB * t)) - 1.0)


def cf_eq(bb, p_bar, tau):
    """cf[L][W] from B[L][W], pressures p_bar[L] and tau[L][W], all from the top: cf[0] = 0,
    cf[k] = B[k] (exp(-tau[k-1]) - exp(-tau[k])) / (ln(p_k 1e6) - ln(p_{k-1} 1e6))."""
    p = np.asarray(p_bar, float)
    out = np.zeros_like(np.asarray(bb, float))
    dlogp = np.log(p[1:] * 1e6) - np.log(p[:-1] * 1e6)
    out[1:] = bb[1:] * (np.exp(-tau[:-1]) - np.exp(-tau[1:])) / dlogp[:, None]
    return out


def contribution(temp_atm, p_bar_atm, tau, wns):
    """cf[L][W] (from the top) of a profile given in atm order (bottom first) and tau[L][W] from the top."""
    return cf_eq(planck(np.asarray(temp_atm)[::-1], wns), np.asarray(p_bar_atm)[::-1], tau)
