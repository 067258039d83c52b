"""GPU, one device, no RCCL: the band integration on gathered blocks (include/bartrt.h,
bartrt_step_bandflux_blocks_dev) gives the full-spectrum band integration's bits.  One unsharded engine stands in for
any rank count: its full spectra are laid out as the slots an all-gather of n ranks leaves (slot r = [nwalkers][W_r]
packed, unused tails poisoned with NaN) and both kernels must return the same band fluxes and statuses (torch.equal),
with filter windows inside a block, across three or more blocks, on either side of a block edge and at the grid's two
ends, and the energy balance rejecting some walkers and not others."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RANKS = (1, 2, 3, 5, 8)
GOOD = np.array([-2.0, 0.0, 1.0, 0.0, 0.98, -0.5])
HOT = np.array([-1.0, -2.0, -2.0, 0.0, 1.2, -0.5])      # T > Tmax deep down: status 1
RICH = np.array([-2.0, 0.0, 1.0, 0.0, 0.98, 4.1])       # CH4 > 1, q < 0: status 2


def _starts(total, n):
    return [total * r // n for r in range(n + 1)]


def _filters(total, n, rng):
    """(idx0, npts) of the windows: inside one block, across most of the grid (three or more blocks once n >= 3),
    two samples on either side of a block edge, the grid's first and last samples."""
    s = _starts(total, n)
    b = n // 2
    inside = (s[b] + 2, min(41, s[b + 1] - s[b] - 4))
    span = (total // 20, total - 2 * (total // 20))
    edge = s[1] if n > 1 else total // 2
    wins = [inside, span, (edge - 1, 2), (0, 25), (total - 30, 30)]
    idx0 = np.array([w[0] for w in wins], np.int32)
    npts = np.array([w[1] for w in wins], np.int32)
    if n >= 3:
        lo, hi = idx0[1], idx0[1] + npts[1] - 1
        assert sum(1 for r in range(n) if s[r] <= hi and s[r + 1] > lo) >= 3
    assert s[b] <= idx0[0] and idx0[0] + npts[0] <= s[b + 1]
    return idx0, npts, rng.uniform(0.2, 1.0, int(npts.sum())), rng.uniform(1e5, 3e5, int(npts.sum()))


def _slots(spec, n):
    """Full spectra [nw, W] -> the receive buffer of an all-gather over n ranks: n slots of nw * wmax doubles."""
    import torch
    nw, total = spec.shape
    s = _starts(total, n)
    wmax = max(s[r + 1] - s[r] for r in range(n))
    buf = torch.full((n, nw * wmax), float("nan"), dtype=torch.float64, device=spec.device)
    for r in range(n):
        wr = s[r + 1] - s[r]
        buf[r, :nw * wr] = spec[:, s[r]:s[r + 1]].reshape(-1)
    return buf.reshape(-1).contiguous()


@pytest.mark.parametrize("nwave", [1777, 2424])
def test_block_bandflux_is_bit_identical_to_full(tmp_path, nwave):
    import torch
    from bart_amd import engine, synth, transit_module as trm
    case = synth.make_case(str(tmp_path / "case"), nlayers=60, nwave=nwave, wnlow=1200.0, opmol=("CH4",), seed=11)
    ptargs = np.load(__file__.rsplit("/", 1)[0] + "/golden/pt_golden.npz")["line_args"]
    imol = [case.species.index("CH4")]
    rng = np.random.default_rng(nwave)
    good = GOOD + rng.normal(0, [0.3, 0.2, 0.2, 0.0, 0.05, 0.4], (6, 6))
    params = np.vstack([good[:3], HOT, good[3:5], RICH, good[5:]])
    nw = len(params)
    engine.init(case.tcfg)
    try:
        assert trm.get_no_samples() == nwave
        wn = torch.from_numpy(trm.get_waveno_arr(nwave)).cuda()
        d_par = torch.from_numpy(params).cuda()
        seen = set()
        for n in RANKS:
            idx0, npts, nif, star = _filters(nwave, n, rng)
            engine.step_setup(ptargs, 400.0, 3000.0, case.abund0, imol, idx0, npts, nif, star, 0.11, solution=0)
            _, status0 = engine.step_profiles_dev(d_par)
            _, _, spec = engine.step_batch_dev(d_par, len(idx0), want_spec=True)
            torch.cuda.synchronize()
            # energy balance on, e_in between the walkers' own outputs: some rejected (3), some not
            st = status0.cpu().numpy()
            assert list(st[[3, 6]]) == [1, 2]
            e_out = np.sort(torch.trapezoid(spec, wn, dim=1).cpu().numpy()[st == 0])
            k = len(e_out) // 2
            engine.step_set_ebalance(True, 0.5 * (e_out[k - 1] + e_out[k]), 1.0)
            st_full, st_blk = status0.clone(), status0.clone()
            band_full = torch.empty((nw, len(idx0)), dtype=torch.float64, device="cuda")
            trm.check(trm.lib().bartrt_step_bandflux_dev(
                C.c_void_p(spec.data_ptr()), nw, C.c_void_p(st_full.data_ptr()), C.c_void_p(band_full.data_ptr()),
                engine._stream_ptr()))
            band_blk = engine.step_bandflux_blocks_dev(_slots(spec, n), n, st_blk, len(idx0))
            torch.cuda.synchronize()
            got = sorted(set(st_full.cpu().tolist()))
            assert got == [0, 1, 2, 3], got
            print("nwave %d n %d: statuses %s, bands %s" % (nwave, n, st_blk.cpu().tolist(),
                                                            band_blk[0].cpu().tolist()))
            assert torch.equal(st_blk, st_full), (n, st_blk, st_full)
            assert torch.equal(band_blk, band_full), (n, (band_blk - band_full).abs().max())
            seen.add(n)
        assert seen == set(RANKS)
        # rank counts the grid cannot hold are refused
        blk = torch.zeros(nwave + 1, dtype=torch.float64, device="cuda")
        for bad in (0, nwave + 1):
            assert trm.lib().bartrt_step_bandflux_blocks_dev(
                C.c_void_p(blk.data_ptr()), bad, 1, C.c_void_p(status0.data_ptr()),
                C.c_void_p(band_full.data_ptr()), None) < 0
    finally:
        trm.free_memory()
