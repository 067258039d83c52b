"""Batched / device-resident front end of libbartrt.so.

``transit_module`` keeps the reference's one-profile-per-call shape; this
module adds what the MI355X build needs on top of the same engine: walker
batches, HBM-resident tensors (torch is used only as the owner of device
memory, streams and the RCCL process group), wavenumber-block sharding with an
all-gather that reassembles each spectrum, and the per-step
converters of code/BARTfunc.py:309-399 on the device.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import transit_module as trm

_check, _ptr = trm.check, trm._ptr


def init(tcfg: str, shard: tuple[int, int] | None = None, device: int | None = None, kernel_by: str | None = None) -> None:
    """An engine IN THIS PROCESS (this module's batched / device-resident calls need one): with `shareOpacity`
    in the cfg the grid is shared through HIP IPC, never through the chain service (include/bartrt.h,
    bartrt_get_share) -- the service is for the reference's one-profile-per-process workers."""
    argv = ["transit", "-c", tcfg, "--no-service"]
    if shard is not None:
        argv += ["--shard", str(shard[0]), str(shard[1])]
    if device is not None:
        argv += ["--device", str(device)]
    trm.transit_init(len(argv), argv)
    if kernel_by is not None:
        # 'whole': a sharded engine's blocks are the unsharded spectrum bit for bit; 'local' (default): the kernel
        # variant fits the block (include/bartrt.h, bartrt_set_kernel_by)
        trm.set_kernel_by(kernel_by)


def nlayers() -> int:
    return _check(trm.lib().bartrt_get_nlayers())


def nspecies() -> int:
    return _check(trm.lib().bartrt_get_nspecies())


def nprof() -> int:
    return _check(trm.lib().bartrt_get_nprof())


def species() -> list[str]:
    buf = C.create_string_buffer(4096)
    _check(trm.lib().bartrt_get_species(buf, 4096))
    return buf.value.decode().split()


def pressure() -> np.ndarray:
    out = np.zeros(nlayers())
    _check(trm.lib().bartrt_get_pressure(_ptr(out), out.size))
    return out


def local_range() -> tuple[int, int]:
    lo, hi = C.c_int(), C.c_int()
    _check(trm.lib().bartrt_get_local_range(C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def run_batch(profiles: np.ndarray, want_ok: bool = False):
    """profiles [nwalkers, (S+1)*L] (host) -> spectra [nwalkers, local samples]."""
    prof = np.ascontiguousarray(profiles, np.double)
    prof = prof.reshape(-1, nprof())
    lo, hi = local_range()
    spec = np.zeros((prof.shape[0], hi - lo))
    ok = np.zeros(prof.shape[0], np.uint8)
    _check(trm.lib().bartrt_run_transit_batch(_ptr(prof), prof.shape[0], prof.shape[1],
                                              _ptr(spec), hi - lo, _ptr(ok)))
    return (spec, ok) if want_ok else spec


def get_tau(walker=None):
    """Optical depth of the latest host-buffer call's profile: (tau[W_local, L], last[W_local]),
    layer index 0 = top (the tau.dat convention, code/cf.py:68-94).  After a batch call the
    walker has to be named (include/bartrt.h, bartrt_get_tau_of)."""
    lo, hi = local_range()
    tau = np.zeros((hi - lo, nlayers()))
    last = np.zeros(hi - lo, np.int32)
    if walker is None:
        _check(trm.lib().bartrt_get_tau(_ptr(tau), _ptr(last), hi - lo, nlayers()))
    else:
        _check(trm.lib().bartrt_get_tau_of(int(walker), _ptr(tau), _ptr(last), hi - lo, nlayers()))
    return tau, last


def get_radius() -> np.ndarray:
    """Hydrostatic radii [L] (cm, atm layer order) of the latest run's first profile."""
    out = np.zeros(nlayers())
    _check(trm.lib().bartrt_get_radius(_ptr(out), out.size))
    return out


def prep_records(walker: int):
    """What the latest launch's preparation wrote for one walker of its batch (diagnostics; include/bartrt.h,
    bartrt_get_prep_records): (coef[L, 4 + 2 M + 2 C], idx[L, 1 + C], kstop, ok), layers from the top.  Raises
    when the launch prepared its walkers inside the RT kernel, and for a walker outside the batch."""
    m, c = C.c_int(), C.c_int()
    _check(trm.lib().bartrt_get_prep_shape(C.byref(m), C.byref(c)))
    L = nlayers()
    coef = np.zeros((L, 4 + 2 * m.value + 2 * c.value))
    idx = np.zeros((L, 1 + c.value), np.int64)
    kstop = np.zeros(1, np.int32)
    ok = np.zeros(1, np.uint8)
    _check(trm.lib().bartrt_get_prep_records(int(walker), _ptr(coef), _ptr(idx), _ptr(kstop), _ptr(ok)))
    return coef, idx, int(kstop[0]), int(ok[0])


def chord_table(walker: int):
    """The transit geometry's radii and chord table as the latest launch's preparation wrote them for one walker of
    its batch (diagnostics; include/bartrt.h, bartrt_get_chord_table): (rtop[L], ds[L, L], raw[nkt, 4 nkt, 64]) --
    the radii top to bottom, ds[k, j] = s_{j-1} - s_j of chord k in layer j (zero for j = 0 and j > k), and the table
    as it lies in memory (row tile, step, lane; nkt = ceil(L / 16)).  Raises on an eclipse engine and for a walker
    outside the batch."""
    L = nlayers()
    nkt = (L + 15) // 16
    rtop, ds, raw = np.zeros(L), np.zeros((L, L)), np.zeros((nkt, 4 * nkt, 64))
    _check(trm.lib().bartrt_get_chord_table(int(walker), _ptr(rtop), _ptr(ds), _ptr(raw)))
    return rtop, ds, raw


def lbl_extinction(profile: np.ndarray) -> np.ndarray:
    """Line-by-line extinction [L, W_local] (cm-1, atm layer order) of one profile."""
    prof = np.ascontiguousarray(profile, np.double).ravel()
    lo, hi = local_range()
    ext = np.zeros((nlayers(), hi - lo))
    _check(trm.lib().bartrt_get_lbl_extinction(_ptr(prof), prof.size, _ptr(ext), ext.shape[0],
                                               ext.shape[1]))
    return ext


def lbl_owners(profile: np.ndarray) -> np.ndarray:
    """Which accumulation kernel writes each (layer state, 256-point tile) of `lbl_extinction(profile)`:
    uint8 [L, ntile], by the device's own rule on the state vectors the accumulation reads (diagnostics;
    the codes are listed in include/bartrt.h, bartrt_lbl_owners)."""
    prof = np.ascontiguousarray(profile, np.double).ravel()
    lo, hi = local_range()
    own = np.zeros((nlayers(), (hi - lo + 255) // 256), np.uint8)
    _check(trm.lib().bartrt_lbl_owners(_ptr(prof), prof.size, _ptr(own), own.shape[0], own.shape[1]))
    return own


def lbl_states(profile: np.ndarray | None = None) -> dict:
    """The state vectors the accumulation kernels read (diagnostics; include/bartrt.h, bartrt_lbl_get_states): what
    lbl_states and lbl_smax wrote for `lbl_extinction(profile)`, which is run first -- or, with no profile, for the
    latest line-by-line call as it stands (a batch, the opacity-grid generator's last slab).  A dict of T[nstate],
    dv[nstate] (int), dop[nstate, niso], lor[nstate, niso], scale[nstate, niso] (SIGCTE * scale) and
    smax[nstate, ngroup]."""
    if profile is not None:
        lbl_extinction(profile)
    ns, ni, ng = C.c_int(), C.c_int(), C.c_int()
    _check(trm.lib().bartrt_lbl_get_states(C.byref(ns), C.byref(ni), C.byref(ng), None, None))
    state = np.zeros((ns.value, 2 + 3 * ni.value))
    smax = np.zeros((ns.value, ng.value))
    _check(trm.lib().bartrt_lbl_get_states(C.byref(ns), C.byref(ni), C.byref(ng), _ptr(state), _ptr(smax)))
    per = state[:, 2:].reshape(ns.value, ni.value, 3)
    return dict(T=state[:, 0].copy(), dv=state[:, 1].astype(int), dop=per[:, :, 0].copy(), lor=per[:, :, 1].copy(),
                scale=per[:, :, 2].copy(), smax=smax)


def voigt(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """Re w(x + i y) as the line-by-line kernels evaluate it (diagnostics; no engine needed)."""
    x, y = np.broadcast_arrays(np.asarray(x, np.double), np.asarray(y, np.double))
    xs, ys = np.ascontiguousarray(x).ravel(), np.ascontiguousarray(y).ravel()
    k = np.empty_like(xs)
    _check(trm.lib().bartrt_voigt(_ptr(xs), _ptr(ys), _ptr(k), xs.size))
    return k.reshape(x.shape)


def expint_e2(x: np.ndarray) -> np.ndarray:
    """E_2(x) as the "line" T(p) model's kernels evaluate it (diagnostics; no engine needed)."""
    x = np.asarray(x, np.double)
    xs = np.ascontiguousarray(x).ravel()
    out = np.empty_like(xs)
    _check(trm.lib().bartrt_expint_e2(_ptr(xs), _ptr(out), xs.size))
    return out.reshape(x.shape)


# the selectors of bartrt_rt_math (include/bartrt.h, BARTRT_RT_MATH_*)
RT_MATH = {"exp_rt": 0, "exp_rt_n4": 1, "exp_rt_fma3": 2, "exp_core": 3, "rcp_core": 4, "rcp_n1": 5, "rcp_raw": 6,
           "planck_inv": 7, "alive_flags": 8}


def rt_math(name: str, x: np.ndarray) -> np.ndarray:
    """One of the RT kernels' elementary functions (a key of RT_MATH) as the device evaluates it (diagnostics; no
    engine needed).  The arguments are not checked: the exponentials take -708 .. 700 (exp_core: 709), the
    reciprocals normal positive numbers."""
    if name not in RT_MATH:
        raise ValueError("rt_math: %r is not one of %s" % (name, ", ".join(RT_MATH)))
    x = np.asarray(x, np.double)
    xs = np.ascontiguousarray(x).ravel()
    out = np.empty_like(xs)
    _check(trm.lib().bartrt_rt_math(RT_MATH[name], _ptr(xs), _ptr(out), xs.size))
    return out.reshape(x.shape)


def alive_flags(tm: np.ndarray, thr: np.ndarray) -> np.ndarray:
    """The ray flag of rule 1's `cut slant` kernel (csrc/rt_eclipse_s1s.hpp alive_flags) for pairs of a running
    optical depth and a ray's threshold, as the device evaluates it: 1.0 where the ray is alive (diagnostics; no
    engine needed; include/bartrt.h, BARTRT_RT_MATH_ALIVE_FLAGS)."""
    tm, thr = np.broadcast_arrays(np.asarray(tm, np.double), np.asarray(thr, np.double))
    pairs = np.ascontiguousarray(np.stack([tm.ravel(), thr.ravel()], axis=1))
    return rt_math("alive_flags", pairs).ravel()[:tm.size].reshape(tm.shape)


def slant_thresholds(toomuch: float, invmu: np.ndarray):
    """(thr, thrb) of `cut slant` for the rays' 1 / cos(theta), as the host forms them for a launch (no GPU, no engine;
    include/bartrt.h, bartrt_slant_thresholds)."""
    im = np.ascontiguousarray(invmu, np.double).ravel()
    thr, thrb = np.zeros(im.size), np.zeros(im.size)
    _check(trm.lib().bartrt_slant_thresholds(float(toomuch), _ptr(im), im.size, _ptr(thr), _ptr(thrb)))
    return thr, thrb


def ray_args() -> dict:
    """The ray quadrature of the initialised eclipse engine as its launches carry it (diagnostics; include/bartrt.h,
    bartrt_get_ray_args): invmu, wgt, wq, thr, thrb in the order of the raygrid, `order` (the ray in each slot of the
    specialised kernels' order) and `sq` (that order is the square-root one: the last slot's transmittance is the
    square of the first's)."""
    n = trm.lib().bartrt_get_nangles()
    out = {k: np.zeros(n) for k in ("invmu", "wgt", "wq", "thr", "thrb")}
    order, sq = np.zeros(n, np.int32), C.c_int()
    _check(trm.lib().bartrt_get_ray_args(n, *[_ptr(out[k]) for k in ("invmu", "wgt", "wq", "thr", "thrb")], _ptr(order),
                                         C.byref(sq)))
    out["order"], out["sq"] = order, bool(sq.value)
    return out


# ---- device-resident (torch tensors own the memory) ----------------------
def _stream_ptr(stream=None):
    """The HIP stream the library is to enqueue on: torch's current stream.  torch's DEFAULT stream
    is the null stream (handle 0), which the C ABI reads as "the engine's own stream"
    (include/bartrt.h) -- a different, non-blocking stream that torch's next operation (a clone, a
    collective) would not wait for.  The default stream therefore travels as hipStreamLegacy (1),
    HIP's explicit handle for it."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream or 1)


def run_batch_dev(d_prof, d_spec=None, stream=None, next_prof=None):
    """d_prof: float64 CUDA tensor [nwalkers, (S+1)*L]; returns [nwalkers, W_local]
    on the same device.  Asynchronous on torch's current stream.

    ``next_prof``: the batch of the NEXT call, if it is known and already complete in HBM
    (include/bartrt.h, bartrt_prefetch_profiles_dev): this call's RT launch prepares its layer
    records on the side and the next call skips its preparation launch.  Bit-identical results."""
    import torch
    assert d_prof.is_cuda and d_prof.dtype == torch.float64 and d_prof.is_contiguous()
    n = d_prof.shape[0]
    if next_prof is not None:
        assert next_prof.is_cuda and next_prof.dtype == torch.float64 and next_prof.is_contiguous()
        _check(trm.lib().bartrt_prefetch_profiles_dev(C.c_void_p(next_prof.data_ptr()), next_prof.shape[0]))
    lo, hi = local_range()
    if d_spec is None:
        d_spec = torch.empty((n, hi - lo), dtype=torch.float64, device=d_prof.device)
    _check(trm.lib().bartrt_run_transit_batch_dev(
        C.c_void_p(d_prof.data_ptr()), n, C.c_void_p(d_spec.data_ptr()), None,
        _stream_ptr(stream)))
    return d_spec


def run_batch_sharded(d_prof, group=None, force=False):
    """Every rank holds one wavenumber block of the tables and the full (tiny)
    profile batch; each computes spec[nwalkers, W/G] and one RCCL all-gather
    reassembles spec[nwalkers, W] on every rank.  A group of one
    skips the collective unless ``force`` (the single-GPU test of the RCCL path)."""
    import torch.distributed as dist
    local = run_batch_dev(d_prof)
    world = dist.get_world_size(group)
    if world == 1 and not force:
        return local
    return allgather_blocks(local, group, total=trm.get_no_samples())


def block_sizes(total, world):
    """Samples per rank under the engine's integer split (Engine::setup): W*(r+1)//n - W*r//n."""
    return [total * (r + 1) // world - total * r // world for r in range(world)]


def pad_block(local, wmax):
    """A rank's block [n, W_r] as the all-gather sends it: [n, wmax], zero-padded on the right."""
    import torch
    if local.shape[1] == wmax:
        return local.contiguous()
    send = torch.zeros((local.shape[0], wmax), dtype=local.dtype, device=local.device)
    send[:, :local.shape[1]] = local
    return send


def reassemble_blocks(out, n, sizes):
    """The all-gather's receive buffer [world * n, wmax] (rank-major) -> spectra [n, sum(sizes)]."""
    import torch
    world, wmax = len(sizes), out.shape[1]
    o = out.view(world, n, wmax)
    if min(sizes) == wmax:
        return o.permute(1, 0, 2).reshape(n, world * wmax)
    return torch.cat([o[r, :, :sizes[r]] for r in range(world)], dim=1)


def allgather_blocks(local, group=None, total=None, async_op=False, out=None):
    """local [n, W_r] on rank r (block sizes may differ by one sample) ->
    [n, sum_r W_r] on every rank.  With ``total`` (the full sample count) the
    block sizes follow from the engine's integer split W*r//n and ONE collective
    per call is issued; without it the sizes are exchanged first.

    ``async_op=True`` returns ``(work, finish)``: the collective is enqueued on
    RCCL's stream behind the kernels already queued on the current stream, the
    current stream is NOT made to wait, and ``finish()`` (wait + reassembly) is
    called when the spectra are needed -- so the next batch's kernels overlap
    the xGMI traffic of this one.  ``out`` may supply the [world*n, wmax]
    receive buffer (double buffering)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    n = local.shape[0]
    if total is not None:
        sizes = block_sizes(total, world)
        assert sizes[dist.get_rank(group)] == local.shape[1]
    else:
        sizes = [torch.zeros(1, dtype=torch.int64, device=local.device) for _ in range(world)]
        dist.all_gather(sizes, torch.tensor([local.shape[1]], dtype=torch.int64,
                                            device=local.device), group=group)
        sizes = [int(s.item()) for s in sizes]
    wmax = max(sizes)
    send = pad_block(local, wmax)
    if out is None:
        out = torch.empty((world * n, wmax), dtype=local.dtype, device=local.device)
    if local.is_cuda and dist.get_backend(group) == "gloo":
        # Device blocks under a process group that moves host memory only (two ranks on ONE GPU, which RCCL
        # refuses -- tests/test_gpu_two_ranks.py; a node without xGMI): the block goes through pinned host memory.
        # The collective must not start before the kernels that write `local` have finished: the stream is waited
        # for here (RCCL orders that on the device; gloo cannot).
        h_send = torch.empty(send.shape, dtype=send.dtype, pin_memory=True)
        h_send.copy_(send, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        h_out = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
        hwork = dist.all_gather_into_tensor(h_out, h_send, group=group, async_op=async_op)

        def finish_host():
            if hwork is not None:
                hwork.wait()
            out.copy_(h_out, non_blocking=True)      # on the current stream, ahead of the reassembly
            return reassemble_blocks(out, n, sizes)

        return (hwork, finish_host) if async_op else finish_host()
    work = dist.all_gather_into_tensor(out, send, group=group, async_op=async_op)

    def finish():
        if work is not None:
            work.wait()                      # the current stream waits; the host does not
        return reassemble_blocks(out, n, sizes)

    return (work, finish) if async_op else finish()


class GatherPipeline:
    """Bucketed, double-buffered all-gather of per-step wavenumber blocks.

    Each step writes its local block spec[nwalkers, W_r] into ``slot(i)``; every
    ``group`` steps one collective carries the whole bucket (fewer, larger
    transfers over xGMI, and one cross-stream wait per bucket instead of one per
    step on the compute stream), issued asynchronously on RCCL's stream while the
    next bucket's kernels run.  ``submit(i)`` returns the reassembled spectra
    [steps, nwalkers, W] of the bucket whose buffers step i+1 is about to reuse (or
    None); ``drain()`` flushes what is still in flight."""

    def __init__(self, nwalkers, wlocal, total, steps_per_bucket, device, pg=None, dtype=None):
        import torch
        import torch.distributed as dist
        self.n, self.wl, self.total, self.G, self.pg = nwalkers, wlocal, total, max(1, steps_per_bucket), pg
        world = dist.get_world_size(pg)
        wmax = max(block_sizes(total, world))
        dtype = dtype or torch.float64
        self.local = [torch.empty((self.G, nwalkers, wlocal), dtype=dtype, device=device) for _ in range(2)]
        self.recv = [torch.empty((world * self.G * nwalkers, wmax), dtype=dtype, device=device) for _ in range(2)]
        self.pending = [None, None]      # per buffer: (finish, steps it holds)
        self.filled = 0                  # steps written into the open bucket

    def slot(self, i):
        """Where step i's kernels write; first finishes the bucket that used these buffers."""
        b, k = (i // self.G) & 1, i % self.G
        done = None
        if k == 0:
            done = self._finish(b)
        self._done = done
        return self.local[b][k]

    def submit(self, i):
        b, k = (i // self.G) & 1, i % self.G
        self.filled = k + 1
        if k == self.G - 1:
            self._issue(b)
        return self._done

    def _issue(self, b):
        k = self.filled                  # a partly filled bucket (drain) sends its filled steps only
        world = self.recv[b].shape[0] // (self.G * self.n)
        _, fin = allgather_blocks(self.local[b][:k].view(k * self.n, self.wl), self.pg, total=self.total,
                                  async_op=True, out=self.recv[b][:world * k * self.n])
        self.pending[b] = (fin, k)
        self.filled = 0

    def _finish(self, b):
        if self.pending[b] is None:
            return None
        fin, k = self.pending[b]
        self.pending[b] = None
        return fin().view(k, self.n, self.total)

    def drain(self, last_step):
        """After the last submit(last_step): returns the remaining buckets in step order."""
        b = (last_step // self.G) & 1
        if self.filled:
            self._issue(b)
        outs = [self._finish(1 - b), self._finish(b)]
        return [o for o in outs if o is not None]


# ---- per-step converters --------------------------------------------------
def step_setup(ptargs5, tmin, tmax, abund, imol, idx0, npts, nifilter, istarfl,
               rprs, solution=0, pttype=0, tint_thorngren=False):
    a = lambda x, t: np.ascontiguousarray(x, t)
    ptargs5 = a(ptargs5 if ptargs5 is not None else np.zeros(5), np.double)
    abund = a(abund, np.double)
    imol = a(imol, np.int32)
    idx0 = a(idx0, np.int32)
    npts = a(npts, np.int32)
    nif = a(nifilter, np.double)
    star = a(istarfl, np.double) if istarfl is not None else None
    _check(trm.lib().bartrt_step_setup(
        _ptr(ptargs5), int(bool(tint_thorngren)), int(pttype), float(tmin), float(tmax),
        _ptr(abund), imol.size, _ptr(imol), idx0.size, _ptr(idx0), _ptr(npts), _ptr(nif),
        _ptr(star) if star is not None else None, float(rprs), int(solution)))


def step_set_extras(nrad: int, ncloud: int, nray: int) -> None:
    """Radius / cloud-top / scattering parameters (0 or 1 each) sit between the T(p)
    parameters and the abundance factors of every walker (BARTfunc.py:350-360)."""
    _check(trm.lib().bartrt_step_set_extras(int(nrad), int(ncloud), int(nray)))


def step_set_carry(on: bool) -> None:
    """The reference's carry-over of the previous temperature profile when the T(p)
    model raises ValueError (BARTfunc.py:318-324); walker w of every batch = chain w."""
    _check(trm.lib().bartrt_step_set_carry(int(bool(on))))


def step_set_ebalance(on, e_in, e_fac):
    _check(trm.lib().bartrt_step_set_ebalance(int(bool(on)), float(e_in), float(e_fac)))


def step_batch(params: np.ndarray, nfilters: int):
    p = np.ascontiguousarray(params, np.double)
    p = p.reshape(-1, p.shape[-1])
    band = np.zeros((p.shape[0], nfilters))
    status = np.zeros(p.shape[0], np.int32)
    _check(trm.lib().bartrt_step_batch(_ptr(p), p.shape[0], p.shape[1], _ptr(band), _ptr(status)))
    return band, status


def step_batch_dev(d_params, nfilters, want_spec=False, stream=None):
    import torch
    n, npars = d_params.shape
    dev = d_params.device
    band = torch.empty((n, nfilters), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    spec = None
    if want_spec:
        spec = torch.empty((n, trm.get_no_samples()), dtype=torch.float64, device=dev)
    _check(trm.lib().bartrt_step_batch_dev(
        C.c_void_p(d_params.data_ptr()), n, npars, C.c_void_p(band.data_ptr()),
        C.c_void_p(status.data_ptr()), C.c_void_p(spec.data_ptr()) if want_spec else None,
        _stream_ptr(stream)))
    return (band, status, spec) if want_spec else (band, status)


def step_profiles_dev(d_params, stream=None):
    """Profiles [n, (S+1)*L] and status [n] of parameter vectors [n, npars] on the device (after step_setup;
    include/bartrt.h, bartrt_step_profiles_dev): the input of run_batch_dev / contribution_dev."""
    import torch
    n, npars = d_params.shape
    prof = torch.empty((n, nprof()), dtype=torch.float64, device=d_params.device)
    status = torch.empty(n, dtype=torch.int32, device=d_params.device)
    _check(trm.lib().bartrt_step_profiles_dev(
        C.c_void_p(d_params.data_ptr()), n, npars, C.c_void_p(prof.data_ptr()),
        C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
    return prof, status


def step_batch_sharded(d_params, nfilters, group=None, stream=None, force=False):
    """Per-step callable on a wavenumber-sharded node: profiles on every rank,
    RT on the local block, all-gather, band integration on the full grid.
    ``force``: issue the collective on a group of one too (run_batch_sharded)."""
    import torch
    n, npars = d_params.shape
    dev = d_params.device
    prof = torch.empty((n, nprof()), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _check(trm.lib().bartrt_step_profiles_dev(
        C.c_void_p(d_params.data_ptr()), n, npars, C.c_void_p(prof.data_ptr()),
        C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
    spec = run_batch_sharded(prof, group, force=force)
    band = torch.empty((n, nfilters), dtype=torch.float64, device=dev)
    _check(trm.lib().bartrt_step_bandflux_dev(
        C.c_void_p(spec.data_ptr()), n, C.c_void_p(status.data_ptr()),
        C.c_void_p(band.data_ptr()), _stream_ptr(stream)))
    return band, status, spec


def step_bandflux_blocks_dev(d_blocks, nranks, d_status, nfilters, stream=None):
    """Band fluxes [n, nfilters] of the ranks' blocks where an all-gather leaves them: d_blocks a float64 CUDA tensor
    of nranks slots of n * max(block_sizes) doubles, slot r = [n, W_r] packed rows of block r (include/bartrt.h,
    bartrt_step_bandflux_blocks_dev).  d_status (int32 [n], from step_profiles_dev) may be set to 3 (energy balance).
    The same bits as the band integration of the reassembled spectra."""
    import torch
    assert d_blocks.is_cuda and d_blocks.dtype == torch.float64 and d_blocks.is_contiguous()
    assert d_status.is_cuda and d_status.dtype == torch.int32
    n = d_status.shape[0]
    assert d_blocks.numel() >= nranks * n * max(block_sizes(trm.get_no_samples(), nranks))
    band = torch.empty((n, nfilters), dtype=torch.float64, device=d_blocks.device)
    _check(trm.lib().bartrt_step_bandflux_blocks_dev(
        C.c_void_p(d_blocks.data_ptr()), int(nranks), n, C.c_void_p(d_status.data_ptr()),
        C.c_void_p(band.data_ptr()), _stream_ptr(stream)))
    return band


# ---- the library's own communicator (include/bartrt.h, bartrt_comm_*) -------
COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """Rank 0's part of the bring-up: the id every rank passes to comm_attach."""
    buf = (C.c_char * COMM_ID_BYTES)()
    _check(trm.lib().bartrt_comm_get_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


def comm_attach(uid: bytes, rank: int, nranks: int) -> None:
    """Every rank, its engine initialised with --shard rank nranks (unsharded: 0 / 1), attaches the communicator
    named by rank 0's id (a launcher of its own -- MPI, a file -- hands the bytes over)."""
    assert len(uid) == COMM_ID_BYTES
    buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(uid)
    _check(trm.lib().bartrt_comm_init(C.cast(buf, C.c_void_p), int(rank), int(nranks)))


def comm_init(group=None) -> None:
    """Attaches the library's communicator over the ranks of a torch process group (gloo or nccl): rank 0 makes the
    id, one broadcast over the group hands its 128 bytes to the others, every rank attaches.  The group's ranks must be
    the engine's --shard ranks.  Afterwards step_batch / step_batch_dev / sampler.run_native run on the sharded engine
    with one collective per step, inside the library, and so do cf_setup, contribution* and transmittance* (one
    collective per chunk of walkers)."""
    import torch
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    uid = comm_unique_id() if rank == 0 else bytes(COMM_ID_BYTES)
    t = torch.tensor(list(uid), dtype=torch.uint8)
    if dist.get_backend(group) == "nccl":
        t = t.cuda()
    src = dist.get_global_rank(group, 0) if group is not None else 0
    dist.broadcast(t, src=src, group=group)
    comm_attach(bytes(t.cpu().tolist()), rank, world)


def comm_free() -> None:
    _check(trm.lib().bartrt_comm_free())


def comm_info() -> dict:
    """-> dict(rank, nranks, ncollectives): the attached communicator (rank -1, nranks 0 without one) and the
    collectives the engine has issued."""
    r, n, k = C.c_int(0), C.c_int(0), C.c_ulonglong(0)
    _check(trm.lib().bartrt_get_comm(C.byref(r), C.byref(n), C.byref(k)))
    return {"rank": r.value, "nranks": n.value, "ncollectives": k.value}


def timing_begin(stride: int = 1):
    """HIP events around every `stride`-th RT launch until timing_end()."""
    _check(trm.lib().bartrt_timing_begin_sampled(int(stride)))


def timing_end():
    ms, n = C.c_double(), C.c_int()
    _check(trm.lib().bartrt_timing_end(C.byref(ms), C.byref(n)))
    return ms.value, n.value


def walked_begin():
    """Record, for the eclipse launches that follow, how many layers each wave walks (transit launches: the kernel
    name only)."""
    _check(trm.lib().bartrt_walked_begin())


def walked_end():
    """-> (walked[nwalkers, ncolumns], wavenumbers per column, kernel name) of the last launch."""
    n, nc, wpc = C.c_int(), C.c_int(), C.c_int()
    name = C.create_string_buffer(256)   # (the name and its notes)
    _check(trm.lib().bartrt_walked_end(None, 0, C.byref(n), C.byref(nc), C.byref(wpc), name, 256))
    # the record itself (the first call switched recording off; the buffer stays)
    out = np.zeros((n.value, nc.value), np.int32)
    if out.size:
        _check(trm.lib().bartrt_walked_end(_ptr(out), out.size, C.byref(n), C.byref(nc), C.byref(wpc), name, 256))
    return out, wpc.value, name.value.decode()


def walked_restarts():
    """-> restarts[nwalkers] of the record walked_end() returned: the waves of each walker that walked their column
    a second time (the optimistic loop of the single-wave `cut slant` kernel, trm.set_slant_opt)."""
    n = C.c_int()
    _check(trm.lib().bartrt_walked_restarts(None, 0, C.byref(n)))
    out = np.zeros(n.value, np.int32)
    if out.size:
        _check(trm.lib().bartrt_walked_restarts(_ptr(out), out.size, C.byref(n)))
    return out


def kernel_inventory() -> list[tuple[str, bool, str]]:
    """The eclipse kernels the library holds ahead of time: (template-id, max-ILP run-time build, object) each.  No GPU,
    no engine."""
    buf = C.create_string_buffer(1 << 18)
    _check(trm.lib().bartrt_kernel_inventory(buf, len(buf)))
    return [(e, i == "1", o) for e, i, o in (line.split("\t") for line in buf.value.decode().splitlines())]


def algorithmic_bytes(nwalkers: int) -> float:
    return trm.lib().bartrt_algorithmic_bytes(int(nwalkers))


# ---- contribution functions / band transmittance (include/bartrt.h, bartrt_cf_*) --------------
CF_CONTRIB, CF_TRANSMIT = 0, 1
_cf_nfilters = 0     # filters of the latest cf_setup (the band tensors' middle axis)


def _cf_wlocal() -> int:
    """Rows of a walker's ``full`` output: the engine's own samples (the whole grid unless sharded)."""
    lo, hi = local_range()
    return hi - lo


def cf_setup(filters, block=False) -> int:
    """The filter windows of the batched contribution-function calls: a list of filter files (read and
    windowed on the engine's FULL grid by bart_amd.cf.filter_windows) or the (idx0, npts, resp, trapz) that
    function returns.  Kept by the engine until the next cf_setup / init / free_memory.  -> nfilters.
    A sharded engine takes it after comm_init (every rank the same windows); ``block`` (cf_setup_block): the same
    tables for the engine's block without a communicator, for cf_partials_dev / cf_combine_dev."""
    if isinstance(filters, tuple) and len(filters) == 4 and not isinstance(filters[0], (str, bytes, os.PathLike)):
        idx0, npts, resp, _ = filters
    else:
        from .cf import filter_windows
        idx0, npts, resp, _ = filter_windows(trm.get_waveno_arr(trm.get_no_samples()), list(filters))
    idx0, npts = np.ascontiguousarray(idx0, np.int32), np.ascontiguousarray(npts, np.int32)
    resp = np.ascontiguousarray(resp, np.double)
    assert idx0.size == npts.size and resp.size == int(npts.sum())
    global _cf_nfilters
    setup = trm.lib().bartrt_cf_setup_block if block else trm.lib().bartrt_cf_setup
    _check(setup(idx0.size, _ptr(idx0), _ptr(npts), _ptr(resp)))
    _cf_nfilters = int(idx0.size)
    return _cf_nfilters


def cf_setup_block(filters) -> int:
    """cf_setup on any engine, sharded or not, with no communicator (include/bartrt.h, bartrt_cf_setup_block): the
    windows, stated on the full grid, are clipped to the engine's block.  For cf_partials_dev / cf_combine_dev."""
    return cf_setup(filters, block=True)


def cf_partials_dev(d_prof, kind, full=False, d_ok=None, stream=None, over=None):
    """This engine's part of the band sums (bartrt_cf_partials_dev) for the filters of the latest cf_setup /
    cf_setup_block: d_prof a float64 CUDA tensor [nwalkers, (S+1)*L], kind CF_CONTRIB / CF_TRANSMIT -> part
    [nwalkers, nfilters, L] (layers from the top, not divided: one slot of cf_combine_dev), and with ``full`` the
    block's own per-wavenumber values [nwalkers, W_local, L] (atm layer order).  d_ok, over as contribution_dev."""
    import torch
    assert d_prof.is_cuda and d_prof.dtype == torch.float64 and d_prof.is_contiguous()
    n = d_prof.shape[0]
    part, fout = _cf_dev_outputs(n, full, d_prof.device)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    if d_ok is not None:
        assert d_ok.is_cuda and d_ok.dtype == torch.uint8 and d_ok.numel() >= n
    if over is not None:
        assert over.is_cuda and over.dtype == torch.float64 and over.is_contiguous() and tuple(over.shape) == (n, 3)
    _check(trm.lib().bartrt_cf_partials_dev(vp(d_prof), n, int(kind), vp(over), vp(part), vp(fout), vp(d_ok),
                                            _stream_ptr(stream)))
    return (part, fout) if full else part


def cf_combine_dev(d_slots, nranks, d_ok=None, stream=None):
    """The ranks' parts where an all-gather leaves them -> band rows (bartrt_cf_combine_dev): d_slots a float64 CUDA
    tensor of nranks slots [nwalkers, nfilters, L] (slot r = rank r's cf_partials_dev), added in rank order, divided by
    trapz(resp), atm layer order -> [nwalkers, nfilters, L]; NaN rows where d_ok (uint8 [nwalkers]) is 0."""
    import torch
    assert d_slots.is_cuda and d_slots.dtype == torch.float64 and d_slots.is_contiguous()
    per = _cf_nfilters * nlayers()
    assert _cf_nfilters and nranks >= 1 and d_slots.numel() % (nranks * per) == 0
    n = d_slots.numel() // (nranks * per)
    if d_ok is not None:
        assert d_ok.is_cuda and d_ok.dtype == torch.uint8 and d_ok.numel() >= n
    band = torch.empty((n, _cf_nfilters, nlayers()), dtype=torch.float64, device=d_slots.device)
    _check(trm.lib().bartrt_cf_combine_dev(
        C.c_void_p(d_slots.data_ptr()), int(nranks), n, C.c_void_p(d_ok.data_ptr()) if d_ok is not None else None,
        C.c_void_p(band.data_ptr()), _stream_ptr(stream)))
    return band


CF_KERNELS = ("cf_eclipse", "cf_transit<staged>", "cf_transit<unstaged>")


class _CfRecords(C.Structure):
    """include/bartrt.h, bartrt_cf_records."""
    _fields_ = ([(k, C.c_int) for k in ("nlayers", "nmol", "ncs", "transit", "nwalkers", "nfilters", "ntiles", "nent", "kernel",
                                        "kstop", "ok")] + [("lds_bytes", C.c_longlong)] +
                [(k, C.c_void_p) for k in ("coef", "idx", "rdlp", "rtop", "ds", "tile_ptr", "wt", "f_ptr", "f_ent", "trapz")])


def cf_launch():
    """The shapes of the latest cf_setup and the CF kernel of the latest launch, a refused one included (diagnostics;
    include/bartrt.h, bartrt_cf_get_records with no buffers): dict(nwalkers, nfilters, ntiles, nent, kernel, lds_bytes,
    nmol, ncs, transit) -- kernel one of CF_KERNELS, nmol / ncs the engine's M and C, transit True on a transit
    engine; nwalkers = 0 when no chunk has run since the setup."""
    r = _CfRecords()
    _check(trm.lib().bartrt_cf_get_records(-1, C.byref(r)))
    return {"nwalkers": r.nwalkers, "nfilters": r.nfilters, "ntiles": r.ntiles, "nent": r.nent,
            "kernel": CF_KERNELS[r.kernel], "lds_bytes": int(r.lds_bytes), "nmol": r.nmol, "ncs": r.ncs, "transit": bool(r.transit)}


def cf_records(walker: int):
    """What the CF kernel of the latest contribution / transmittance call read for one walker of its last chunk, and
    the filter tables of the latest cf_setup (diagnostics; include/bartrt.h, bartrt_cf_get_records): a dict of
    coef[L, 4 + 2 M + 2 C], idx[L, 1 + C], kstop, ok, rdlp[L] (layers from the top), on a transit engine rtop[L] and
    ds[L, L] as chord_table gives them, tile_ptr[ntiles + 1], wt[nent, 64], f_ptr[nf + 1], f_ent[nent], trapz[nf],
    and cf_launch()'s entries.  Raises without a setup, without a call since it, and for a walker outside the chunk."""
    out = cf_launch()
    L = nlayers()
    a = {"coef": np.zeros((L, 4 + 2 * out["nmol"] + 2 * out["ncs"])), "idx": np.zeros((L, 1 + out["ncs"]), np.int64),
         "rdlp": np.zeros(L), "tile_ptr": np.zeros(out["ntiles"] + 1, np.int32), "wt": np.zeros((out["nent"], 64)),
         "f_ptr": np.zeros(out["nfilters"] + 1, np.int32), "f_ent": np.zeros(out["nent"], np.int32),
         "trapz": np.zeros(out["nfilters"])}
    if out["transit"]:
        a["rtop"], a["ds"] = np.zeros(L), np.zeros((L, L))
    r = _CfRecords()
    for k, v in a.items():
        setattr(r, k, v.ctypes.data)
    _check(trm.lib().bartrt_cf_get_records(int(walker), C.byref(r)))
    out.update(a)
    out.update(kstop=r.kstop, ok=r.ok, nwalkers=r.nwalkers)
    return out


def _cf_over(over, n):
    """over [nwalkers, 3] = (radius km, log10 cloud-top bar, Rayleigh value) per walker, NaN = the engine-wide
    setting (include/bartrt.h, bartrt_cf_batch_over) -> contiguous float64 [n, 3]."""
    o = np.ascontiguousarray(over, np.double)
    if o.shape != (n, 3):
        raise ValueError("over must have shape (nwalkers, 3) = (%d, 3), not %s" % (n, o.shape))
    return o


def _cf_batch(profiles, filters, kind, full, want_ok, over=None):
    prof = np.ascontiguousarray(profiles, np.double).reshape(-1, nprof())
    nf = cf_setup(filters)
    n, L, W = prof.shape[0], nlayers(), _cf_wlocal()
    band = np.zeros((n, nf, L))
    fout = np.zeros((n, W, L)) if full else None
    ok = np.zeros(n, np.uint8)
    pover = None if over is None else _ptr(_cf_over(over, n))    # (null: the plain call)
    _check(trm.lib().bartrt_cf_batch_over(_ptr(prof), n, prof.shape[1], pover, kind, _ptr(band),
                                          _ptr(fout) if full else None, _ptr(ok) if want_ok else None))
    return band, fout, ok


def contribution(profiles, filters, normalize=True, full=False, want_ok=False, over=None):
    """Band-averaged contribution functions of a batch (cf.cf's result per walker; eclipse geometry):
    profiles [nwalkers, (S+1)*L] as run_batch, filters as cf_setup ->
    filt_cf [nwalkers, nfilters, L] in atm layer order, then (normalize) filt_cf_norm of the same shape,
    then (full) the per-wavenumber values [nwalkers, W, L], then (want_ok) the walkers' flags -- without
    want_ok a non-finite profile raises; with it, that walker's rows are NaN.  A single array is returned
    bare, several as a tuple.  ``over`` [nwalkers, 3]: every walker's own reference radius (km), log10 cloud-top
    pressure (bar) and Rayleigh value, NaN = the engine-wide setting (bartrt_cf_batch_over).
    On a sharded engine after comm_init every rank makes the same call and gets the same band rows; ``filters`` are
    windows on the full grid and the per-wavenumber values are the rank's own block [nwalkers, W_local, L]."""
    from .cf import normalize as _norm
    band, fout, ok = _cf_batch(profiles, filters, CF_CONTRIB, full, want_ok, over)
    out = [band] + ([_norm(band)] if normalize else []) + ([fout] if full else []) + ([ok] if want_ok else [])
    return out[0] if len(out) == 1 else tuple(out)


def transmittance(profiles, filters, full=False, want_ok=False, over=None):
    """Band-averaged transmittance exp(-tau) of a batch (cf.transmittance's result per walker; vertical depth
    on an eclipse engine, chord depth on a transit engine): [nwalkers, nfilters, L] in atm layer order,
    then (full) [nwalkers, W, L], then (want_ok) the flags, as contribution(); ``over`` as there."""
    band, fout, ok = _cf_batch(profiles, filters, CF_TRANSMIT, full, want_ok, over)
    out = [band] + ([fout] if full else []) + ([ok] if want_ok else [])
    return out[0] if len(out) == 1 else tuple(out)


def _cf_dev_outputs(n, full, device):
    import torch
    if not _cf_nfilters:
        raise trm.TransitError("the device forms of the contribution-function calls: call engine.cf_setup(filters) first")
    band = torch.empty((n, _cf_nfilters, nlayers()), dtype=torch.float64, device=device)
    fout = torch.empty((n, _cf_wlocal(), nlayers()), dtype=torch.float64, device=device) if full else None
    return band, fout


def _cf_batch_dev(d_prof, kind, full, d_ok, stream, d_over=None):
    import torch
    assert d_prof.is_cuda and d_prof.dtype == torch.float64 and d_prof.is_contiguous()
    n = d_prof.shape[0]
    band, fout = _cf_dev_outputs(n, full, d_prof.device)
    if d_ok is not None:
        assert d_ok.is_cuda and d_ok.dtype == torch.uint8 and d_ok.numel() >= n
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    if d_over is not None:
        assert d_over.is_cuda and d_over.dtype == torch.float64 and d_over.is_contiguous() and tuple(d_over.shape) == (n, 3)
    _check(trm.lib().bartrt_cf_batch_over_dev(vp(d_prof), n, vp(d_over), kind, vp(band), vp(fout), vp(d_ok),
                                              _stream_ptr(stream)))
    return (band, fout) if full else band


def contribution_dev(d_prof, full=False, d_ok=None, stream=None, over=None):
    """Device form of contribution() for the filters of the latest cf_setup: d_prof a float64 CUDA tensor
    [nwalkers, (S+1)*L] (run_batch_dev's input, e.g. from bartrt_step_profiles_dev) -> band tensor
    [nwalkers, nfilters, L] (atm layer order; not normalised), and [nwalkers, W, L] with ``full``.
    Asynchronous on torch's current stream; d_ok (uint8 [nwalkers]) receives the flags (flagged rows: NaN);
    ``over``: a float64 CUDA tensor [nwalkers, 3] as contribution()'s."""
    return _cf_batch_dev(d_prof, CF_CONTRIB, full, d_ok, stream, over)


def transmittance_dev(d_prof, full=False, d_ok=None, stream=None, over=None):
    """Device form of transmittance(), as contribution_dev."""
    return _cf_batch_dev(d_prof, CF_TRANSMIT, full, d_ok, stream, over)


# ---- parameters in: a posterior's samples (include/bartrt.h, bartrt_cf_params) ----------------
def _cf_params(params, filters, kind, full):
    p = np.ascontiguousarray(params, np.double)
    p = p.reshape(-1, p.shape[-1])
    nf = cf_setup(filters)
    n, L, W = p.shape[0], nlayers(), _cf_wlocal()
    band = np.zeros((n, nf, L))
    fout = np.zeros((n, W, L)) if full else None
    status = np.zeros(n, np.int32)
    _check(trm.lib().bartrt_cf_params(_ptr(p), n, p.shape[1], kind, _ptr(band), _ptr(fout) if full else None,
                                      _ptr(status)))
    return band, fout, status


def contribution_from_params(params, filters, normalize=True, full=False):
    """Band-averaged contribution functions of parameter vectors [nwalkers, npars] as step_batch takes them (after
    step_setup; eclipse geometry): T(p), abundances and the radius / cloud-top / Rayleigh slots declared with
    step_set_extras are each sample's own.  -> (filt_cf [nwalkers, nfilters, L], then (normalize) filt_cf_norm, then
    (full) [nwalkers, W, L], status [nwalkers]): status 0, 1 (temperature), 2 (abundance) as step_batch reports it; a
    rejected sample's rows are NaN."""
    from .cf import normalize as _norm
    band, fout, status = _cf_params(params, filters, CF_CONTRIB, full)
    if normalize:
        # (filt_cf_norm of the accepted samples; a rejected sample's rows stay NaN without a warning)
        norm = np.full_like(band, np.nan)
        good = status == 0
        if good.any():
            norm[good] = _norm(band[good])
    return tuple([band] + ([norm] if normalize else []) + ([fout] if full else []) + [status])


def transmittance_from_params(params, filters, full=False):
    """Band-averaged transmittance of parameter vectors, as contribution_from_params (any geometry):
    -> (band [nwalkers, nfilters, L], then (full) [nwalkers, W, L], status)."""
    band, fout, status = _cf_params(params, filters, CF_TRANSMIT, full)
    return tuple([band] + ([fout] if full else []) + [status])


def _cf_params_dev(d_params, kind, full, stream):
    import torch
    assert d_params.is_cuda and d_params.dtype == torch.float64 and d_params.is_contiguous() and d_params.dim() == 2
    n, npars = d_params.shape
    band, fout = _cf_dev_outputs(n, full, d_params.device)
    status = torch.empty(n, dtype=torch.int32, device=d_params.device)
    _check(trm.lib().bartrt_cf_params_dev(
        C.c_void_p(d_params.data_ptr()), n, npars, kind, C.c_void_p(band.data_ptr()),
        C.c_void_p(fout.data_ptr()) if full else None, C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
    return (band, fout, status) if full else (band, status)


def contribution_from_params_dev(d_params, full=False, stream=None):
    """Device form of contribution_from_params for the filters of the latest cf_setup: a float64 CUDA tensor
    [nwalkers, npars] -> (band, status) tensors (band not normalised), (band, full, status) with ``full``.
    Asynchronous on torch's current stream."""
    return _cf_params_dev(d_params, CF_CONTRIB, full, stream)


def transmittance_from_params_dev(d_params, full=False, stream=None):
    """Device form of transmittance_from_params, as contribution_from_params_dev."""
    return _cf_params_dev(d_params, CF_TRANSMIT, full, stream)


# ---- exact order statistics and posterior envelopes (include/bartrt.h, bartrt_colselect) ----------------
def colselect_slab() -> int:
    """The rows of a column one workgroup of the selection owns (tests place their shapes around it)."""
    rows = C.c_long()
    _check(trm.lib().bartrt_colselect_slab(C.byref(rows)))
    return rows.value


def colselect_set_slab(rows: int) -> None:
    """Another slab size (0: the default).  For tests: results do not depend on it."""
    _check(trm.lib().bartrt_colselect_set_slab(int(rows)))


def _row_stride(shape, strides, itemsize):
    """ld of a two-dimensional array whose rows are contiguous (a padded view is taken as it lies)."""
    if len(shape) != 2 or (shape[1] > 1 and strides[1] != itemsize) or strides[0] % itemsize or strides[0] < 0:
        return None
    ld = strides[0] // itemsize
    return ld if (ld >= shape[1] or shape[0] == 1) else None


def _matrix_arg(x, ok, who):
    """The matrix of colselect, marginals and marginals_range (``who``): -> (x, nrows, ld, x pointer, ok, ok pointer,
    is_host).  x [nrows, ncols] float64, numpy or CUDA tensor, rows contiguous (a padded view is read in place), else
    copied; ok [nrows] or None.  Pure numpy / torch: the library is not touched."""
    if isinstance(x, np.ndarray):
        if x.dtype != np.double or x.ndim != 2:
            x = np.ascontiguousarray(x, np.double)
            x = x.reshape(-1, x.shape[-1]) if x.ndim != 2 else x
        ld = _row_stride(x.shape, x.strides, 8)
        if ld is None:
            x = np.ascontiguousarray(x)
            ld = x.shape[1]
        m = None if ok is None else np.ascontiguousarray(np.asarray(ok) != 0, np.uint8)
        if m is not None and m.shape != (x.shape[0],):
            raise ValueError(who + ": ok must have one entry per row")
        return x, x.shape[0], max(ld, x.shape[1]), C.c_void_p(x.ctypes.data), m, (_ptr(m) if m is not None else None), True
    import torch
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    ld = _row_stride(tuple(x.shape), tuple(s * 8 for s in x.stride()), 8)
    if ld is None:
        x = x.contiguous()
        ld = x.shape[1]
    if ok is not None:
        assert ok.is_cuda and ok.dtype == torch.uint8 and ok.is_contiguous() and ok.shape == (x.shape[0],)
    return (x, x.shape[0], max(ld, x.shape[1]), C.c_void_p(x.data_ptr()), ok,
            (C.c_void_p(ok.data_ptr()) if ok is not None else None), False)


def colselect(x, ranks, ok=None, stream=None):
    """Order statistics of the columns of x [nrows, ncols]: -> [nranks, ncols], row r the values
    np.sort(x[ok], axis=0)[ranks[r]] has, bit for bit.  ``x``: a float64 numpy array (host form: a rank at or above
    the rows that count raises) or a float64 CUDA tensor (device form, asynchronous on torch's current stream: such a
    rank gives NaN).  Rows may be padded (a view x[:, :ncols] of a wider array is read in place).  ``ok`` [nrows]:
    rows with 0 do not exist.  At most 16 ranks, any order, duplicates allowed."""
    r = np.ascontiguousarray(ranks, np.int64).ravel()
    x, nrows, ld, xp, ok, okp, host = _matrix_arg(x, ok, "colselect")
    if host:
        out = np.zeros((r.size, x.shape[1]))
        _check(trm.lib().bartrt_colselect(xp, nrows, x.shape[1], ld, okp, r.size, _ptr(r), _ptr(out)))
        return out
    import torch
    out = torch.empty((r.size, x.shape[1]), dtype=torch.float64, device=x.device)
    _check(trm.lib().bartrt_colselect_dev(xp, nrows, x.shape[1], ld, okp, r.size, _ptr(r), C.c_void_p(out.data_ptr()),
                                          _stream_ptr(stream)))
    return out


def percentile_rule(n: int, q: float):
    """np.percentile's default linear rule for n sorted values: -> (lo, hi, w), the two neighbouring ranks and the
    weight (csrc/quant_core.hpp)."""
    lo, hi, w = C.c_long(), C.c_long(), C.c_double()
    _check(trm.lib().bartrt_percentile_rule(int(n), float(q), C.byref(lo), C.byref(hi), C.byref(w)))
    return lo.value, hi.value, w.value


def percentile_lerp(a, b, w: float) -> np.ndarray:
    """The value between the order statistics a (rank lo) and b (rank hi) at weight w, elementwise."""
    a, b = np.ascontiguousarray(a, np.double), np.ascontiguousarray(b, np.double)
    out = np.empty_like(a)
    _check(trm.lib().bartrt_percentile_lerp(_ptr(a), _ptr(b), float(w), _ptr(out), a.size))
    return out


def percentiles_dev(d_x, q, d_ok=None, count=None):
    """Percentiles q (at most 8) of every column of the CUDA tensor d_x [nrows, ncols] over the rows d_ok (uint8
    tensor) lets count: two order statistics per percent selected on the device (colselect), interpolated by
    percentile_lerp.  ``count``: the rows that count, when the caller knows it (else read from d_ok).
    -> (values [nq, ncols], order [2 nq, ncols], ranks [2 nq]) numpy arrays; NaN values when no row counts."""
    q = [float(v) for v in np.atleast_1d(q)]
    ncols = d_x.shape[1]
    if count is None:
        count = d_x.shape[0] if d_ok is None else int(d_ok.count_nonzero().item())
    if count == 0:
        return np.full((len(q), ncols), np.nan), np.full((2 * len(q), ncols), np.nan), np.zeros(2 * len(q), np.int64)
    rules = [percentile_rule(count, v) for v in q]
    ranks = np.array([k for lo, hi, _ in rules for k in (lo, hi)], np.int64)
    order = colselect(d_x, ranks, d_ok).cpu().numpy()
    vals = np.stack([percentile_lerp(order[2 * i], order[2 * i + 1], rules[i][2]) for i in range(len(q))])
    return vals, order, ranks


def posterior_set_chunk(rows: int) -> None:
    """Rows per chunk of posterior_tp (0: the default).  The envelope does not depend on it."""
    _check(trm.lib().bartrt_posterior_set_chunk(int(rows)))


def posterior_tp(params, q, chunk=None, want_order=False):
    """The percentile envelope of the temperature profiles of parameter vectors [nsamples, npars] as step_batch takes
    them (after step_setup; include/bartrt.h, bartrt_posterior_tp): -> (env [nq, L] in atm layer order, status
    [nsamples], ngood); with ``want_order`` also (ranks [2 nq], order [2 nq, L]), the order statistics behind the
    envelope (None, None when no sample was accepted).  At most 8 percents.  ``chunk``: rows per conversion launch."""
    p = np.ascontiguousarray(params, np.double)
    p = p.reshape(-1, p.shape[-1])
    qs = np.ascontiguousarray(np.atleast_1d(q), np.double)
    L = nlayers()
    env = np.zeros((qs.size, L))
    status = np.zeros(p.shape[0], np.int32)
    ngood = C.c_long()
    if chunk is not None:
        posterior_set_chunk(chunk)
    try:
        _check(trm.lib().bartrt_posterior_tp(_ptr(p), p.shape[0], p.shape[1], qs.size, _ptr(qs), _ptr(env),
                                             _ptr(status), C.byref(ngood)))
    finally:
        if chunk is not None:
            posterior_set_chunk(0)
    if not want_order:
        return env, status, ngood.value
    if ngood.value == 0:
        return env, status, 0, None, None
    ranks, order = np.zeros(2 * qs.size, np.int64), np.zeros((2 * qs.size, L))
    _check(trm.lib().bartrt_posterior_tp_order(qs.size, L, _ptr(ranks), _ptr(order)))
    return env, status, ngood.value, ranks, order


# ---- posterior spectra: the display quantity and its envelopes (include/bartrt.h, bartrt_posterior_spectrum) ----
def _display_args(half, stride):
    half = np.ascontiguousarray(half, np.double).ravel()
    if half.size < 1:
        raise ValueError("the half kernel holds at least its centre weight")
    return half, half.size - 1, int(stride)


def spectrum_display_tile(r: int, stride: int = 1) -> int:
    """The kept output columns one workgroup of the display kernel owns (tests place their shapes around it)."""
    cols = C.c_long()
    _check(trm.lib().bartrt_spectrum_display_tile(int(r), int(stride), C.byref(cols)))
    return cols.value


def spectrum_display_dev(d_spec, half, d_sflux=None, rprs=1.0, stride=1, nwave=None, stream=None):
    """The display quantity of the spectra d_spec [nrows, >= nwave] (float64 CUDA tensor, rows contiguous; a padded view
    is read in place): -> [nrows, ceil(nwave / stride)] CUDA tensor, asynchronous on torch's current stream.  With
    ``d_sflux`` [nwave] the rows are x / sflux * rprs * rprs before the smoothing; ``half`` [r + 1]: the symmetric
    kernel's half, centre first (posterior.gauss_half); csrc/specenv_core.hpp has the rule."""
    import torch
    half, r, stride = _display_args(half, stride)
    assert d_spec.is_cuda and d_spec.dtype == torch.float64 and d_spec.dim() == 2
    ld = _row_stride(tuple(d_spec.shape), tuple(s * 8 for s in d_spec.stride()), 8)
    if ld is None:
        d_spec = d_spec.contiguous()
        ld = d_spec.shape[1]
    nwave = d_spec.shape[1] if nwave is None else int(nwave)
    if d_sflux is not None:
        assert d_sflux.is_cuda and d_sflux.dtype == torch.float64 and d_sflux.is_contiguous() and d_sflux.numel() >= nwave
    wk = -(-nwave // stride) if stride >= 1 and nwave >= 1 else 1
    out = torch.empty((d_spec.shape[0], wk), dtype=torch.float64, device=d_spec.device)
    _check(trm.lib().bartrt_spectrum_display_dev(
        C.c_void_p(d_spec.data_ptr()), d_spec.shape[0], nwave, max(ld, d_spec.shape[1]),
        C.c_void_p(d_sflux.data_ptr()) if d_sflux is not None else None, float(rprs), r, _ptr(half), stride,
        C.c_void_p(out.data_ptr()), wk, _stream_ptr(stream)))
    return out


def posterior_spectrum(params, q, sflux, half, stride=1, chunk=None, want_order=False):
    """The percentile envelopes of the display quantity and of the band fluxes of parameter vectors [nsamples, npars]
    as step_batch takes them (after step_setup, whose rprs and filters are used; include/bartrt.h,
    bartrt_posterior_spectrum): -> (env_spec [nq, Wk], env_band [nq, F], status [nsamples], ngood); with ``want_order``
    also (ranks [2 nq], order_spec [2 nq, Wk], order_band [2 nq, F]), the order statistics behind the envelopes (None
    each when no sample was accepted).  ``sflux`` [nwave]: the stellar flux on the engine's grid (eclipse) or None;
    ``half``: the smoothing kernel's half; ``stride``: every stride-th grid sample is kept, Wk = ceil(nwave / stride),
    and the sample matrix takes nsamples * Wk * 8 bytes of device memory.  ``chunk``: rows per launch, at most 4096 (a
    larger value is cut to that); the result does not depend on it, because every launch's RT kernel variant is chosen
    as for 4096 rows -- which is also why a sample's spectrum here can differ in the last bits from step_batch_dev's
    on a small batch."""
    p = np.ascontiguousarray(params, np.double)
    p = p.reshape(-1, p.shape[-1])
    qs = np.ascontiguousarray(np.atleast_1d(q), np.double)
    half, r, stride = _display_args(half, stride)
    wk, nf = C.c_long(), C.c_int()
    _check(trm.lib().bartrt_posterior_spectrum_shape(stride, C.byref(wk), C.byref(nf)))
    wk, nf = wk.value, nf.value
    if sflux is not None:
        sflux = np.ascontiguousarray(sflux, np.double).ravel()
        if sflux.size != trm.get_no_samples():
            raise ValueError("posterior_spectrum: sflux has one value per sample of the engine's grid")
    env_spec, env_band = np.zeros((qs.size, wk)), np.zeros((qs.size, nf))
    status = np.zeros(p.shape[0], np.int32)
    ngood = C.c_long()
    if chunk is not None:
        posterior_set_chunk(chunk)
    try:
        _check(trm.lib().bartrt_posterior_spectrum(
            _ptr(p), p.shape[0], p.shape[1], qs.size, _ptr(qs), _ptr(sflux) if sflux is not None else None, r,
            _ptr(half), stride, _ptr(env_spec), _ptr(env_band), _ptr(status), C.byref(ngood)))
    finally:
        if chunk is not None:
            posterior_set_chunk(0)
    if not want_order:
        return env_spec, env_band, status, ngood.value
    if ngood.value == 0:
        return env_spec, env_band, status, 0, None, None, None
    ranks, ospec, oband = np.zeros(2 * qs.size, np.int64), np.zeros((2 * qs.size, wk)), np.zeros((2 * qs.size, nf))
    _check(trm.lib().bartrt_posterior_spectrum_order(qs.size, wk, nf, _ptr(ranks), _ptr(ospec), _ptr(oband)))
    return env_spec, env_band, status, ngood.value, ranks, ospec, oband


def posterior_spectrum_rows(row0: int, nrows: int, wk: int) -> np.ndarray:
    """Rows row0 .. row0 + nrows - 1 of the latest posterior_spectrum's sample matrix -> [nrows, wk] (``wk``: the
    call's kept columns, env_spec.shape[1]): every sample's display curve, rejected samples' rows as they lie."""
    out = np.zeros((int(nrows), int(wk)))
    _check(trm.lib().bartrt_posterior_spectrum_rows(int(row0), int(nrows), _ptr(out)))
    return out


# ---- posterior marginals: histograms, ranges, HPD regions (include/bartrt.h, bartrt_marginals) ------------------
def marginals_slab() -> int:
    """The rows one workgroup of the histogram kernels owns (tests place their shapes around it)."""
    rows = C.c_long()
    _check(trm.lib().bartrt_marginals_slab(C.byref(rows)))
    return rows.value


def marginals_set_slab(rows: int) -> None:
    """Another slab size (0: the default).  For tests: no count depends on it."""
    _check(trm.lib().bartrt_marginals_set_slab(int(rows)))


def marginals_set_chunk(rows: int) -> None:
    """Rows per upload of the host forms (0: the default, 64 MiB).  For tests: no count depends on it."""
    _check(trm.lib().bartrt_marginals_set_chunk(int(rows)))


def _marginals_cols(x, cols, who):
    c = np.ascontiguousarray(cols, np.int32).ravel()
    if c.size and (c.min() < 0 or c.max() >= x.shape[1]):
        raise ValueError("%s: cols must lie in 0..%d" % (who, x.shape[1] - 1))
    return c


def marginals_range(x, cols, ok=None, stream=None):
    """The smallest and largest finite value of the columns ``cols`` of x [nrows, ncols] among the rows ``ok`` lets
    count, and their number: -> (lohi [nsel, 2], nfinite [nsel]).  np.nanmin / np.nanmax over the finite values, bit
    for bit; NaN, NaN, 0 for a column without one.  ``x``: a float64 numpy array (host form, uploaded in chunks) or a
    float64 CUDA tensor (device form, asynchronous on torch's current stream; the results are CUDA tensors, nfinite
    as int64).  Needs no engine."""
    x, nrows, ld, xp, ok, okp, host = _matrix_arg(x, ok, "marginals_range")
    c = _marginals_cols(x, cols, "marginals_range")
    if host:
        lohi, nfin = np.zeros((c.size, 2)), np.zeros(c.size, np.uint64)
        _check(trm.lib().bartrt_marginals_range(xp, nrows, ld, okp, c.size, _ptr(c), _ptr(lohi), _ptr(nfin)))
        return lohi, nfin
    import torch
    lohi = torch.zeros((c.size, 2), dtype=torch.float64, device=x.device)
    nfin = torch.zeros(c.size, dtype=torch.int64, device=x.device)
    _check(trm.lib().bartrt_marginals_range_dev(xp, nrows, ld, okp, c.size, _ptr(c), C.c_void_p(lohi.data_ptr()),
                                                C.c_void_p(nfin.data_ptr()), _stream_ptr(stream)))
    return lohi, nfin


def marginals(x, cols, edges, pairs=True, ok=None, stream=None):
    """1-D and pairwise histograms of the columns ``cols`` of x [nrows, ncols] (include/bartrt.h, bartrt_marginals):
    -> (h1 [nsel, nbins], outside [nsel, 3], h2 [npairs, nbins, nbins] or None without ``pairs``).  ``edges`` [nsel,
    nbins + 1] (host): finite, strictly increasing, uniform or not; h1[s] is np.histogram(x[ok, cols[s]],
    bins=edges[s])[0], outside[s] the values below / above the edges and the NaNs, h2[p] np.histogram2d of the pair
    (a, b) of selection indices, a < b, a-major, with bins=[edges[a], edges[b]] -- equal integers.  At most 64 columns,
    1024 bins, 128 bins with pairs.  ``x``: a float64 numpy array (host form: uploaded in chunks, uint64 results) or
    a float64 CUDA tensor (device form, asynchronous on torch's current stream, int64 CUDA tensors).  Needs no engine."""
    x, nrows, ld, xp, ok, okp, host = _matrix_arg(x, ok, "marginals")
    c = _marginals_cols(x, cols, "marginals")
    e = np.ascontiguousarray(edges, np.double)
    if e.ndim != 2 or e.shape[0] != c.size or e.shape[1] < 2:
        raise ValueError("marginals: edges must be [nsel, nbins + 1]")
    nbins, npairs = e.shape[1] - 1, c.size * (c.size - 1) // 2
    lib = trm.lib()
    if host:
        h1, out = np.zeros((c.size, nbins), np.uint64), np.zeros((c.size, 3), np.uint64)
        h2 = np.zeros((npairs, nbins, nbins), np.uint64) if pairs else None
        _check(lib.bartrt_marginals(xp, nrows, ld, okp, c.size, _ptr(c), nbins, _ptr(e), _ptr(h1), _ptr(out),
                                    _ptr(h2) if pairs else None))
        return h1, out, h2
    import torch
    new = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=x.device)
    h1, out, h2 = new(c.size, nbins), new(c.size, 3), (new(npairs, nbins, nbins) if pairs else None)
    _check(lib.bartrt_marginals_dev(xp, nrows, ld, okp, c.size, _ptr(c), nbins, _ptr(e), C.c_void_p(h1.data_ptr()),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(h2.data_ptr()) if pairs else None,
                                    _stream_ptr(stream)))
    return h1, out, h2


def hpd(counts, p: float):
    """The highest-density region of a histogram at fraction 0 < p <= 1 (include/bartrt.h, bartrt_hpd; the rule is
    csrc/hist_core.hpp's): -> (mask [nbins] bool, threshold, included, nruns).  On the host; needs no device."""
    c = np.ascontiguousarray(counts, np.uint64).ravel()
    mask = np.zeros(c.size, np.uint8)
    thr, inc, runs = C.c_ulonglong(), C.c_ulonglong(), C.c_int()
    _check(trm.lib().bartrt_hpd(_ptr(c), c.size, float(p), _ptr(mask), C.byref(thr), C.byref(inc), C.byref(runs)))
    return mask.astype(bool), thr.value, inc.value, runs.value


# ---- posterior kernel density estimates (include/bartrt.h, bartrt_kde) ------------------------------------------
KDE_RULES = {"scott": 0, "silverman": 1}


def kde_tile() -> int:
    """The rows of a tile of the density's sums, a constant of the rule (tests place their shapes around it)."""
    rows = C.c_long()
    _check(trm.lib().bartrt_kde_tile(C.byref(rows)))
    return rows.value


def kde_chunk() -> int:
    rows = C.c_long()
    _check(trm.lib().bartrt_kde_chunk(C.byref(rows)))
    return rows.value


def kde_set_chunk(rows: int) -> None:
    """Rows per upload of the host form and per round of launches of either form (0: the default, 64 MiB).  For tests:
    no result depends on it."""
    _check(trm.lib().bartrt_kde_set_chunk(int(rows)))


def _kde_rule(bw):
    if isinstance(bw, str):
        if bw not in KDE_RULES:
            raise ValueError("kde: bw is 'scott', 'silverman' or a positive number")
        return KDE_RULES[bw], 0.0
    return 2, float(bw)


def kde(x, cols, grid, bw="scott", ok=None, stream=None):
    """Gaussian kernel density estimates of the columns ``cols`` of x [nrows, ncols], column cols[s] on grid[s]
    (include/bartrt.h, bartrt_kde; the rule is csrc/kde_core.hpp's): -> (pdf [nsel, ngrid], stat [nsel, 4] = n, mean,
    std (ddof 1), h, nonfinite [nsel]).  ``grid`` [nsel, ngrid] (host): finite values in any order, at most 1024 per
    column.  ``bw``: 'scott', 'silverman' or a positive factor, as scipy.stats.gaussian_kde's bw_method; pdf[s] is
    gaussian_kde(x[ok, cols[s]], bw)(grid[s]) over the finite values, to about 1e-13 relative (the RT kernels' exponential
    is that far from exp).  A column with fewer than two finite values or
    without spread has a NaN row and h = NaN.  ``x``: a float64 numpy array (host form: uploaded in chunks, twice) or a
    float64 CUDA tensor (device form, asynchronous on torch's current stream; CUDA tensors come back, nonfinite as
    int64).  kde_dev is the device form by name.  Needs no engine."""
    x, nrows, ld, xp, ok, okp, host = _matrix_arg(x, ok, "kde")
    c = _marginals_cols(x, cols, "kde")
    g = np.ascontiguousarray(grid, np.double)
    if g.ndim != 2 or g.shape[0] != c.size or g.shape[1] < 1:
        raise ValueError("kde: grid must be [nsel, ngrid]")
    rule, factor = _kde_rule(bw)
    lib = trm.lib()
    if host:
        pdf, stat, bad = np.zeros(g.shape), np.zeros((c.size, 4)), np.zeros(c.size, np.uint64)
        _check(lib.bartrt_kde(xp, nrows, ld, okp, c.size, _ptr(c), g.shape[1], _ptr(g), rule, factor, _ptr(pdf),
                              _ptr(stat), _ptr(bad)))
        return pdf, stat, bad
    import torch
    pdf = torch.zeros(g.shape, dtype=torch.float64, device=x.device)
    stat = torch.zeros((c.size, 4), dtype=torch.float64, device=x.device)
    bad = torch.zeros(c.size, dtype=torch.int64, device=x.device)
    _check(lib.bartrt_kde_dev(xp, nrows, ld, okp, c.size, _ptr(c), g.shape[1], _ptr(g), rule, factor,
                              C.c_void_p(pdf.data_ptr()), C.c_void_p(stat.data_ptr()), C.c_void_p(bad.data_ptr()),
                              _stream_ptr(stream)))
    return pdf, stat, bad


def kde_dev(d_x, cols, grid, bw="scott", d_ok=None, stream=None):
    """kde on a float64 CUDA tensor: asynchronous on ``stream`` (None: torch's current stream), CUDA tensors back."""
    assert not isinstance(d_x, np.ndarray)
    return kde(d_x, cols, grid, bw, d_ok, stream)


def hpd_pdf(pdf, p: float):
    """The credible region of a density on a grid at fraction 0 < p <= 1 (include/bartrt.h, bartrt_hpd_pdf; the rule is
    csrc/kde_core.hpp's): -> (mask [n] bool, threshold, included, nruns).  On the host; needs no device."""
    v = np.ascontiguousarray(pdf, np.double).ravel()
    mask = np.zeros(v.size, np.uint8)
    thr, inc, runs = C.c_double(), C.c_double(), C.c_int()
    _check(trm.lib().bartrt_hpd_pdf(_ptr(v), v.size, float(p), _ptr(mask), C.byref(thr), C.byref(inc), C.byref(runs)))
    return mask.astype(bool), thr.value, inc.value, runs.value
