// The display quantity of model spectra (specenv_core.hpp) as one kernel over a chunk of spectra as they leave the RT
// launch, and the posterior spectrum / band-flux envelope: the chunk loop of posterior_tp (quant.hip) with the step's
// whole run in it, spec_display between the run and the selection.
//
// TILES.  A workgroup owns (one sample row, one tile of kept output columns).  It stages the tile's y values -- the
// divide by the stellar flux happens on load -- plus a halo of r grid samples on each side in LDS; halo indices outside
// the row go through specenv::reflect_index, so the row's ends and rows shorter than the radius need no second path.
// One lane then computes one kept output from LDS (specenv::smooth_at) and the wave's 64 outputs are 64 neighbouring
// doubles of row `row` of the output matrix: one coalesced store.  Every spectrum value is read from HBM once per tile
// it falls into (the halo of 2r values per tile apart) and 1 / stride of them are written.  fp64 VALU, no atomics:
// every output is written by exactly one lane from values that depend on the row alone, so the result depends on no
// launch shape.
//
// The staged window of a tile of t outputs is (t - 1) stride + 1 + 2r doubles.  With kSpecTileOut outputs it fits the
// 64 kB every kernel gets up to stride 32; above that a tile has fewer outputs (spec_tile_out), down to one.
#include "specenv.hpp"

#include <algorithm>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "quant.hpp"
#include "scratch.hpp"
#include "step.hpp"

namespace bartrt {

namespace {

constexpr int kSpecThreads = kSpecTileOut;
constexpr long kSpecLdsDoubles = 64 * 1024 / sizeof(double);
constexpr unsigned kSpecMaxGridY = 65535;
// The RT kernel variant depends on the walkers of a launch (rt_launch.hpp), and two variants add the same terms in
// another order.  Every chunk's launch is therefore chosen as for this many walkers -- the default chunk, and the most
// rows a chunk of this call has (a larger bartrt_posterior_set_chunk is cut to it) -- so that the sample matrix holds
// the same bits whatever chunk size is set.  The price: a one-row call or a small posterior runs the variant made for
// full chunks, not the small-batch forms.
constexpr int kSpecSelWalkers = 4096;

__global__ __launch_bounds__(kSpecThreads) void spec_display(const double *__restrict__ spec, long nrows, long W, long ld,
                                                             const double *__restrict__ sflux, double rprs, int r,
                                                             specenv::HalfKernel half, long stride, int tile_out, long Wk,
                                                             double *__restrict__ out, long ldo) {
  extern __shared__ double lds_y[];   // [(nout - 1) stride + 1 + 2r]: grid samples g0 .. of the row, reflected
  const int tid = threadIdx.x;
  const long c0 = (long)blockIdx.x * tile_out;
  const int nout = (int)(Wk - c0 < tile_out ? Wk - c0 : tile_out);
  const long g0 = c0 * stride - r;
  const int span = (int)((nout - 1) * stride) + 1 + 2 * r;
  const bool star = sflux != nullptr;
  for (long row = blockIdx.y; row < nrows; row += gridDim.y) {
    const double *x = spec + (size_t)row * ld;
    for (int i = tid; i < span; i += kSpecThreads) {
      const long g = specenv::reflect_index(g0 + i, W);
      lds_y[i] = specenv::display_value(x[g], star, star ? sflux[g] : 1.0, rprs);
    }
    __syncthreads();
    if (tid < nout) {
      const double *centre = lds_y + r + (long)tid * stride;
      out[(size_t)row * ldo + c0 + tid] = specenv::smooth_at([&](long i) { return centre[i]; }, 0, r, half.w);
    }
    __syncthreads();
  }
}

}  // namespace

int spec_tile_out(int r, long stride) {
  const long fit = (kSpecLdsDoubles - 2 * r - 1) / stride + 1;
  return (int)std::min<long>(kSpecTileOut, fit);
}

void spectrum_display_dev(const double *d_spec, long nrows, int nwave, long ld, const double *d_sflux, double rprs, int r,
                          const double *half, long stride, double *d_out, long ldo, hipStream_t st) {
  specenv::HalfKernel hk{};
  for (int j = 0; j <= r; j++) hk.w[j] = half[j];
  const long Wk = specenv::kept_columns(nwave, stride);
  const int tile = spec_tile_out(r, stride);
  const size_t sh = sizeof(double) * (size_t)((tile - 1) * stride + 1 + 2 * r);
  const dim3 grid((unsigned)((Wk + tile - 1) / tile), (unsigned)std::min<long>(nrows, kSpecMaxGridY));
  hipLaunchKernelGGL(spec_display, grid, dim3(kSpecThreads), sh, st, d_spec, nrows, (long)nwave, ld, d_sflux, rprs, r, hk,
                     stride, tile, Wk, d_out, ldo);
  HIPCHK(hipGetLastError());
}

// the engine's scratch of the posterior spectrum envelope (scratch.hpp: the reuse rule)
struct SpecEnvState : Scratch {
  DevBuf<double> params, spec, sflux;
  DevBuf<double> disp, band;          // the sample matrices [nsamples][Wk], [nsamples][F]
  DevBuf<double> order_spec, order_band;
  DevBuf<int> status;
  DevBuf<unsigned char> good;
  long nrows = 0, Wk = 0;             // the latest sample matrix (nrows == 0: none)
  std::vector<long> last_ranks;
  std::vector<double> last_order_spec, last_order_band;
  int last_nq = 0, last_F = 0;
};

namespace {

SpecEnvState &state_of(Engine &e) {
  if (!e.specenv) e.specenv = new SpecEnvState;
  return *e.specenv;
}

__global__ void spec_mask_of_status(const int *__restrict__ status, long n, unsigned char *__restrict__ ok) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ok[i] = status[i] == 0;
}

// the step without the chains' carry-over for the length of a call: samples are independent
struct NoCarry {
  StepArgs &s;
  const int was;
  explicit NoCarry(StepArgs &a) : s(a), was(a.carry) { s.carry = 0; }
  ~NoCarry() { s.carry = was; }
};

}  // namespace

void specenv_release(Engine &e) {
  delete e.specenv;
  e.specenv = nullptr;
}

void posterior_spectrum(Engine &e, const double *params, long nsamples, int npars, int nq, const double *pct,
                        const double *sflux, int r, const double *half, long stride, double *env_spec, double *env_band,
                        int *status, long *ngood) {
  SpecEnvState &q = state_of(e);
  hipStream_t st = e.stream;
  const int W = e.Wfull, F = e.step->nfilters;
  const long Wk = specenv::kept_columns(W, stride);
  const long chunk = std::min({nsamples, posterior_chunk(e), (long)kSpecSelWalkers});
  const double nan = std::numeric_limits<double>::quiet_NaN();
  q.nrows = 0;
  q.last_nq = 0;
  q.room(q.params, (size_t)chunk * npars);
  q.room(q.spec, (size_t)chunk * W);
  q.room(q.band, (size_t)nsamples * std::max(F, 1));
  q.room(q.status, (size_t)nsamples);
  q.room(q.good, (size_t)nsamples);
  q.room(q.order_spec, (size_t)2 * nq * Wk);
  q.room(q.order_band, (size_t)2 * nq * std::max(F, 1));
  try {
    q.room(q.disp, (size_t)nsamples * Wk);
  } catch (const HipError &err) {
    if (err.e != hipErrorOutOfMemory) throw;
    (void)hipGetLastError();
    throw std::invalid_argument("posterior_spectrum: the sample matrix of " + std::to_string(nsamples) + " x " +
                                std::to_string(Wk) + " doubles asks for " + std::to_string((size_t)nsamples * Wk * 8) +
                                " bytes of device memory, which are not there: keep fewer columns (stride) or fewer "
                                "samples (thinning)");
  }
  if (sflux) {
    q.room(q.sflux, (size_t)W);
    HIPCHK(hipMemcpyAsync(q.sflux, sflux, sizeof(double) * W, hipMemcpyHostToDevice, st));
  }
  {
    NoCarry independent(*e.step);
    for (long off = 0; off < nsamples; off += chunk) {
      const int n = (int)std::min(chunk, nsamples - off);
      HIPCHK(hipMemcpyAsync(q.params, params + (size_t)off * npars, sizeof(double) * n * npars, hipMemcpyHostToDevice, st));
      // the band fluxes land in their rows of the [nsamples][F] matrix as the step writes them
      step_run_dev(e, q.params, n, npars, q.band + (size_t)off * F, q.status + off, q.spec, st, nullptr, kSpecSelWalkers);
      spectrum_display_dev(q.spec, n, W, W, sflux ? q.sflux.get() : nullptr, e.step->rprs, r, half, stride,
                           q.disp + (size_t)off * Wk, Wk, st);
    }
  }
  hipLaunchKernelGGL(spec_mask_of_status, dim3((unsigned)((nsamples + 255) / 256)), dim3(256), 0, st, q.status.get(),
                     nsamples, q.good.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(status, q.status, sizeof(int) * nsamples, hipMemcpyDeviceToHost, st));
  e.wait(st);
  q.nrows = nsamples;
  q.Wk = Wk;
  long good = 0;
  for (long i = 0; i < nsamples; i++) good += status[i] == 0;
  *ngood = good;
  if (good == 0) {
    for (size_t i = 0; i < (size_t)nq * Wk; i++) env_spec[i] = nan;
    for (size_t i = 0; i < (size_t)nq * F; i++) env_band[i] = nan;
    return;
  }
  std::vector<long> ranks((size_t)2 * nq);
  std::vector<double> w((size_t)nq);
  for (int i = 0; i < nq; i++) quant::percentile_rule(good, pct[i], &ranks[2 * i], &ranks[2 * i + 1], &w[i]);
  q.last_order_spec.resize((size_t)2 * nq * Wk);
  q.last_order_band.resize((size_t)2 * nq * F);
  colselect_dev(e, q.disp, nsamples, (int)Wk, Wk, q.good, 2 * nq, ranks.data(), q.order_spec, st);
  HIPCHK(hipMemcpyAsync(q.last_order_spec.data(), q.order_spec, sizeof(double) * 2 * nq * Wk, hipMemcpyDeviceToHost, st));
  if (F > 0) {
    colselect_dev(e, q.band, nsamples, F, F, q.good, 2 * nq, ranks.data(), q.order_band, st);
    HIPCHK(hipMemcpyAsync(q.last_order_band.data(), q.order_band, sizeof(double) * 2 * nq * F, hipMemcpyDeviceToHost, st));
  }
  e.wait(st);
  for (int i = 0; i < nq; i++) {
    for (long c = 0; c < Wk; c++)
      env_spec[(size_t)i * Wk + c] = quant::interpolate(q.last_order_spec[(size_t)(2 * i) * Wk + c],
                                                        q.last_order_spec[(size_t)(2 * i + 1) * Wk + c], w[i]);
    for (int f = 0; f < F; f++)
      env_band[(size_t)i * F + f] = quant::interpolate(q.last_order_band[(size_t)(2 * i) * F + f],
                                                       q.last_order_band[(size_t)(2 * i + 1) * F + f], w[i]);
  }
  q.last_ranks = ranks;
  q.last_nq = nq;
  q.last_F = F;
}

bool posterior_spectrum_order(const Engine &e, int nq, long Wk, int F, long *ranks, double *order_spec, double *order_band) {
  const SpecEnvState *q = e.specenv;
  if (!q || q->last_nq == 0 || q->last_nq != nq || q->Wk != Wk || q->last_F != F) return false;
  std::copy(q->last_ranks.begin(), q->last_ranks.end(), ranks);
  std::copy(q->last_order_spec.begin(), q->last_order_spec.end(), order_spec);
  std::copy(q->last_order_band.begin(), q->last_order_band.end(), order_band);
  return true;
}

long posterior_spectrum_cols(const Engine &e) { return e.specenv && e.specenv->nrows > 0 ? e.specenv->Wk : 0; }

bool posterior_spectrum_rows(Engine &e, long row0, long nrows, double *out) {
  SpecEnvState *q = e.specenv;
  if (!q || q->nrows == 0 || row0 < 0 || nrows < 0 || row0 > q->nrows || nrows > q->nrows - row0) return false;
  if (nrows == 0) return true;
  q->wait();
  HIPCHK(hipMemcpyAsync(out, q->disp + (size_t)row0 * q->Wk, sizeof(double) * (size_t)nrows * q->Wk, hipMemcpyDeviceToHost,
                        e.stream));
  e.wait(e.stream);
  return true;
}

}  // namespace bartrt
