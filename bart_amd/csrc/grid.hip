// Model grids (MC3's `walk = unif`; the reference makes the training sets of its surrogate models this way,
// code/makecfg.py:177-190): nrows parameter vectors per iteration drawn uniformly in the box (grid_core.hpp), one
// batched model call on them, and the whole model rows -- spectra or band fluxes -- handed to the caller in chunks
// of iterations.  No data, no chi-square, no acceptance, no population.  On the engine's stream an iteration is three
// things, enqueued without a host wait: grid_draw, step_run_dev, grid_pack.  A chunk ends with one asynchronous copy
// per array into pinned memory and an event; two chunks are in flight, as the two blocks of mcmc_run_resident.
#include <algorithm>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/bartrt.h"
#include "comm.hpp"
#include "engine.hpp"
#include "grid_core.hpp"
#include "step.hpp"

namespace bartrt {
namespace {

constexpr int kPackTile = 1024;   // entries of a model row one workgroup of grid_pack moves

// One lane per row: the sample of (t, row) into the rows the step reads, and the same values into the chunk's
// params slot (the caller passes the slot of this iteration).
__global__ __launch_bounds__(256) void grid_draw(unsigned long long seed, unsigned long long t, int nrows, int npars,
                                                 const double *params, const double *pmin, const double *pmax,
                                                 const double *stepsize, double *rows, double *slot) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)nrows) return;
  double *r = rows + i * npars;
  grid::sample(seed, t, (int)i, npars, params, pmin, pmax, stepsize, r);
  if (slot)
    for (int j = 0; j < npars; j++) slot[i * npars + j] = r[j];
}

// One workgroup per (row, tile of kPackTile entries of the width), the tile fastest: src [nrows][width] -> the chunk
// slot of this iteration dst [nrows][width], as T.  A row whose status is not 0 becomes -1 in every entry, whatever
// the step left in src.  The first tile's workgroup writes the row's status into the chunk's status slot.
template <class T>
__global__ __launch_bounds__(256) void grid_pack(const double *src, const int *status, int nrows, size_t width,
                                                 unsigned ntiles, T *dst, int *status_slot) {
  const size_t row = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
  if (row >= (size_t)nrows) return;
  const int st = status[row];
  if (tile == 0 && threadIdx.x == 0) status_slot[row] = st;
  const size_t begin = tile * (size_t)kPackTile, end = begin + kPackTile < width ? begin + kPackTile : width;
  const double *s = src + row * width;
  T *d = dst + row * width;
  for (size_t k = begin + threadIdx.x; k < end; k += blockDim.x) d[k] = st == 0 ? (T)s[k] : (T)-1.0;
}

struct Events {
  hipEvent_t ev[2] = {nullptr, nullptr};
  Events() {
    for (hipEvent_t &e : ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  ~Events() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// the refusals that need no engine, `who` in front
void check_problem(const std::string &who, int nrows, int npars, const double *pmin, const double *pmax,
                   const double *stepsize) {
  // (rows: the second grid dimension of the step's band integration)
  if (nrows < 1 || nrows > 65535) throw std::invalid_argument(who + ": 1 <= nrows <= 65535");
  if (npars < 1 || npars > kMaxPars) throw std::invalid_argument(who + ": 1 <= npars <= 64");
  if (const int bad = check_stepsize(npars, stepsize, nullptr))
    throw std::invalid_argument(who + ": stepsize[" + std::to_string(bad - 1) + "] = " +
                                std::to_string(stepsize[bad - 1]) + " shares parameter " + std::to_string(bad - 1) +
                                " with a parameter that is out of range or itself shared");
  if (const int bad = grid::check_box(npars, pmin, pmax, stepsize))
    throw std::invalid_argument(who + ": pmin[" + std::to_string(bad - 1) + "] > pmax[" + std::to_string(bad - 1) +
                                "] on a free parameter");
}

// params pmin pmax stepsize in one device buffer
struct DeviceBox {
  DevBuf<double> buf;
  const double *params, *pmin, *pmax, *stepsize;
  DeviceBox(int npars, const double *par, const double *lo, const double *hi, const double *step) {
    std::vector<double> c;
    for (const double *v : {par, lo, hi, step}) c.insert(c.end(), v, v + npars);
    buf.upload(c);
    params = buf;
    pmin = params + npars;
    pmax = pmin + npars;
    stepsize = pmax + npars;
  }
};

// room for n elements of a chunk slot, or the refusal that names the bytes
template <class Buf>
void reserve_slot(Buf &b, size_t n, const char *what) {
  try {
    b.reserve(n);
  } catch (const HipError &) {
    (void)hipGetLastError();
    throw std::invalid_argument(std::string("grid_run: cannot allocate the ") + what + " of a chunk, " +
                                std::to_string(n * sizeof(*b.get())) + " bytes: give a smaller `chunk`");
  }
}

}  // namespace

void grid_draws_probe(unsigned long long seed, unsigned long long t, int nrows, int npars, const double *params,
                      const double *pmin, const double *pmax, const double *stepsize, double *out) {
  check_problem("bartrt_grid_draws", nrows, npars, pmin, pmax, stepsize);
  const DeviceBox box(npars, params, pmin, pmax, stepsize);
  DevBuf<double> d;
  d.reserve((size_t)nrows * npars);
  grid_draw<<<dim3((unsigned)((nrows + 255) / 256)), dim3(256)>>>(seed, t, nrows, npars, box.params, box.pmin, box.pmax,
                                                                 box.stepsize, d, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, d, sizeof(double) * (size_t)nrows * npars, hipMemcpyDeviceToHost));
}

int grid_run(Engine &e, int nrows, int npars, long nsteps, const double *params, const double *pmin,
             const double *pmax, const double *stepsize, const GridOpts &o, long *nbad) {
  if (!e.step) throw IoError{"grid_run: call step_setup first"};
  if (nsteps < 1 || o.chunk < 0 || o.first < 0) throw std::invalid_argument("grid_run: bad sizes");
  if (!o.sink) throw std::invalid_argument("grid_run: no sink to hand the chunks to");
  check_problem("grid_run", nrows, npars, pmin, pmax, stepsize);
  if (e.lbl && e.comm)
    throw CommError{BARTRT_ENOTSUP, "grid_run: line-by-line engines do not take the communicator's path"};
  if (!e.comm && (e.lo != 0 || e.hi != e.Wfull))
    throw IoError{"grid_run: the engine is sharded and has no communicator (engine.comm_init): it cannot make whole "
                  "model rows"};
  if (e.step->carry)
    throw std::invalid_argument("grid_run: the carry-over of step_set_carry makes a row depend on the call before; "
                                "a grid's samples are independent: switch it off");
  const int nf = e.step->nfilters;
  if (!o.spectra && nf < 1) throw std::invalid_argument("grid_run: band fluxes asked for and no filters set up");
  const size_t n = nrows, np = npars, width = o.spectra ? (size_t)e.Wfull : (size_t)nf;
  const size_t elem = o.f32 ? sizeof(float) : sizeof(double);
  const long C = o.chunk > 0 ? std::min(o.chunk, nsteps) : nsteps, nchunks = (nsteps + C - 1) / C;
  const int nslots = nchunks > 1 ? 2 : 1;
  if ((double)C * (double)n * (double)std::max(width * elem, np * sizeof(double)) * nslots >
      (double)std::numeric_limits<size_t>::max() / 2)
    throw std::invalid_argument("grid_run: a chunk of " + std::to_string(C) + " iterations is too large to address");
  const size_t per_par = (size_t)C * n * np, per_st = (size_t)C * n, per_rows = (size_t)C * n * width * elem;

  step_ensure(e, nrows);   // (it may wait for the device: before anything is enqueued)
  const DeviceBox box(npars, params, pmin, pmax, stepsize);
  DevBuf<double> d_rows, d_band, d_spec, d_par;
  DevBuf<int> d_status, d_st;
  DevBuf<unsigned char> d_out;
  PinBuf<double> h_par;
  PinBuf<int> h_st;
  PinBuf<unsigned char> h_out;
  d_rows.reserve(n * np);
  d_band.reserve(n * std::max(nf, 1));
  d_status.reserve(n);
  if (o.spectra) reserve_slot(d_spec, n * width, "scratch spectra");
  reserve_slot(d_par, per_par * nslots, "device parameter slots");
  reserve_slot(d_st, per_st * nslots, "device status slots");
  reserve_slot(d_out, per_rows * nslots, "device model-row slots");
  reserve_slot(h_par, per_par * nslots, "pinned parameter slots");
  reserve_slot(h_st, per_st * nslots, "pinned status slots");
  reserve_slot(h_out, per_rows * nslots, "pinned model-row slots");

  Events events;
  const hipStream_t st = e.stream;
  const unsigned ntiles = (unsigned)((width + kPackTile - 1) / kPackTile);
  if ((size_t)ntiles * n > 0x7fffffffull) throw std::invalid_argument("grid_run: too many rows for this width");
  auto length = [&](long k) { return std::min(C, nsteps - k * C); };
  auto enqueue = [&](long k) {   // chunk k into slot k % 2
    const size_t s = (size_t)(k % 2);
    for (long q = 0; q < length(k); q++) {
      const unsigned long long t = (unsigned long long)(o.first + k * C + q);
      const size_t at = (size_t)q * n;
      hipLaunchKernelGGL(grid_draw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, o.seed, t, nrows, npars,
                         box.params, box.pmin, box.pmax, box.stepsize, d_rows.get(), d_par + s * per_par + at * np);
      HIPCHK(hipGetLastError());
      step_run_dev(e, d_rows, nrows, npars, d_band, d_status, o.spectra ? d_spec.get() : nullptr, st, nullptr);
      const double *src = o.spectra ? d_spec.get() : d_band.get();
      int *status_slot = d_st + s * per_st + at;
      unsigned char *dst = d_out + s * per_rows + at * width * elem;
      if (o.f32)
        hipLaunchKernelGGL(grid_pack<float>, dim3(ntiles * (unsigned)n), dim3(256), 0, st, src, d_status.get(), nrows,
                           width, ntiles, reinterpret_cast<float *>(dst), status_slot);
      else
        hipLaunchKernelGGL(grid_pack<double>, dim3(ntiles * (unsigned)n), dim3(256), 0, st, src, d_status.get(), nrows,
                           width, ntiles, reinterpret_cast<double *>(dst), status_slot);
      HIPCHK(hipGetLastError());
    }
    const size_t m = (size_t)length(k) * n;
    HIPCHK(hipMemcpyAsync(h_par + s * per_par, d_par + s * per_par, sizeof(double) * m * np, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_st + s * per_st, d_st + s * per_st, sizeof(int) * m, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_out + s * per_rows, d_out + s * per_rows, m * width * elem, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(events.ev[s], st));
  };

  long total[4] = {0, 0, 0, 0};
  int rc = 0;
  try {
    enqueue(0);
    for (long k = 0; k < nchunks && rc == 0; k++) {
      if (k + 1 < nchunks) enqueue(k + 1);   // (slot (k + 1) % 2: the sink has returned from chunk k - 1)
      const size_t s = (size_t)(k % 2);
      HIPCHK(hipEventSynchronize(events.ev[s]));
      const int *hs = h_st + s * per_st;
      for (size_t q = 0; q < (size_t)length(k) * n; q++)
        if (hs[q] >= 1 && hs[q] <= 3) total[hs[q]]++;
      rc = o.sink(k, o.first + k * C, length(k), h_par + s * per_par, hs, h_out + s * per_rows, o.user);
    }
  } catch (...) {
    (void)hipStreamSynchronize(st);   // nothing in flight writes a slot that is about to be freed
    throw;
  }
  HIPCHK(hipStreamSynchronize(st));   // (after a stop: the chunk in flight runs out; it is not handed over)
  if (nbad) {
    nbad[0] = 0;
    for (int k = 1; k < 4; k++) nbad[k] = total[k];
  }
  return rc;
}

}  // namespace bartrt
