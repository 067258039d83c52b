// Band-averaged contribution functions and transmittance of walker batches (include/bartrt.h, bartrt_cf_*).
//
// BART's last stage (reference code/cf.py:114-199) on the optical depths this engine walks, with no `toomuch` cut
// (the `tau.dat` of a `toomuch 1e100` run, without writing it):
//     cf[k] = B(T_k, nu) (exp(-tau[k-1]) - exp(-tau[k])) / (ln p_k - ln p_{k-1}),  cf[0] = 0   (eclipse / direct)
//     tr[k] = exp(-tau[k])                                                                     (any geometry)
// band-averaged per filter as filter_cf does it: trapz(x resp) / trapz(resp) with unit spacing over the grid samples
// inside the filter.
//
//  cf_eclipse<INTEG>  one lane per (walker, wavenumber), one wave per workgroup, the walker's layer records staged in
//                     LDS (the generic rt_eclipse's tiling, kernels.hip): per layer the table extinction (Rayleigh,
//                     grey cloud, molecules, CIA), TauColumn<INTEG>, then the layer's value.
//  cf_transit<STAGE>  the same for the transit geometry: the chord sum of the generic rt_transit (transit_geom.hip).
//  Dynamic LDS        with NC = 4 + 2 M + 2 C doubles and NI = 1 + C offsets per layer and the reduction block of
//                     16 x 65 doubles (8320 bytes): cf_eclipse 8 L (NC + NI) + 8320 (+ 24 (L + kSimpsonPad) under rule 1);
//                     cf_transit<true> 8 L (NC + NI + 64) + 8320, cf_transit<false> 512 L + 8320.  Above 64 kB the launch
//                     raises the kernel's limit first; cf_transit is staged while that fits in 160 kB, unstaged while
//                     512 L + 8320 does (L <= 303), and refused beyond (run_sums, launch_cf).
//  Band reduction     every 16 layers the wave's values go to an LDS block [16 layers][64 lanes]; for each filter
//                     that overlaps the tile, lane (j, q) sums layer j over the 16 wavenumbers of quarter q with the
//                     filter's weights h_i resp_i (h = 1/2 at the window's ends), two cross-lane butterflies add the
//                     quarters, and one partial per (walker, tile, filter, layer) goes to a workspace.
//  cf_block_sums      sums each filter's partials in tile order: this engine's part of the band sum, one value per
//                     (walker, filter, layer), layers from the top, not yet divided.
//  cf_combine         adds the ranks' parts in rank order, divides by trapz(resp), writes atm layer order.
// An engine on a wavenumber block [lo, hi) (--shard r n) does the same on its own samples: lane i of tile t is grid
// sample lo + 64 t + i, as the RT kernels' columns count, and cf_setup clips each window to the block -- the half
// weights stay at the window's true ends, whichever rank holds them, and trapz(resp) is the whole window's.  With a
// communicator (bartrt_comm_init) the parts go into this rank's slot of its receive buffer, ONE in-place all-gather
// per chunk fills the others, and cf_combine reads the slots where they lie; without one the only slot is a
// workspace of this module.  One rank: 0 + (the tile-order sum) is that sum, so the bits are those of a single pass.
// Posterior samples (bartrt_cf_batch_over, bartrt_cf_params): the layer records are prepared under each walker's own
// reference radius, cloud top and Rayleigh value (PrepArgs::over, the per-step path's mechanism); from parameter
// vectors the step's converter (step_convert_dev) writes profiles, statuses and those overrides into this module's
// workspaces first.  The CF kernels themselves do not know: they read records, chord tables and deck layers.
// Host half: every batch call of the C ABI is one CfRequest (contrib.hpp) -- profiles or parameter rows in, overrides,
// band rows or this block's sums out, host or device buffers -- and cf_run holds the module's one chunk loop: stage in,
// convert, run_sums / run_chunk on the chunk's view of the request (CfChunk), stage out.  capi.hip validates a request
// (kind, setup, step setup) before it gets here; nothing below repeats that.
// Every sum has a fixed order and no atomics: the bits do not depend on the batch a walker is in.  Not part of the
// per-step hot path: no kernel table, no run-time instantiation; molecule and CIA counts are run-time parameters.
#include "comm.hpp"
#include "contrib.hpp"
#include "integ.hpp"
#include "kernels.hpp"
#include "step.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace bartrt {

namespace {

constexpr int kCfRows = 16;   // layers per reduction block
constexpr int kCfPitch = 65;  // doubles per row of the LDS block (64 lanes + 1: rows start on different banks)

struct CfArgs {
  int L, M, C, W, nwalkers, ntiles, kind, nent;
  const double *kappa, *cia, *wn;
  const double *coef;
  const idx_t *idx;
  const int *kstop;
  const double *rdlp;      // [L] 1 / (ln p_k - ln p_{k-1}), k from the top ([0] unused)
  const double *rtop, *ds; // transit geometry: radii and chord table (prep_profiles, chord_table_fill)
  const int *tile_ptr;     // [ntiles + 1]: the tile's entries (one per overlapping filter, ascending)
  const double *wt;        // [nent][64]: the entry's weights h_i resp_i on the tile's lanes, 0 outside the window
  double *part;            // [nwalkers][nent][L]
  double *full;            // optional [nwalkers][W][L], atm layer order
};

// XCD-aware block -> (tile, walker) map (as the generic eclipse kernel's)
__device__ inline void cf_block_to_work(int b, int nwalkers, int &tile, int &walker) {
  const int xcd = b & 7, j = b >> 3;
  walker = j % nwalkers;
  tile = (j / nwalkers) * 8 + xcd;
}

// extinction of layer k for this lane: the generic kernels' table path (records in sC / sI)
__device__ __forceinline__ double cf_extinction(const CfArgs &p, const double *sC, const idx_t *sI, int k, int ii,
                                                double nu4) {
  const int M = p.M, C = p.C;
  const double *c = sC + (size_t)k * coef_stride(M, C);
  const idx_t *ix = sI + (size_t)k * idx_stride(C);
  double e = c[2 + 2 * M + 2 * C] * nu4 + c[3 + 2 * M + 2 * C];  // Rayleigh + grey cloud
  // grid [plane][W][M], CIA [pair plane][W][2] (kernels.hpp, "Table layout")
  const double *kb = reinterpret_cast<const double *>(reinterpret_cast<const char *>(p.kappa) + ix[0]) + (size_t)ii * M;
  const size_t MW = (size_t)M * p.W;
  for (int m = 0; m < M; m++) e += c[2 + 2 * m] * kb[m] + c[3 + 2 * m] * kb[MW + m];
  for (int cc = 0; cc < C; cc++) {
    const double *ab = reinterpret_cast<const double *>(reinterpret_cast<const char *>(p.cia) + ix[1 + cc]) + 2 * (size_t)ii;
    e += c[2 + 2 * M + 2 * cc] * ab[0] + c[3 + 2 * M + 2 * cc] * ab[1];
  }
  return e;
}

// Layers k0 .. k0 + nk - 1 are in blk[j][lane]: one partial per overlapping filter and layer, and the full output.
__device__ __forceinline__ void cf_flush(const CfArgs &p, const double *blk, int tile, int w, int k0, int nk) {
  __syncthreads();
  const int lane = threadIdx.x, j = lane & 15, q = lane >> 4;
  const int e1 = p.tile_ptr[tile + 1];
  for (int e = p.tile_ptr[tile]; e < e1; e++) {
    const double *wr = p.wt + (size_t)e * 64 + 16 * q;
    const double *row = blk + j * kCfPitch + 16 * q;
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < 16; t++) s = fma(row[t], wr[t], s);
    s += __shfl_xor(s, 16);   // (q0 + q1), (q2 + q3)
    s += __shfl_xor(s, 32);   // (q0 + q1) + (q2 + q3)
    if (q == 0 && j < nk) p.part[((size_t)w * p.nent + e) * p.L + k0 + j] = s;
  }
  if (p.full && j < nk) {
    const int L = p.L;
    double *out = p.full + (size_t)w * p.W * L + (L - 1 - (k0 + j));
    for (int r = q; r < 64; r += 4) {
      const int i = tile * 64 + r;
      if (i < p.W) out[(size_t)i * L] = blk[j * kCfPitch + r];
    }
  }
  __syncthreads();
}

template <int INTEG>
__global__ __launch_bounds__(64) void cf_eclipse(CfArgs p) {
  extern __shared__ double smem[];
  const int L = p.L, NC = coef_stride(p.M, p.C), NI = idx_stride(p.C);
  int tile, w;
  cf_block_to_work(blockIdx.x, p.nwalkers, tile, w);
  if (tile >= p.ntiles) return;
  double *sC = smem;
  idx_t *sI = reinterpret_cast<idx_t *>(smem + (size_t)L * NC);
  double *sW = smem + (size_t)L * NC + (size_t)L * NI;  // rule 1 only
  double *blk = sW + (INTEG == kIntegSimpson ? simpson_lds_doubles(L) : 0);
  stage2_to_lds(sC, p.coef + (size_t)w * L * NC, L * NC, sI, p.idx + (size_t)w * L * NI, L * NI, threadIdx.x, 64);
  __syncthreads();
  if (INTEG == kIntegSimpson) {
    simpson_radius_weights(sW, sC, NC, L, threadIdx.x, 64);
    __syncthreads();
  }
  const int i = tile * 64 + threadIdx.x;
  const bool valid = i < p.W;
  const int ii = valid ? i : p.W - 1;  // keep every lane's loads in range
  const double nu = p.wn[ii];
  const double bnum = 2.0 * kH * nu * nu * nu * kLS * kLS;
  const double nu4 = (nu * nu) * (nu * nu);
  const int kend = kstop_layer(p.kstop[w]);  // below it (a cloud deck) the optical depth repeats
  TauColumn<INTEG> tc;
  double Eprev = 1.0;
  for (int k = 0; k < L; k++) {
    if (k <= kend) tc.layer(k, true, 0.5, cf_extinction(p, sC, sI, k, ii, nu4), sC[(size_t)k * NC], sW);
    const double E = exp_rt(fmax(-tc.tau, kExpMin));
    double v = E;
    if (p.kind == kCfContrib) {
      const double B = bnum * rcp_n1(exp_rt(fmin(sC[(size_t)k * NC + 1] * nu, 700.0)) - 1.0);
      v = k == 0 ? 0.0 : B * (Eprev - E) * p.rdlp[k];
    }
    Eprev = E;
    blk[(k & (kCfRows - 1)) * kCfPitch + threadIdx.x] = valid ? v : 0.0;
    if ((k & (kCfRows - 1)) == kCfRows - 1 || k == L - 1) cf_flush(p, blk, tile, w, k & ~(kCfRows - 1), (k & (kCfRows - 1)) + 1);
  }
}

// STAGE: the layer records in LDS (without: read where they lie, for deep columns whose pair sums fill LDS)
template <bool STAGE>
__global__ __launch_bounds__(64) void cf_transit(CfArgs p) {
  extern __shared__ double smem[];
  const int L = p.L, NC = coef_stride(p.M, p.C), NI = idx_stride(p.C);
  int tile, w;
  cf_block_to_work(blockIdx.x, p.nwalkers, tile, w);
  if (tile >= p.ntiles) return;
  const double *gC = p.coef + (size_t)w * L * NC;
  const idx_t *gI = p.idx + (size_t)w * L * NI;
  const size_t nrec = STAGE ? (size_t)L * NC + (size_t)L * NI : 0;
  double *sP = smem + nrec;              // pair sums e_{j-1} + e_j, [L][64]
  double *blk = sP + (size_t)L * 64;
  const double *sC = gC;
  const idx_t *sI = gI;
  if constexpr (STAGE) {
    double *lC = smem;
    idx_t *lI = reinterpret_cast<idx_t *>(smem + (size_t)L * NC);
    stage2_to_lds(lC, gC, L * NC, lI, gI, L * NI, threadIdx.x, 64);
    __syncthreads();
    sC = lC;
    sI = lI;
  }
  const int i = tile * 64 + threadIdx.x;
  const bool valid = i < p.W;
  const int ii = valid ? i : p.W - 1;
  const double nu = p.wn[ii];
  const double nu4 = (nu * nu) * (nu * nu);
  const double *dsw = p.ds + (size_t)w * chord_table_size(L);
  const int kend = kstop_layer(p.kstop[w]);
  double eprev = 0.0, tau = 0.0;
  for (int k = 0; k < L; k++) {
    if (k <= kend) {
      const double e = cf_extinction(p, sC, sI, k, ii, nu4);
      if (k > 0) {
        sP[(size_t)k * 64 + threadIdx.x] = eprev + e;
        const double *dk = dsw + chord_table_index(L, k, 0);   // + (j / 4) * 64 + (j % 4) * 16 per layer j
        double t = 0.0;
        for (int j = 1; j <= k; j++) t = fma(sP[(size_t)j * 64 + threadIdx.x], dk[(j >> 2) * 64 + (j & 3) * 16], t);
        tau = t;
      }
      eprev = e;
    }
    blk[(k & (kCfRows - 1)) * kCfPitch + threadIdx.x] = valid ? exp_rt(fmax(-tau, kExpMin)) : 0.0;
    if ((k & (kCfRows - 1)) == kCfRows - 1 || k == L - 1) cf_flush(p, blk, tile, w, k & ~(kCfRows - 1), (k & (kCfRows - 1)) + 1);
  }
}

// sums[w][f][k] = sum over the filter's entries on this engine's block (tile order) of part[w][e][k]; 0 for a
// filter without a sample here.  Layers from the top, not divided.
__global__ __launch_bounds__(256) void cf_block_sums(const double *part, int nwalkers, int nf, int nent, int L,
                                                     const int *f_ptr, const int *f_ent, double *sums) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)nwalkers * nf * L) return;
  const int k = (int)(t % L);
  const int f = (int)((t / L) % nf);
  const int w = (int)(t / ((size_t)L * nf));
  double s = 0.0;
  for (int j = f_ptr[f]; j < f_ptr[f + 1]; j++) s += part[((size_t)w * nent + f_ent[j]) * L + k];
  sums[t] = s;
}

// band[w][f][L - 1 - k] = (sum over the ranks' slots, rank order, of slots[r][w][f][k]) / trapz(resp_f); NaN for a
// walker whose profile prep_profiles flagged (ok null: none is).  `slot` doubles from one rank's part to the next's.
__global__ __launch_bounds__(256) void cf_combine(const double *slots, int nranks, size_t slot, int nwalkers, int nf,
                                                  int L, const double *trapz, const unsigned char *ok, double *band) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)nwalkers * nf * L) return;
  const int k = (int)(t % L);
  const int f = (int)((t / L) % nf);
  const int w = (int)(t / ((size_t)L * nf));
  double s = 0.0;
  for (int r = 0; r < nranks; r++) s += slots[(size_t)r * slot + t];
  band[((size_t)w * nf + f) * L + (L - 1 - k)] = !ok || ok[w] ? s / trapz[f] : __builtin_nan("");
}

// Per-walker settings as the caller states them (what bartrt_set_radius / _set_cloudtop take: km, log10 bar) -> as
// prep_profiles reads them (cm, barye); NaN ("the engine's setting") stays NaN.  The device-buffer call's conversion:
// 10^x is the device's pow here and the host's in the setters and in the host-buffer call (over_units below) -- the
// two may differ in the last bit, which matters only to a cloud top that is a layer's pressure to the bit.
__global__ __launch_bounds__(256) void cf_over_units(const double *in, double *out, int n3) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n3) return;
  const int c = t % 3;
  const double v = in[t];
  out[t] = c == 0 ? v * 1e5 : (c == 1 ? pow(10.0, v) * 1e6 : v);
}

// After the preparation: a sample the step's converter rejected (status, optional) and a walker whose own radius
// (over, optional, prep_profiles' units) is not a positive finite number -- bartrt_set_radius refuses such a value --
// are flagged like a profile the preparation cannot evaluate.
__global__ __launch_bounds__(256) void cf_mask(const int *status, const double *over, unsigned char *ok, int n) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= n) return;
  bool bad = status && status[w] != 0;
  if (over) {
    const double r = over[3 * (size_t)w];
    bad = bad || (r == r && !(r > 0.0 && r < 1e300));
  }
  if (bad) ok[w] = 0;
}

}  // namespace

// ---- host state of one engine (Engine::cf; made by cf_setup): the per-walker workspaces of one chunk of walkers ----
struct CfWork {
  int cap = 0;
  RecordSet rec;
  DevBuf<double> d_rtop, d_ds, d_part;
  DevBuf<double> d_sums;              // [cap][nf][L]: the block's band sums where no receive buffer takes them
  // per-walker overrides in prep_profiles' units [cap_over][3]; the parameter front end's profiles [cap_par][nprof]
  // and statuses
  int cap_over = 0, cap_par = 0;
  DevBuf<double> d_over, d_prof;
  DevBuf<int> d_status;
  DevBuf<char> d_stage;               // staging of the host-buffer call
  hipStream_t last_stream = nullptr;  // the workspaces' latest user
  // the latest chunk as bartrt_cf_get_records reports it: its walkers (0: none since the latest setup, or its launch
  // was refused), where its flags lie, the kernel form and the dynamic LDS of its launch
  int seen_n = 0, seen_form = kCfFormEclipse;
  size_t seen_lds = 0;
  const unsigned char *seen_ok = nullptr;
};
struct CfState : CfWork {   // ... and the filter tables
  int nf = 0, ntiles = 0, nent = 0;
  int nent_bound = 0;   // at least any block's entry count, from the windows alone: the same on every rank
  DevBuf<int> d_tile_ptr, d_f_ptr, d_f_ent;
  DevBuf<double> d_wt, d_trapz, d_rdlp;
};

namespace {

// Bytes of the workspaces (partials, layer records, chord tables) a chunk may hold: BARTRT_CF_WORKSPACE_BYTES,
// default 256 MiB.  Read per call.
size_t workspace_cap() {
  const char *c = std::getenv("BARTRT_CF_WORKSPACE_BYTES");
  return c && *c ? std::max<size_t>(1, std::strtoull(c, nullptr, 10)) : (size_t)256 << 20;
}

// (over: the chunk holds per-walker overrides; params: and the converter's profiles and statuses)
size_t per_walker_bytes(const Engine &e, bool over, bool params) {
  const CfState &g = *e.cf;
  // (nothing here depends on the engine's block: ranks that make the same call cut it into the same chunks)
  size_t b = sizeof(double) * ((size_t)g.nent_bound + g.nf) * e.L + sizeof(double) * (size_t)e.L * coef_stride(e.M, e.C) +
             sizeof(idx_t) * (size_t)e.L * idx_stride(e.C) + sizeof(int) + 1;
  if (e.solution == 1) b += sizeof(double) * ((size_t)e.L + chord_table_size(e.L));
  if (over || params) b += sizeof(double) * 3;
  if (params) b += sizeof(double) * (size_t)(e.S + 1) * e.L + sizeof(int);
  return b;
}

// a stream other than the previous call's may not reuse the workspaces while that call still runs
void claim(CfState &g, hipStream_t st) {
  if (g.last_stream && g.last_stream != st) HIPCHK(hipStreamSynchronize(g.last_stream));
  g.last_stream = st;
}

void ensure_cap(const Engine &e, int n, bool over, bool params) {
  CfState &g = *e.cf;
  over = over || params;
  if (n <= g.cap && (!over || n <= g.cap_over) && (!params || n <= g.cap_par)) return;
  HIPCHK(hipDeviceSynchronize());   // (an earlier launch on any stream may still use the old buffers)
  if (n > g.cap) {
    g.rec.reserve((size_t)n, e.L, e.M, e.C);
    g.d_part.reserve((size_t)n * g.nent * e.L);
    g.d_sums.reserve((size_t)n * g.nf * e.L);
    if (e.solution == 1) {
      g.d_rtop.reserve((size_t)n * e.L);
      g.d_ds.reserve((size_t)n * chord_table_size(e.L));
    }
    g.cap = n;
  }
  if (over && n > g.cap_over) {
    g.d_over.reserve((size_t)n * 3);
    g.cap_over = n;
  }
  if (params && n > g.cap_par) {
    g.d_prof.reserve((size_t)n * (e.S + 1) * e.L);
    g.d_status.reserve((size_t)n);
    g.cap_par = n;
  }
}

// One chunk of a request as the kernels see it: m walkers, every pointer the device's and already at the chunk.
struct CfChunk {
  int m, kind;
  const double *prof;     // [m][(S+1) L]
  const double *over;     // [m][3] in prep_profiles' units (cm, barye, Rayleigh value; NaN: the engine's), or null
  bool check_radius;      // the radii in `over` are checked on the device (cf_mask); false: the host has refused bad ones
  const int *status;      // [m] the converter's verdicts, or null: a rejected sample's flag is cleared
  double *out;            // [m][nf][L] band rows (run_chunk)
  double *full;           // [m][W][L] or null
  unsigned char *ok;      // [m] flags, never null
  hipStream_t st;
};

// the CF kernel of this engine's geometry and rule, with the dynamic LDS it needs (above 64 kB: asked for first)
template <class K>
void launch_cf(K kernel, size_t lds, int nblocks, hipStream_t st, const CfArgs &a) {
  if (lds > 160 * 1024) throw std::invalid_argument("cf: the column's layer records and sums do not fit in LDS (160 kB)");
  if (lds > 64 * 1024)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(64), lds, st, a);
}

// one chunk up to this engine's band sums d_sums [m][nf][L] (cf_block_sums, not divided)
void run_sums(Engine &e, const CfChunk &c, double *d_sums) {
  CfState &g = *e.cf;
  const int m = c.m;
  g.seen_n = 0;
  hipStream_t st = c.st;
  // the layer records under the engine's settings, as run_transit_batch builds them, into this module's buffers
  // (no radii output, only the caller's own per-walker overrides: the engine's own state is left as it was)
  PrepArgs pa = e.prep_args(RunRequest(c.prof, m, nullptr, c.ok, st), g.rec);
  pa.rad_out = nullptr;
  pa.over = c.over;
  pa.rtop = e.solution == 1 ? g.d_rtop.get() : nullptr;
  pa.ds = e.solution == 1 ? g.d_ds.get() : nullptr;
  HIPCHK(launch_prep(pa, st));
  // (transit: the radii the preparation wrote are the walker's own -- hydrostatic from ITS reference radius -- and so
  // is the chord table filled from them)
  if (e.solution == 1) HIPCHK(launch_chord_table(pa, st));
  const double *radii = c.check_radius ? c.over : nullptr;
  if (c.status || radii) {
    hipLaunchKernelGGL(cf_mask, dim3((m + 255) / 256), dim3(256), 0, st, c.status, radii, c.ok, m);
    HIPCHK(hipGetLastError());
  }

  CfArgs a{};
  a.L = e.L; a.M = e.M; a.C = e.C; a.W = e.W(); a.nwalkers = m; a.ntiles = g.ntiles; a.kind = c.kind; a.nent = g.nent;
  a.kappa = e.rt.kappa; a.cia = e.rt.cia; a.wn = e.rt.wn;
  a.coef = g.rec.coef; a.idx = g.rec.idx; a.kstop = g.rec.kstop;
  a.rdlp = g.d_rdlp;
  a.rtop = g.d_rtop; a.ds = g.d_ds;
  a.tile_ptr = g.d_tile_ptr; a.wt = g.d_wt;
  a.part = g.d_part; a.full = c.full;
  const int nblocks = (g.ntiles + 7) / 8 * 8 * m;
  const size_t L = e.L, NC = coef_stride(e.M, e.C), NI = idx_stride(e.C), blk = (size_t)kCfRows * kCfPitch;
  if (e.solution == 1) {
    const size_t with = sizeof(double) * (L * NC + L * NI + L * 64 + blk), without = sizeof(double) * (L * 64 + blk);
    g.seen_form = with <= 160 * 1024 ? kCfFormStaged : kCfFormUnstaged;
    g.seen_lds = with <= 160 * 1024 ? with : without;
    if (with <= 160 * 1024) launch_cf(cf_transit<true>, with, nblocks, st, a);
    else launch_cf(cf_transit<false>, without, nblocks, st, a);
  } else {
    const size_t base = sizeof(double) * (L * NC + L * NI + blk);
    const size_t simp = base + sizeof(double) * simpson_lds_doubles(e.L);
    g.seen_form = kCfFormEclipse;
    g.seen_lds = e.integ == kIntegSimpson ? simp : base;
    switch (e.integ) {
      case kIntegTransmittance: launch_cf(cf_eclipse<kIntegTransmittance>, base, nblocks, st, a); break;
      case kIntegSimpson: launch_cf(cf_eclipse<kIntegSimpson>, simp, nblocks, st, a); break;
      default: launch_cf(cf_eclipse<kIntegTrapzTau>, base, nblocks, st, a); break;
    }
  }
  HIPCHK(hipGetLastError());
  const size_t nout = (size_t)m * g.nf * e.L;
  hipLaunchKernelGGL(cf_block_sums, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, g.d_part, m, g.nf, g.nent,
                     e.L, g.d_f_ptr, g.d_f_ent, d_sums);
  HIPCHK(hipGetLastError());
  g.seen_n = m;
  g.seen_ok = c.ok;
}

void combine(const Engine &e, const double *d_slots, int nranks, size_t slot, int m, const unsigned char *okp,
             double *d_band, hipStream_t st) {
  const CfState &g = *e.cf;
  const size_t nout = (size_t)m * g.nf * e.L;
  hipLaunchKernelGGL(cf_combine, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, d_slots, nranks, slot, m, g.nf,
                     e.L, g.d_trapz, okp, d_band);
  HIPCHK(hipGetLastError());
}

// one chunk, band rows out.  With a communicator: the sums go into this rank's slot of its receive buffer, one
// in-place all-gather on c.st (every rank makes the same call: m is the same everywhere), the slots combined in rank
// order.  Without one the engine holds the whole grid and its sums are the only slot.
void run_chunk(Engine &e, const CfChunk &c) {
  const CfState &g = *e.cf;
  const size_t count = (size_t)c.m * g.nf * e.L;
  if (Comm *cm = e.comm) {
    double *recv = comm_recv(*cm, count * cm->nranks);
    run_sums(e, c, recv + (size_t)cm->rank * count);
    comm_allgather_inplace(*cm, recv, count, c.st);
    e.ncollectives++;   // (one per chunk: bartrt_get_comm reports it)
    combine(e, recv, cm->nranks, count, c.m, c.ok, c.out, c.st);
    return;
  }
  // The backstop: capi.hip answers the combining calls on a sharded engine without a communicator with BARTRT_ENOTSUP
  // before they get here; rq.partials (run_sums alone) is served on such an engine.
  if (e.lo != 0 || e.hi != e.Wfull) throw std::invalid_argument("cf: a sharded engine needs a communicator (bartrt_comm_init)");
  run_sums(e, c, g.d_sums);
  combine(e, g.d_sums, 1, count, c.m, c.ok, c.out, c.st);
}

// samples per row of `full` as the chunk size counts them: the largest block under a communicator (the same on
// every rank), else this engine's own
size_t full_rows(const Engine &e) { return e.comm ? step_block_max(e.Wfull, e.comm->nranks) : (size_t)e.W(); }

}  // namespace

void cf_setup(Engine &e, int nf, const int *idx0, const int *npts, const double *resp) {
  if (nf < 1 || !idx0 || !npts || !resp) throw std::invalid_argument("cf_setup: no filters");
  // the engine's block [lo, hi) of the grid (the whole grid on an unsharded engine): tiles count from lo
  const int Wfull = e.Wfull, lo = e.lo, hi = e.hi, L = e.L;
  std::vector<double> trapz(nf);
  std::vector<size_t> off(nf + 1, 0);
  for (int f = 0; f < nf; f++) {
    if (npts[f] < 2 || idx0[f] < 0 || (long)idx0[f] + npts[f] > Wfull)
      throw std::invalid_argument("cf_setup: filter " + std::to_string(f) + " needs a window of at least two samples inside the grid");
    off[f + 1] = off[f] + npts[f];
  }
  // trapz(resp) with unit spacing (np.trapz without x): half weights at the window's ends -- its true ends on the
  // full grid; where the block cuts a window the cut sample keeps weight 1 -- and the whole window's sum on every rank
  auto weight = [&](int f, int s) { return (s == 0 || s == npts[f] - 1 ? 0.5 : 1.0) * resp[off[f] + s]; };
  for (int f = 0; f < nf; f++) {
    double t = 0.0;
    for (int s = 0; s + 1 < npts[f]; s++) t += 0.5 * (resp[off[f] + s] + resp[off[f] + s + 1]);
    if (!std::isfinite(t) || t == 0.0)
      throw std::invalid_argument("cf_setup: filter " + std::to_string(f) + " has no response inside the grid");
    trapz[f] = t;
  }
  const int ntiles = (hi - lo + 63) / 64;
  std::vector<int> tile_ptr(ntiles + 1, 0), ent_f;
  std::vector<double> wt;
  for (int t = 0; t < ntiles; t++) {
    const int t0 = lo + 64 * t, t1 = std::min(t0 + 64, hi);   // the tile's samples on the full grid
    for (int f = 0; f < nf; f++) {
      const int a = std::max(idx0[f], t0), b = std::min(idx0[f] + npts[f], t1);
      if (a >= b) continue;
      ent_f.push_back(f);
      const size_t at = wt.size();
      wt.resize(at + 64, 0.0);
      for (int i = a; i < b; i++) wt[at + (i - t0)] = weight(f, i - idx0[f]);
    }
    tile_ptr[t + 1] = (int)ent_f.size();
  }
  const int nent = (int)ent_f.size();
  // a window of n samples meets at most (n - 1) / 64 + 2 <= n / 64 + 2 tiles, wherever the tiles start
  long bound = 0;
  for (int f = 0; f < nf; f++) bound += npts[f] / 64 + 2;
  std::vector<int> f_ptr(nf + 1, 0), f_ent;
  for (int f = 0; f < nf; f++) {
    for (int j = 0; j < nent; j++)
      if (ent_f[j] == f) f_ent.push_back(j);   // entries are tile-major: ascending j is tile order
    f_ptr[f + 1] = (int)f_ent.size();
  }
  // 1 / (ln p_k - ln p_{k-1}), k from the top (cf_eq's d_logp, code/cf.py:130)
  std::vector<double> rdlp(L, 0.0);
  for (int k = 1; k < L; k++) rdlp[k] = 1.0 / (std::log(e.atm.press[L - 1 - k]) - std::log(e.atm.press[L - k]));

  HIPCHK(hipDeviceSynchronize());   // (a CF launch may still read the old tables)
  std::unique_ptr<CfState> old(std::exchange(e.cf, nullptr)), g(new CfState());
  g->d_tile_ptr.upload(tile_ptr);
  g->d_f_ptr.upload(f_ptr);
  g->d_f_ent.upload(f_ent);
  g->d_wt.upload(wt);
  g->d_trapz.upload(trapz);
  g->d_rdlp.upload(rdlp);
  g->nf = nf; g->nent = nent; g->ntiles = ntiles; g->nent_bound = (int)std::min<long>(bound, INT_MAX);
  // an earlier setup's workspaces stay unless the entry or filter count changes (they size the partials and the
  // sums); its tables go with `old`
  if (old && old->nent == nent && old->nf == nf) static_cast<CfWork &>(*g) = std::move(*old);
  g->seen_n = 0;   // (no chunk has run under these tables)
  e.cf = g.release();
}

int cf_nfilters(const Engine &e) { return e.cf ? e.cf->nf : 0; }

CfSeen cf_seen(const Engine &e) {
  CfSeen s;
  if (const CfState *g = e.cf) {
    s.n = g->seen_n; s.nf = g->nf; s.ntiles = g->ntiles; s.nent = g->nent;
    s.form = g->seen_form; s.lds = g->seen_lds;
  }
  return s;
}

void cf_get_records(Engine &e, int walker, const CfReadback &o) {
  CfState &g = *e.cf;
  if (g.seen_n <= 0) throw std::invalid_argument("cf_get_records: no contribution-function call has run since the latest setup");
  if (walker < 0 || walker >= g.seen_n)
    throw std::invalid_argument("cf_get_records: walker " + std::to_string(walker) + " is outside the latest chunk of " +
                                std::to_string(g.seen_n));
  const size_t L = (size_t)e.L, NC = (size_t)coef_stride(e.M, e.C), NI = (size_t)idx_stride(e.C), w = (size_t)walker;
  HIPCHK(hipStreamSynchronize(g.last_stream));
  auto get = [](void *dst, const void *src, size_t bytes) {
    if (dst && bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
  };
  get(o.coef, g.rec.coef.get() + w * L * NC, sizeof(double) * L * NC);
  get(o.idx, g.rec.idx.get() + w * L * NI, sizeof(idx_t) * L * NI);
  get(o.kstop, g.rec.kstop.get() + w, sizeof(int));
  get(o.ok, g.seen_ok + w, 1);   // (the module's own buffer, its staging, or the caller's device buffer: alive still)
  get(o.rdlp, g.d_rdlp.get(), sizeof(double) * L);
  if (e.solution == 1) {
    get(o.rtop, g.d_rtop.get() + w * L, sizeof(double) * L);
    get(o.ds, g.d_ds.get() + w * chord_table_size(e.L), sizeof(double) * chord_table_size(e.L));
  }
  get(o.tile_ptr, g.d_tile_ptr.get(), sizeof(int) * ((size_t)g.ntiles + 1));
  get(o.f_ptr, g.d_f_ptr.get(), sizeof(int) * ((size_t)g.nf + 1));
  get(o.f_ent, g.d_f_ent.get(), sizeof(int) * (size_t)g.nent);
  get(o.wt, g.d_wt.get(), sizeof(double) * (size_t)g.nent * 64);
  get(o.trapz, g.d_trapz.get(), sizeof(double) * (size_t)g.nf);
}

void cf_combine_dev(Engine &e, const double *d_slots, int nranks, int n, const unsigned char *d_ok, double *d_band,
                    hipStream_t st) {
  if (nranks < 1 || nranks > e.Wfull) throw std::invalid_argument("cf_combine: nranks must lie in [1, the grid's sample count]");
  if (n <= 0) return;
  combine(e, d_slots, nranks, (size_t)n * e.cf->nf * e.L, n, d_ok, d_band, st);
}

namespace {

// Host buffers are staged chunk by chunk in one allocation: consecutive arrays of `chunk` rows each.
struct Staging {
  char *base = nullptr;
  size_t at = 0;
  int chunk = 0;
  template <class T> T *take(size_t bytes_per_row) {
    T *p = reinterpret_cast<T *>(base + at);
    at += (size_t)chunk * bytes_per_row;
    return p;
  }
};

}  // namespace

void cf_run(Engine &e, const CfRequest &rq) {
  const int n = rq.n;
  if (n <= 0) return;
  const bool host = rq.host, params = rq.from_params, over = rq.over && !params;
  // Host-buffer profile calls refuse a bad radius as bartrt_set_radius does, naming the walker, before any launch;
  // device buffers cannot be read here: cf_mask flags such a walker instead.
  if (host && over)
    for (int w = 0; w < n; w++) {
      const double r = rq.over[3 * (size_t)w];
      if (r == r && !(r > 0 && r < 1e295))
        throw std::invalid_argument("cf: walker " + std::to_string(w) + "'s radius must be positive");
    }
  CfState &g = *e.cf;
  hipStream_t st = host ? e.stream : rq.stream;
  const size_t nin = params ? (size_t)rq.npars : (size_t)(e.S + 1) * e.L, nband = (size_t)g.nf * e.L,
               nfull = (size_t)e.W() * e.L;
  // Chunk size: what the cap leaves for a walker's workspaces plus, for host buffers, its staged rows -- input, band
  // row, `full` counted at the LARGEST block's samples under a communicator (full_rows), the flag or status.  Nothing
  // in it depends on this engine's block, so ranks that make the same call cut it identically and issue the same
  // number of collectives (one per chunk).
  const size_t bin = sizeof(double) * nin, bband = sizeof(double) * nband,
               bfull_max = rq.full ? sizeof(double) * full_rows(e) * e.L : 0, bflag = params ? sizeof(int) : 1,
               brow = host ? bin + bband + bfull_max + bflag : 0;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>(n, workspace_cap() / (per_walker_bytes(e, over, params) + brow)));
  // Order kept: the workspaces grow (a device-wide synchronize if they do: an earlier launch on any stream may still
  // use the old ones), then the staging buffer likewise, then the stream claims them.  Workspaces that fit stay, also
  // across a cf_setup with equal entry and filter counts.
  ensure_cap(e, chunk, over, params);
  Staging s;
  s.chunk = chunk;
  if (host && (size_t)chunk * brow > g.d_stage.count()) {
    HIPCHK(hipDeviceSynchronize());
    g.d_stage.reserve((size_t)chunk * brow);
  }
  claim(g, st);
  s.base = g.d_stage;
  double *din = nullptr, *dband = nullptr, *dfull = nullptr;
  unsigned char *dok = nullptr;
  int *dstatus = nullptr;
  std::vector<unsigned char> hok;
  std::vector<double> hov;
  if (host) {
    din = s.take<double>(bin);
    dband = s.take<double>(bband);
    if (rq.full) dfull = s.take<double>(bfull_max);
    if (params) dstatus = s.take<int>(sizeof(int));
    else dok = s.take<unsigned char>(1);
    hok.resize(params ? 0 : chunk);
    hov.resize(over ? (size_t)3 * chunk : 0);
  }
  // the module's one chunk loop
  for (int off = 0; off < n; off += chunk) {
    const int m = std::min(chunk, n - off);
    const double *in = rq.in + (size_t)off * nin;
    if (host) {
      HIPCHK(hipMemcpyAsync(din, in, bin * m, hipMemcpyHostToDevice, st));
      in = din;
    }
    CfChunk c{};
    c.m = m; c.kind = rq.kind; c.st = st;
    c.out = host ? dband : rq.out + (size_t)off * nband;
    c.full = !rq.full ? nullptr : host ? dfull : rq.full + (size_t)off * nfull;
    if (params) {
      // the converter's overrides are in the preparation's units as written; cf_mask clears a rejected sample's flag
      // (and checks the radius): the sample is reported through status, never an error
      int *status = host ? dstatus : rq.status ? rq.status + off : g.d_status.get();
      step_convert_dev(e, in, m, rq.npars, g.d_prof, status, g.d_over, st);
      c.prof = g.d_prof; c.over = g.d_over; c.status = status; c.ok = g.rec.ok; c.check_radius = true;
    } else {
      c.prof = in;
      c.ok = host ? dok : rq.ok ? rq.ok + off : g.rec.ok.get();
      c.check_radius = !host;
      if (over && host) {
        // converted here with the setters' own arithmetic (capi.hip: km -> cm, log10 bar -> barye; NaN stays NaN),
        // so a walker's deck is the layer the setter would give it
        for (int w = 0; w < m; w++) {
          const double *o = rq.over + 3 * (size_t)(off + w);
          hov[3 * w] = o[0] * 1e5;
          hov[3 * w + 1] = std::pow(10.0, o[1]) * 1e6;
          hov[3 * w + 2] = o[2];
        }
        HIPCHK(hipMemcpyAsync(g.d_over, hov.data(), sizeof(double) * 3 * m, hipMemcpyHostToDevice, st));
        c.over = g.d_over;
      } else if (over) {
        // converted on the device (cf_over_units: the device's pow); cf_mask flags a bad radius
        hipLaunchKernelGGL(cf_over_units, dim3((3 * m + 255) / 256), dim3(256), 0, st, rq.over + (size_t)3 * off,
                           g.d_over.get(), 3 * m);
        HIPCHK(hipGetLastError());
        c.over = g.d_over;
      }
    }
    if (rq.partials) run_sums(e, c, c.out);
    else run_chunk(e, c);
    if (!host) continue;
    HIPCHK(hipMemcpyAsync(rq.out + (size_t)off * nband, dband, bband * m, hipMemcpyDeviceToHost, st));
    if (rq.full) HIPCHK(hipMemcpyAsync(rq.full + (size_t)off * nfull, dfull, sizeof(double) * nfull * m, hipMemcpyDeviceToHost, st));
    if (params && rq.status) HIPCHK(hipMemcpyAsync(rq.status + off, dstatus, sizeof(int) * m, hipMemcpyDeviceToHost, st));
    if (!params) HIPCHK(hipMemcpyAsync(hok.data(), dok, (size_t)m, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // (the one wait per chunk: the staging rows, hov and hok are free again)
    if (params) continue;
    // a profile call without `ok` fails on a flagged profile
    if (rq.ok) std::copy(hok.begin(), hok.begin() + m, rq.ok + off);
    else
      for (int w = 0; w < m; w++)
        if (!hok[w]) throw std::invalid_argument("cf: profile " + std::to_string(off + w) + " holds a non-finite or non-positive temperature");
  }
}

void cf_release(Engine &e) {
  delete e.cf;
  e.cf = nullptr;
}

}  // namespace bartrt
