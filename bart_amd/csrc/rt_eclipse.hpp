// Specialised eclipse kernels (compile-time ray-angle / molecule / CIA counts and
// integration rule): device code only -- this text is also what hiprtc compiles at run time (rtc.hpp).  Which unit
// instantiates which kernel, and which launch takes which: rt_launch.hpp.
//
//  rt_eclipse_fast   one lane per (walker, wavenumber) walks the layers from the
//                    top: buffer loads with scalar plane offsets, two pairs of
//                    register slots in flight, layer records from LDS.
//  rt_eclipse_split  5-8 walkers: producer / consumer wave pair per column.
//  rt_eclipse_quad   1-4 walkers: 16 wavenumbers x 4 layers (or 8 x 8) per wave
//                    and step, the optical depth by a lane-row prefix scan.
//
// INTEG: the integration rule (integ.hpp).  Rule 1 is the default and what the bench
// runs; its single-wave walk is its own kernel (rt_eclipse_s1.hpp, rt_eclipse_s1s.hpp for
// the per-angle `cut slant`); rules 0 and 2 are the walks below with their accumulators.
#pragma once
#include "integ.hpp"
#include "kernels.hpp"
#include "prep.hpp"

#ifndef __HIPCC_RTC__
#include <cmath>
#include <type_traits>
#endif

// upper bound on resident waves per SIMD the specialised kernels are compiled
// for: lets the compiler spend registers on loads in flight (measured best: 3-4)
#ifndef BARTRT_WPE
#define BARTRT_WPE 4
#endif

namespace bartrt {

// SCHED of rt_eclipse_simpson_slant (rt_eclipse_s1s.hpp) by shape: the record read-ahead up to twelve table loads per
// layer, none beyond (rt_eclipse_slant_ilp.hip) -- a template argument of the ahead-of-time builds and of the ids the
// launchers ask for (rt_launch.hpp)
constexpr int slant_sched(int M, int C, int dflt) { return 2 * M + 2 * C > 12 ? 0 : dflt; }

// ---------------------------------------------------------------------------
// XCD-aware block -> (tile, walker) map.  Blocks b and b+8 share an XCD (and
// its L2), so all walkers of one wavenumber tile are placed on one XCD, walker
// index fastest: they stream the same grid rows at about the same time and
// the XCD's L2 serves the repeats.
__device__ inline void block_to_work(int b, int nwalkers, int &tile, int &walker) {
  const int xcd = b & 7, j = b >> 3;
  walker = j % nwalkers;
  tile = (j / nwalkers) * 8 + xcd;
}

// LDS beyond the layer records: rule 1 keeps the Simpson weights of the radius grid (three
// words per layer in the producer / consumer and quad-layer kernels, four in rt_eclipse_simpson)
template <int INTEG>
__host__ __device__ inline size_t integ_lds_doubles(int L) {
  return INTEG == kIntegSimpson ? 4 * (size_t)(L + kSimpsonPad) : 0;
}

// Specialised kernel: compile-time angle / molecule / CIA counts, scalar row
// bases (SGPR) + one 32-bit lane offset for every load, and two pairs of
// register slots of 2M+2C loads kept in flight ahead of the arithmetic, so that
// the one or two waves a SIMD holds at small batch sizes cover the HBM latency
// by themselves.
// SQ: the last ray angle has exactly half the cosine of the first (launch_rt
// orders them so; 0 and 60 degrees of the usual raygrid), so its transmittance
// is the first one's square: exp(-2 tau / mu) = exp(-tau / mu)^2 -- one
// multiplication instead of one of the six exponentials of a layer.
// SCHED only names the instantiation: SCHED = 1 is compiled in its own translation
// unit (rt_eclipse_i0_ilp.hip) under the compiler's maximum-ILP scheduling strategy.
// The default (maximum-occupancy) schedule lays the A + 1 exponentials' Horner
// chains out one after the other -- nine dependent fp64 FMAs in a row, five times
// -- which a SIMD with three resident waves hides and a SIMD with one or two does
// not; the ILP schedule keeps the chains interleaved as written, at 211 instead of
// 138 VGPRs (two resident waves per SIMD instead of three).  Measured on the bench
// grid: 10 walkers 75 -> 71 us, 16: 113 -> 107, 64: 326 -> 324, 256: 1062 -> 1082;
// launch_rt_spec (rt_launch.hpp) takes the ILP build below kIlpMaxColumns columns.
// EXT: the line-by-line path's hand-off -- the layer's line extinction ext[w][l][W]
// (atm layer order) is one more coalesced 8-byte load per layer and one more addend
// (line-by-line engines have no table: MT = 0).
// SLANT: the `toomuch` cut on each ray's slant depth (cfg `cut slant`): the rays' terms are masked
// one by one (ColumnFluxSlant, integ.hpp) and the column is walked while its longest-lived ray is alive.
template <int AT, int MT, int CT, bool SQ, int INTEG, int SCHED = 0, bool EXT = false, bool SLANT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, BARTRT_WPE)))
void rt_eclipse_fast(RtArgs p) {
  extern __shared__ double smem[];
  constexpr int A = AT, M = MT, C = CT;
  constexpr int NC = 4 + 2 * M + 2 * C, NI = 1 + C, NLD = 2 * M + 2 * C;
  constexpr int NR = NLD + (EXT ? 1 : 0) > 0 ? NLD + (EXT ? 1 : 0) : 1;
  const int L = p.L, W = p.W;
  int bid = blockIdx.x;
  if (p.nprep > 0) {   // the head of the grid prepares the NEXT batch's layer records (RtArgs::nprep)
    if (bid < p.nprep) { prep_block(p.prep_next, bid, smem); return; }
    bid -= prep_slots(p.nprep);
    if (bid < 0) return;
  }
  int tile, w;
  block_to_work(bid, p.nwalkers, tile, w);
  if (tile >= p.ntiles) return;

  double *sC = smem;
  idx_t *sI = reinterpret_cast<idx_t *>(smem + (size_t)L * NC);
  const double *sW = smem + (size_t)L * NC + (size_t)L * NI;  // rule 1 only
  {
    const double *gC = p.coef + (size_t)w * L * NC;
    const idx_t *gI = p.idx + (size_t)w * L * NI;
    stage2_to_lds(sC, gC, L * NC, sI, gI, L * NI, threadIdx.x, blockDim.x);
  }
  __syncthreads();
  if (INTEG == kIntegSimpson) {
    simpson_radius_weights(const_cast<double *>(sW), sC, NC, L, threadIdx.x, blockDim.x);
    __syncthreads();
  }

  const int i = tile * blockDim.x + threadIdx.x;
  const bool valid = i < W;
  const unsigned ii = valid ? (unsigned)i : (unsigned)(W - 1);
  const double nu = p.wn[ii];
  const double bnum = 2.0 * kH * nu * nu * nu * kLS * kLS;
  const double nu4 = (nu * nu) * (nu * nu);
  const TableLoader<M, C> tab(p, ii, sI);
  const double *extw = EXT ? p.ext + (size_t)w * L * W + ii : nullptr;
  auto load_layer = [&](int k, double (&r)[NR]) {
    tab.load(k, r);
    if (EXT) r[NLD] = extw[(size_t)(L - 1 - k) * W];
  };

  TauColumn<INTEG> tc;
  std::conditional_t<SLANT, ColumnFluxSlant<INTEG, A>, ColumnFlux<INTEG, A>> ci(p);
  double Bprev = 0.0;
  bool active = true;
  const int kraw = p.kstop[w], kend = kstop_layer(kraw);
  const bool deck_on = kstop_deck(kraw);
  const double tcap = tau_cap(p, A);
  // the optical depth that ends the lane's walk: toomuch itself, or (SLANT) the threshold of the ray that goes last
  double tstop = p.toomuch;
  if constexpr (SLANT) {
    tstop = p.thr[0];
#pragma unroll
    for (int a = 1; a < A; a++) tstop = p.thr[a] > tstop ? p.thr[a] : tstop;
  }

  // One layer's arithmetic.  Straight-line: layer indices past the end are
  // clamped and masked instead of branched around, so that inside an unrolled
  // block the compiler waits (counted vmcnt) on exactly the loads a layer
  // needs and leaves the younger ones in flight.
  // The record of a layer is read from LDS one layer ahead (cf / cfn alternate
  // between two register sets), so its latency is not waited out at the head of
  // the layer that uses it; masking by multiplication keeps the reads of the
  // path length and of c2/T out of conditional blocks.
  auto read_rec = [&](int k, double (&cf)[NC]) {
    const double *c = sC + (k < kend ? k : kend) * NC;
#pragma unroll
    for (int j = 0; j < NC; j++) cf[j] = c[j];
  };
  auto layer = [&](int k, const double (&r)[NR], const double (&cf)[NC], double (&cfn)[NC]) {
    const bool live = active && k <= kend;
    read_rec(k + 1, cfn);
    const double lv = live ? 0.5 : 0.0;
    double e = fma(cf[2 + 2 * M + 2 * C], nu4, cf[3 + 2 * M + 2 * C]);   // Rayleigh + grey cloud
#pragma unroll
    for (int j = 0; j < NLD; j++) e = fma(cf[2 + j], r[j], e);
    if (EXT) e += r[NLD];
    tc.layer(k, live, lv, e, cf[0], sW);
    // Planck exponent and the A slant-path exponents in one interleaved batch
    const double tcl = fmin(tc.tau, tcap);
    constexpr int AE = SQ ? A - 1 : A;  // transmittances that need an exponential
    double xs[AE + 1], ex[AE + 1], es[A];
    xs[AE] = fmin(cf[1] * nu, 700.0);
#pragma unroll
    for (int a = 0; a < AE; a++) xs[a] = -tcl * p.invmu[a];
    exp_rt_n<AE + 1>(xs, ex);
#pragma unroll
    for (int a = 0; a < AE; a++) es[a] = ex[a];
    if (SQ) es[A - 1] = ex[0] * ex[0];
    const double B = bnum * rcp_n1(ex[AE] - 1.0);
    ci.layer(p, A, live, lv, tc.tau, Bprev, B, es);
    Bprev = SLANT ? (live ? B : Bprev) : B;
    active = active && !(live && tc.tau > tstop);
  };
  auto clampk = [&](int k) { return k < kend ? k : kend; };

  // two pairs of slots; each pair is reloaded two layers before it is used and
  // the loads that cross the loop's back edge were issued two layers earlier
  double a0[NR], a1[NR], b0[NR], b1[NR];
  load_layer(clampk(0), a0);
  load_layer(clampk(1), a1);
  double cfE[NC], cfO[NC];
  read_rec(0, cfE);
  int k0 = 0;
  for (; k0 <= kend; k0 += 4) {
    load_layer(clampk(k0 + 2), b0);
    load_layer(clampk(k0 + 3), b1);
    layer(k0, a0, cfE, cfO);
    layer(k0 + 1, a1, cfO, cfE);
    load_layer(clampk(k0 + 4), a0);
    load_layer(clampk(k0 + 5), a1);
    layer(k0 + 2, b0, cfE, cfO);
    layer(k0 + 3, b1, cfO, cfE);
    if (!__any(active)) break;
  }
  const double F = ci.flux(p, A, SLANT ? deck_on : (deck_on && active), Bprev, L);
  if (valid) p.spec[(size_t)w * W + i] = F;
  if (p.walked_out && threadIdx.x == 0)  // diagnostics: layers this wave walked (bench.py's byte model)
    p.walked_out[(size_t)w * p.ntiles + tile] = (k0 + 4 < kend + 1 ? k0 + 4 : kend + 1);
}

// Few-walker variant (5-8 walkers at W = 1e4; below that the quad-layer
// kernel is faster still): the layer loop is split over TWO waves per 64
// wavenumbers.  Wave 0 (producer) streams the tables and advances the optical
// depth and the Planck term; wave 1 (consumer) turns each tau into the A
// transmittances and accumulates the intensities.  The halves are about equal
// in issue slots, so the serial time per layer halves at unchanged total work
// -- it pays while the single-wave columns cannot load the 1 024 SIMDs evenly
// (8 walkers: 68 vs 75 us; from 9 walkers on the single-wave kernel is as fast).
// Hand-off: an LDS ring of two 4-layer halves per lane -- rule 0:
// [tau, (B_{k-1}+B_k)/2 * live], rule 2: [tau, live ? B_k : -1] -- and ONE
// raw workgroup barrier per 4 layers (the consumer reads half b while the
// producer fills half b+1).  Rules 0 and 2 only: rule 1 never takes the pair (the measurements above).
template <int AT, int MT, int CT, bool SQ, int INTEG>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, BARTRT_WPE)))
void rt_eclipse_split(RtArgs p) {
  static_assert(INTEG != kIntegSimpson, "rt_eclipse_split: rules 0 and 2");
  extern __shared__ double smem[];
  constexpr int A = AT, M = MT, C = CT;
  constexpr int NC = 4 + 2 * M + 2 * C, NI = 1 + C, NLD = 2 * M + 2 * C;
  constexpr int NR = NLD > 0 ? NLD : 1;
  const int L = p.L, W = p.W;
  int bid = blockIdx.x;
  if (p.nprep > 0) {   // the head of the grid prepares the NEXT batch's layer records (RtArgs::nprep)
    if (bid < p.nprep) { prep_block(p.prep_next, bid, smem); return; }
    bid -= prep_slots(p.nprep);
    if (bid < 0) return;
  }
  int tile, w;
  block_to_work(bid, p.nwalkers, tile, w);
  if (tile >= p.ntiles) return;

  double *sC = smem;
  idx_t *sI = reinterpret_cast<idx_t *>(smem + (size_t)L * NC);
  double *sX = smem + (size_t)L * NC + (size_t)L * NI;  // [2 halves][4 layers][tau, hb][64]
  int *sFlag = reinterpret_cast<int *>(sX + 1024);      // [half] producer saw every lane finished
  double *sEnd = sX + 1024 + 2;                         // [64] B of the last layer (cloud deck term)
  {
    const double *gC = p.coef + (size_t)w * L * NC;
    const idx_t *gI = p.idx + (size_t)w * L * NI;
    stage2_to_lds(sC, gC, L * NC, sI, gI, L * NI, threadIdx.x, 128);
    if (threadIdx.x < 2) sFlag[threadIdx.x] = 0;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform
  const int i = tile * 64 + lane;
  const bool valid = i < W;
  const unsigned ii = valid ? (unsigned)i : (unsigned)(W - 1);
  const int kraw = p.kstop[w], kend = kstop_layer(kraw);
  const bool deck_on = kstop_deck(kraw);
  const int nblk = kend / 4 + 1;  // 4-layer blocks; both waves run the same count

  if (role == 0) {
    // ---------------- producer: extinction, tau, Planck ----------------
    const double nu = p.wn[ii];
    const double bnum = 2.0 * kH * nu * nu * nu * kLS * kLS;
    const double nu4 = (nu * nu) * (nu * nu);
    const TableLoader<M, C> tab(p, ii, sI);
    auto load_layer = [&](int k, double (&r)[NR]) { tab.load(k, r); };
    TauColumn<INTEG> tc;
    double Bprev = 0.0;
    bool active = true;
    auto layer = [&](int k, const double (&r)[NR]) {
      const int kc = k < kend ? k : kend;
      const bool live = active && k <= kend;
      const double *c = sC + kc * NC;
      double cf[NC];
#pragma unroll
      for (int j = 0; j < NC; j++) cf[j] = c[j];
      const double lv = live ? 0.5 : 0.0;
      double e = fma(cf[2 + 2 * M + 2 * C], nu4, cf[3 + 2 * M + 2 * C]);   // Rayleigh + grey cloud
#pragma unroll
      for (int j = 0; j < NLD; j++) e = fma(cf[2 + j], r[j], e);
      tc.layer(k, live, lv, e, cf[0], nullptr);
      const double B = bnum * rcp_n1(exp_rt(fmin(cf[1] * nu, 700.0)) - 1.0);
      double *slot = sX + (k & 7) * 128;   // half (k/4)&1, layer k&3
      slot[lane] = tc.tau;
      slot[64 + lane] = INTEG == kIntegTransmittance ? (Bprev + B) * lv : (live ? B : -1.0);
      Bprev = B;
      active = active && !(live && tc.tau > p.toomuch);
    };
    // LDS writes of a 4-layer block complete, then meet the consumer (raw
    // barrier: a __syncthreads() fence would also drain the table loads in flight)
    auto handoff = [&]() {
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    };
    auto clampk = [&](int k) { return k < kend ? k : kend; };
    double a0[NR], a1[NR], b0[NR], b1[NR];
    load_layer(clampk(0), a0);
    load_layer(clampk(1), a1);
    int blk = 0;
    for (; blk < nblk; blk++) {
      const int k0 = blk * 4;
      load_layer(clampk(k0 + 2), b0);
      load_layer(clampk(k0 + 3), b1);
      layer(k0, a0);
      layer(k0 + 1, a1);
      load_layer(clampk(k0 + 4), a0);
      load_layer(clampk(k0 + 5), a1);
      layer(k0 + 2, b0);
      layer(k0 + 3, b1);
      // the exit decision travels with the block, so both waves leave after
      // the same barrier
      const bool stop = !__any(active);
      if (lane == 0) sFlag[blk & 1] = stop ? 1 : 0;
      handoff();
      if (stop) break;
    }
    sEnd[lane] = (deck_on && active) ? Bprev : 0.0;
    handoff();
    if (p.walked_out && lane == 0)
      p.walked_out[(size_t)w * p.ntiles + tile] = (4 * blk + 4 < kend + 1 ? 4 * blk + 4 : kend + 1);
  } else {
    // ---------------- consumer: transmittances and intensities ----------------
    ColumnFlux<INTEG, A> ci(p);
    const double tcap = tau_cap(p, A);
    for (int blk = 0; blk < nblk; blk++) {
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const int stop = sFlag[blk & 1];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const double *slot = sX + ((blk & 1) * 4 + u) * 128;
        const double tau = slot[lane], hb = slot[64 + lane];
        const double tcl = fmin(tau, tcap);
        constexpr int AE = SQ ? A - 1 : A;
        double xs[AE], es[A];
#pragma unroll
        for (int a = 0; a < AE; a++) xs[a] = -tcl * p.invmu[a];
        {
          double ex[AE];
          exp_rt_n<AE>(xs, ex);
#pragma unroll
          for (int a = 0; a < AE; a++) es[a] = ex[a];
          if (SQ) es[A - 1] = ex[0] * ex[0];
        }
        if constexpr (INTEG == kIntegTransmittance) {
          const double G = angle_sum<A>(p, es);     // the producer's hb already carries the 1/2 and the mask
          ci.F = fma(hb, ci.Gprev - G, ci.F);
          ci.Gprev = G;
        } else {
          const bool live = hb >= 0.0;   // the producer's "layer counts" flag
          ci.layer(p, A, live, live ? 0.5 : 0.0, tau, 0.0, live ? hb : 0.0, es);
        }
      }
      if (__builtin_amdgcn_readfirstlane(stop)) break;
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const double bsurf = sEnd[lane];   // > 0: the deck was reached below toomuch
    const double F = ci.flux(p, A, bsurf != 0.0, bsurf, L);
    if (valid) p.spec[(size_t)w * W + i] = F;
  }
}

// ---------------------------------------------------------------------------
// Quad-layer variant: a wave takes 16 wavenumbers and FOUR layers at a time.
// Lane (q = l / 16, m = l % 16) owns wavenumber m in the layers j = 4 s + q: per
// step s the four lane rows load and evaluate four consecutive layers side by
// side, the optical depth is a 4-lane prefix sum on top of the running value of
// the previous step (the wavefront scan of the tau integral), and every lane
// turns its own tau into its layer's Planck term and A transmittances.  The
// previous layer's values a trapezoid step needs come from the lane row below
// (row 3 of the previous step for row 0).  Same arithmetic per (layer,
// wavenumber) as the single-wave kernel, but a column is 25 steps deep instead
// of 100 layers, and a launch is made of four times as many, four times shorter
// waves: ten walkers are 6 250 of them over 1 024 SIMDs instead of 1 570 that
// leave half of the SIMDs with two and half with one.  The `toomuch` exit is
// per 16 wavenumbers and per step of four layers.
// R = lane rows = layers per step (4, or 8 for the smallest launches: 8
// wavenumbers x 8 layers per wave, twice the waves, half the depth).
//
// Rule 1 (Simpson) in this layout: the panel that ends on layer j is evaluated by
// the lane that owns j, from the values of the rows q-1 and q-2 (the two carries
// of rows 0 / 1 come from the previous step); R is even, so a lane's panels all
// end on the parity of q and each lane keeps ONE sum.  The padded point falls to
// the row after the one that passed `toomuch` (row 0 of the next step when that
// was the last row), and at the end the rows whose parity is that of the last
// point's index are added up.  The optical depth is the prefix sum of the even
// rows' radius panels plus, on odd rows, the trapezoid of the last interval.
//
// RAYS (rules 0 / 2): one ray angle per lane -- a wave's 64 / R columns are (wavenumber, ray) pairs instead of
// wavenumbers (R = 4, five angles: three wavenumbers x five rays, one column idle).  Every lane then runs the single-ray
// form of the walk with its own ray's constants: one transmittance and ITS cut (`cut slant`: the ray's threshold
// RtArgs::thr, so the ballots that find a column's cut work per ray as they stand); the five rays of a wavenumber meet
// in a five-lane sum at the very end.  Extinction, optical depth and Planck term are computed five times over -- on launches that leave
// most of the chip idle anyway (one to three walkers) -- in exchange for a layer-parallel walk whose per-step work
// is a fifth of the five-ray lane's: this is how `cut slant`, whose rays cannot share a layer sum, keeps a
// few-walker kernel (the single-wave slant kernel walks a column's 100 layers serially: 50 us at any small batch).
//
// ALLR (rule 1, `cut slant`): all rays in every lane.  What `cut slant` takes away from this kernel is the single
// integrand that crossed the lane rows -- each ray needs its own last two integrands from the rows below -- not the
// layer parallelism: the rays' alive flags need no ballots at all (a ray is alive on layer j iff the largest optical
// depth of the layers above, an exclusive prefix MAXIMUM across the rows on top of the previous steps' carry, is at or
// below its threshold RtArgs::thr), the row after a ray's last layer is its padded point (alive at the start of layer
// j - 1, dead at the start of j: the same two prefix maxima), whose panel takes weights of its own (one unit of slant
// depth = mu_a of vertical depth: computed only in waves where some lane pads that ray), and every lane keeps one sum
// per ray (its layers all have the parity of its row).  At the end each ray's last point index is the largest padded
// row of its column (or the column's last layer) and the rows of that parity are added up.  Ten values cross the rows
// per step instead of two; extinction, optical depth and Planck term are computed once per (layer, wavenumber) --
// which the one-ray-per-lane form (RAYS) does five times.
// (BARTRT_QUAD_WPE, A/B builds: waves per SIMD the register allocation is held to.  Three -- 168 registers instead of
// 170-188 -- was measured in round 5: two walkers on the demo shape 23.8 -> 20.2 us, one walker 18.9 -> 19.6; left as it was.)
#ifndef BARTRT_QUAD_WPE
#define BARTRT_QUAD_WPE 1
#endif
template <int AT, int MT, int CT, bool SQ, int R, int INTEG, bool RAYS = false, bool ALLR = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BARTRT_QUAD_WPE))) void rt_eclipse_quad(RtArgs p) {
  extern __shared__ double smem[];
  constexpr int A = AT, M = MT, C = CT;
  constexpr int NC = 4 + 2 * M + 2 * C, NI = 1 + C, NLD = 2 * M + 2 * C, NR = NLD > 0 ? NLD : 1;
  constexpr int AL = RAYS ? 1 : A;                    // ray angles a lane evaluates
  constexpr int AE = RAYS ? 1 : (SQ ? A - 1 : A);     // transmittances that need an exponential
  constexpr int WN = 64 / R;                          // columns per wave
  constexpr int WNR = RAYS ? WN / A : WN;             // wavenumbers per wave
  static_assert(!RAYS || (WNR >= 1 && !SQ && INTEG != kIntegSimpson), "RAYS: rules 0 / 2, the ray grid fits a lane row, no squared-transmittance shortcut");
  static_assert(!ALLR || (INTEG == kIntegSimpson && !RAYS), "ALLR: rule 1, all rays per lane");
  constexpr bool SIMPSON = INTEG == kIntegSimpson;
  const int L = p.L, W = p.W;
  int bid = blockIdx.x;
  if (p.nprep > 0) {   // the head of the grid prepares the NEXT batch's layer records (RtArgs::nprep)
    if (bid < p.nprep) { prep_block(p.prep_next, bid, smem); return; }
    bid -= prep_slots(p.nprep);
    if (bid < 0) return;
  }
  int tile, w;
  block_to_work(bid, p.nwalkers, tile, w);
  if (tile >= p.ntiles) return;

  // (16 rows and up: the rows of a wave read 16 / 32 different layer records at once -- an even record stride would
  // put them on 2-4 of the 64 LDS banks' positions; one double of padding per record spreads them over all)
  constexpr int NCS = (R >= 16 && NC % 2 == 0) ? NC + 1 : NC;
  double *sC = smem;
  idx_t *sI = reinterpret_cast<idx_t *>(smem + (size_t)L * NCS);
  const double *sW = smem + (size_t)L * NCS + (size_t)L * NI;  // rule 1 only
  // nprep < 0: this launch prepares its own walkers -- every workgroup builds its walker's layer records in LDS itself
  // (prep_body, the same code and bits as the prep_profiles launch it replaces; launch_rt_folded)
  __shared__ int sKstopFold;
  const bool fold = p.nprep < 0;
  if (fold) {
    PrepFold pf;
    pf.coef = sC; pf.stride = NCS; pf.idx = sI; pf.kstop = &sKstopFold; pf.global = tile == 0;
    prep_block(p.prep_next, w, smem + (size_t)L * NCS + (size_t)L * NI + integ_lds_doubles<INTEG>(L), pf);
  } else if constexpr (NCS == NC) {
    stage2_to_lds(sC, p.coef + (size_t)w * L * NC, L * NC, sI, p.idx + (size_t)w * L * NI, L * NI,
                  threadIdx.x, 256);
  } else {
    const double *src = p.coef + (size_t)w * L * NC;
    const idx_t *srci = p.idx + (size_t)w * L * NI;
    for (int k = threadIdx.x; k < L * NC; k += 256) sC[(k / NC) * NCS + k % NC] = src[k];
    for (int k = threadIdx.x; k < L * NI; k += 256) sI[k] = srci[k];
  }
  __syncthreads();
  if (SIMPSON) {
    simpson_radius_weights(const_cast<double *>(sW), sC, NCS, L, threadIdx.x, 256);
    __syncthreads();
  }

  const int lane = threadIdx.x & 63;
  const int q = lane / WN, m = lane % WN;
  const int ray = RAYS ? m % A : 0, mw = RAYS ? m / A : m;   // column m = wavenumber mw (and ray)
  const bool col_on = !RAYS || m < WNR * A;                  // (RAYS: the columns past the last whole wavenumber idle)
  const int i0 = (tile * 4 + (threadIdx.x >> 6)) * WNR;  // this wave's first wavenumber
  if (i0 >= W) return;
  const unsigned ii = (col_on && i0 + mw < W) ? (unsigned)(i0 + mw) : (unsigned)(W - 1);
  // this lane's ray (RAYS) -- or, without, the column's cut as it always was
  double invmu_l = p.invmu[0], wgt_l = p.wgt[0], wq_l = p.wq[0], thr_l = p.toomuch;
  if constexpr (RAYS) {
    if (p.cut_slant) thr_l = p.thr[0];
#pragma unroll
    for (int a = 1; a < A; a++)
      if (ray == a) {
        invmu_l = p.invmu[a]; wgt_l = p.wgt[a]; wq_l = p.wq[a];
        if (p.cut_slant) thr_l = p.thr[a];
      }
  }
  const double nu = p.wn[ii];
  const double bnum = 2.0 * kH * nu * nu * nu * kLS * kLS;
  const double nu4 = (nu * nu) * (nu * nu);
  const int kraw = fold ? sKstopFold : p.kstop[w], kend = kstop_layer(kraw);
  const bool deck_on = kstop_deck(kraw);
  const double tcap = tau_cap(p, A);

  // per-lane table addressing: plane offset of the lane's layer + the lane's
  // wavenumber inside the plane (kernels.hpp, "Table layout")
  const auto rs_c = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(p.cia), 0, (int)p.cia_bytes, 0x00020000);
  const unsigned vk = ii * 8u * (unsigned)M, vc = ii * 16u, planeB = (unsigned)M * (unsigned)W * 8u;
  auto load_layer = [&](int j, double (&r)[NR]) {
    const idx_t *ix = sI + j * NI;
    if (M > 0) {
      const idx_t mine = ix[0];
      const long long base = p.window ? row_window_base<R>(mine) : 0ll;
      const unsigned long long left = p.kappa_bytes - (unsigned long long)base;
      const auto rs_k = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<char *>(reinterpret_cast<const char *>(p.kappa) + base), 0,
          (int)(unsigned)(left < 0xffffffffull ? left : 0xffffffffull), 0x00020000);
      load_table_lane<M>(rs_k, (unsigned)(mine - base) + vk, 0, planeB, r);
    }
#pragma unroll
    for (int cc = 0; cc < C; cc++) load_cia_lane(rs_c, (unsigned)ix[1 + cc] + vc, 0, r + 2 * M + 2 * cc);
  };
  auto clampk = [&](int k) { return k < kend ? k : kend; };

  // the lanes of one wavenumber: bits m, WN + m, 2 WN + m, ... of a ballot
  constexpr unsigned long long kColBits = R == 4 ? 0x0001000100010001ull : R == 8 ? 0x0101010101010101ull
                                          : R == 16 ? 0x1111111111111111ull : R == 32 ? 0x5555555555555555ull : ~0ull;
  const unsigned long long col_bits = kColBits << m;
  const unsigned long long below_bits = col_bits & ((1ull << (WN * q)) - 1ull);
  const int from_below = (lane + 64 - WN) & 63;       // row q - 1 (the last row for row 0)
  const int from_below2 = (lane + 64 - 2 * WN) & 63;  // row q - 2 (rule 1)

  double I = 0.0;   // this lane's layers' terms, angle quadrature taken (ColumnFlux, integ.hpp)
  double Fs = 0.0;  // surface term of a cloud deck (one lane per wavenumber sets it)
  // carries of row 0: extinction, Planck term, transmittances of the layer just
  // above this step (row R - 1 of the previous step), and the optical depth there
  double c_e = 0.0, c_B = 0.0, c_tau = 0.0;
  double c_G = RAYS ? wgt_l : p.wgt[0];   // rule 0: sum_a w_a E_a of the layer above (all transmittances 1 at the top)
  if constexpr (!RAYS) {
#pragma unroll
    for (int a = 1; a < A; a++) c_G += p.wgt[a];
  }
  // rule 1: second carries (row R - 2 / R - 1 of the previous step for rows 0 / 1),
  // the running even-index Simpson sum of the optical depth, the index of the last
  // point of the intensity integral and the "next step's row 0 is the padded point" flag
  double c2_e = 0.0, c2_tau = 0.0, c_y = 0.0, c2_y = 0.0, c_S = 0.0;
  int nend = kend;
  bool pad_next = false;
  // ALLR: per ray the lane's sum, the carries of the two integrands above the step, the padded row it evaluated;
  // the running maximum of tau over the layers above the step (and above its last row)
  [[maybe_unused]] double Ia[A], ca_y[A], ca2_y[A], c_tm = 0.0, c_tm1 = 0.0, thr_max = 0.0;
  [[maybe_unused]] int Npad[A];
  [[maybe_unused]] const int kcut = kend < L - 2 ? kend : L - 2;
  if constexpr (ALLR) {
    thr_max = p.thr[0];
#pragma unroll
    for (int a = 0; a < A; a++) { Ia[a] = ca_y[a] = ca2_y[a] = 0.0; Npad[a] = -1; thr_max = p.thr[a] > thr_max ? p.thr[a] : thr_max; }
  }
  // no layer above this step passed `toomuch` (per column, all rows agree); columns that hold no sample of the grid
  // (past its end, or the idle columns of RAYS) are dead from the start: they must not keep the wave walking
  bool active = col_on && i0 + mw < W;

  auto step = [&](int s, const double (&rv)[NR]) {
    const int j = R * s + q, jc = clampk(j);
    const bool inrange = j <= kend;
    const double *c = sC + jc * NCS;
    double cf[NC];
#pragma unroll
    for (int x = 0; x < NC; x++) cf[x] = c[x];
    double e = fma(cf[2 + 2 * M + 2 * C], nu4, cf[3 + 2 * M + 2 * C]);   // Rayleigh + grey cloud
#pragma unroll
    for (int x = 0; x < NLD; x++) e = fma(cf[2 + x], rv[x], e);
    // extinction of the layer above
    const double e_below = __shfl(e, from_below);
    const double eprev = q == 0 ? c_e : e_below;
    c_e = e_below;
    const double tau_above_step = c_tau;   // optical depth of row R - 1 of the previous step
    double tau;
    if constexpr (!SIMPSON) {
      // optical depth: R-lane prefix sum of the step's increments + the running value
      double v = (eprev + e) * cf[0] * ((inrange && active) ? 0.5 : 0.0);
#pragma unroll
      for (int d = 1; d < R; d <<= 1) {
        const double t = __shfl(v, (lane + 64 - d * WN) & 63);
        if (q >= d) v += t;
      }
      tau = c_tau + v;
    } else {
      // even rows contribute the radius panel that ends on them; odd rows add the
      // trapezoid of their last interval on top of the even sum below them
      const double e_below2 = __shfl(e, from_below2);
      const double e2 = q < 2 ? c2_e : e_below2;
      c2_e = e_below2;
      const double *wS = sW + 3 * jc;
      double v = ((q & 1) == 0 && j >= 2 && inrange && active)
                     ? fma(wS[0], e2, fma(wS[1], eprev, wS[2] * e)) : 0.0;
#pragma unroll
      for (int d = 1; d < R; d <<= 1) {
        const double t = __shfl(v, (lane + 64 - d * WN) & 63);
        if (q >= d) v += t;
      }
      const double S = c_S + v;
      c_S = __shfl(S, (R - 1) * WN + m);
      tau = (q & 1) ? fma((eprev + e) * cf[0], 0.5, S) : S;
    }
    c_tau = __shfl(tau, (R - 1) * WN + m);
    if constexpr (ALLR) {
      // ---- all rays per lane (see the comment above the kernel)
      // largest optical depth of the layers above this one / above the one above (layers past kcut do not count:
      // a ray ends only where a deeper layer exists)
      double pm = j <= kcut ? tau : 0.0;
#pragma unroll
      for (int d = 1; d < R; d <<= 1) {
        const double t = __shfl(pm, (lane + 64 - d * WN) & 63);
        if (q >= d) pm = fmax(pm, t);
      }
      const double incl = fmax(c_tm, pm);
      const double incl_b = __shfl(incl, from_below);
      const double excl = q == 0 ? c_tm : incl_b;            // over the layers < j
      const double excl_b = __shfl(excl, from_below);
      const double excl1 = q == 0 ? c_tm1 : excl_b;          // over the layers < j - 1
      c_tm1 = __shfl(excl, (R - 1) * WN + m);
      c_tm = __shfl(incl, (R - 1) * WN + m);
      // Planck term and transmittances
      const double tcl = fmin(tau, tcap);
      double xs[AE + 1], ex[AE + 1], y[A];
      xs[AE] = fmin(cf[1] * nu, 700.0);
#pragma unroll
      for (int a = 0; a < AE; a++) xs[a] = -tcl * p.invmu[a];
      exp_rt_n<AE + 1>(xs, ex);
      const double B = bnum * rcp_n1(ex[AE] - 1.0);
#pragma unroll
      for (int a = 0; a < AE; a++) y[a] = B * ex[a];
      if (SQ) y[A - 1] = y[0] * ex[0];
      // the tau grid of this lane's panel (j - 2, j - 1, j)
      const double tau_b1 = __shfl(tau, from_below);
      const double tau1 = q == 0 ? tau_above_step : tau_b1;
      const double tau_b2 = __shfl(tau, from_below2);
      const double tau2 = q < 2 ? c2_tau : tau_b2;
      c2_tau = tau_b2;
      // Simpson weights of the panel (simpson_tau_weights, integ.hpp, with the reciprocal of the upper half-width kept:
      // the rays' padded panels share that half)
      const double h0 = tau1 - tau2, h1 = tau - tau1, hs = h0 + h1;
      const bool deg0 = h0 == 0.0, deg = deg0 || h1 == 0.0;
      const double r0 = rcp_core(deg0 ? 1.0 : h0), r1 = rcp_core(h1 == 0.0 ? 1.0 : h1);
      const double s6 = hs * (1.0 / 6.0);
      double w0 = deg ? 0.5 * h0 : s6 * (2.0 - h1 * r0);
      double w1 = deg ? 0.5 * hs : s6 * (hs * hs * (r0 * r1));
      double w2 = deg ? 0.5 * h1 : s6 * (2.0 - h0 * r1);
      if (j == 1) { w0 = 0.0; w1 = 0.5 * (tau - tau1); w2 = w1; }   // the first interval: a trapezoid
#pragma unroll
      for (int a = 0; a < A; a++) {
        const double yb = __shfl(y[a], from_below), yb2 = __shfl(y[a], from_below2);
        const double y1 = q == 0 ? ca_y[a] : yb, y2 = q < 2 ? ca2_y[a] : yb2;
        ca_y[a] = yb;
        ca2_y[a] = yb2;
        const bool alive = inrange && excl <= p.thr[a];
        const bool pad = j >= 1 && j < L && !(excl <= p.thr[a]) && excl1 <= p.thr[a];   // the ray died on layer j - 1
        double cterm = fma(w0, y2, fma(w1, y1, w2 * y[a]));
        if (__any(pad)) {
          // one unit of slant depth (mu_a of vertical depth) past the last point, integrand 0 there: the panel's first
          // two weights, no division (1 / h0 is the step's, 1 / mu_a the ray's constant)
          const double hp = h0 + p.mu[a], p6 = hp * (1.0 / 6.0);
          const double v0 = deg0 ? 0.5 * h0 : p6 * (2.0 - p.mu[a] * r0);
          const double v1 = deg0 ? 0.5 * hp : p6 * (hp * hp * (r0 * p.invmu[a]));
          cterm = pad ? fma(v0, y2, v1 * y1) : cterm;
          Npad[a] = pad ? j : Npad[a];
        }
        Ia[a] += ((alive || pad) && j >= 1) ? cterm : 0.0;
        if (deck_on && j == kend && alive && !(tau > p.thr[a])) Fs = fma(p.wgt[a], y[a], Fs);   // deck reached below the ray's cut
      }
      active = c_tm1 <= thr_max;   // some ray was alive when the step's last row began: its pad or more layers may follow
      return;
    }
    // which layers of this step are still above the cut
    const unsigned long long over = __ballot(inrange && active && tau > thr_l);
    const bool live = inrange && active && (over & below_bits) == 0ull;
    // Planck term and transmittances of this lane's layer
    const double tcl = fmin(tau, tcap);
    double xs[AE + 1], ex[AE + 1];
    xs[AE] = fmin(cf[1] * nu, 700.0);
#pragma unroll
    for (int a = 0; a < AE; a++) xs[a] = -tcl * (RAYS ? invmu_l : p.invmu[a]);
    exp_rt_n<AE + 1>(xs, ex);
    const double B = bnum * rcp_n1(ex[AE] - 1.0);
    double E[AL];
#pragma unroll
    for (int a = 0; a < AE; a++) E[a] = ex[a];
    if (SQ) E[AL - 1] = E[0] * E[0];
    // the angle quadratures of this lane: all rays, or (RAYS) its one ray with the ray's weight
    auto gsum = [&]() { if constexpr (RAYS) return wgt_l * E[0]; else return angle_sum<AL>(p, E); };
    auto qsum = [&]() { if constexpr (RAYS) return wq_l * E[0]; else return angle_sum_q<AL>(p, E); };
    if constexpr (INTEG == kIntegTransmittance) {
      // the layer above: row q - 1, or the carry for row 0
      const double B_below = __shfl(B, from_below);
      const double Bprev = q == 0 ? c_B : B_below;
      c_B = B_below;
      const double hb = (Bprev + B) * (live ? 0.5 : 0.0);
      // rule 0 is linear in the transmittances: the angle quadrature first (ColumnFlux,
      // integ.hpp), so ONE value crosses the lane rows instead of one per ray angle
      const double G = gsum();
      const double G_below = __shfl(G, from_below);
      const double Gprev = q == 0 ? c_G : G_below;
      c_G = G_below;
      I = fma(hb, Gprev - G, I);
      if (deck_on && j == kend && live && !(tau > thr_l)) Fs = fma(B, G, Fs);  // deck reached below toomuch
    } else {
      // rules 1 / 2 are linear in Y = B sum_a (w_a / mu_a) E_a with angle-independent
      // weights (integ.hpp): ONE integrand per layer crosses the lane rows
      const double tau_b1 = __shfl(tau, from_below);
      const double tau1 = q == 0 ? tau_above_step : tau_b1;
      const double y = B * qsum();
      const double yb = __shfl(y, from_below);
      const double y1 = q == 0 ? c_y : yb;
      c_y = yb;
      if constexpr (INTEG == kIntegTrapzTau) {
        I = fma(y1 + y, (tau - tau1) * (live ? 0.5 : 0.0), I);
      } else {
        const double tau_b2 = __shfl(tau, from_below2);
        const double tau2 = q < 2 ? c2_tau : tau_b2;
        c2_tau = tau_b2;
        const double yb2 = __shfl(y, from_below2);
        const double y2 = q < 2 ? c2_y : yb2;
        c2_y = yb2;
        // the cut: the first row of this wavenumber that passed toomuch
        const unsigned long long mine = over & col_bits;
        const int f = mine ? (int)(__ffsll((long long)mine) - 1) / WN : -1;
        const bool cut_here = active && f >= 0;
        // the padded point: the row after the cut (row 0 of the next step when the
        // cut was the last row), as long as the atmosphere has a layer there
        const bool pad = j < L && ((cut_here && q == f + 1) || (pad_next && q == 0));
        if (cut_here) nend = R * s + f + ((R * s + f + 1 < L) ? 1 : 0);
        pad_next = cut_here && f == R - 1;
        const double x = pad ? tau1 + 1.0 : tau;
        double w0, w1, w2;
        simpson_tau_weights(tau1 - tau2, x - tau1, w0, w1, w2);
        if (j == 1) { w0 = 0.0; w1 = 0.5 * (x - tau1); w2 = w1; }  // the first interval: a trapezoid
        const bool counts = (live || pad) && j >= 1;
        const double cterm = fma(w0, y2, fma(w1, y1, w2 * (pad ? 0.0 : y)));
        I += counts ? cterm : 0.0;
      }
      if (deck_on && j == kend && live && !(tau > thr_l))   // deck reached below toomuch
        Fs = fma(B, gsum(), Fs);
    }
    active = active && (over & col_bits) == 0ull;
  };

  // rule 1 may need the row after the column's last layer for the padded point
  const int klast = SIMPSON ? (kend + 1 < L ? kend + 1 : L - 1) : kend;
  // Loads in flight ahead of the step that uses them: two steps' worth.  (Four, for the eight-row form that serves
  // the smallest launches, was measured in round 4 and changes nothing there -- one walker on the demo grid 25.4
  // against 24.3 us: those launches are bound by the steps' own dependent arithmetic and cross-row traffic, not by
  // memory round trips -- and costs the two-walker launch on the bench grid its occupancy, 42.7 against 34.7 us.)
  constexpr int NBUF = 2;
  double rbuf[NBUF][NR];
#pragma unroll
  for (int b = 0; b < NBUF - 1; b++) load_layer(clampk(R * b + q), rbuf[b]);
  int s = 0;
  bool gone = false;
  for (; R * s <= klast && !gone; s += NBUF) {
#pragma unroll
    for (int b = 0; b < NBUF; b++) {
      if (!gone && R * (s + b) <= klast) {
        load_layer(clampk(R * (s + b + NBUF - 1) + q), rbuf[(b + NBUF - 1) % NBUF]);
        step(s + b, rbuf[b]);
        if (!__any(active || pad_next)) { gone = true; s += b - NBUF; }   // (s: the last step walked, after the loop's increment)
      }
    }
  }
  if (!gone) s -= 1;   // the loop ran out: the last step walked is the one before s (clamped by the record below)
  // the rows of a wavenumber hold its layers' terms: sum them; row 0 writes
  const bool mine_counts = !SIMPSON || ((q & 1) == (nend & 1));
  double F = Fs + (mine_counts ? I : 0.0);   // the lane's layers, angle quadrature already taken
  if constexpr (ALLR) {
    F = Fs;
#pragma unroll
    for (int a = 0; a < A; a++) {
      int np = Npad[a];                    // the ray's padded row, known to the lane that evaluated it
      for (int o = WN; o < 64; o <<= 1) { const int t = __shfl_xor(np, o); np = t > np ? t : np; }
      const int nlast = np >= 0 ? np : kend;   // its last point's index
      F = fma(p.wq[a], ((q & 1) == (nlast & 1)) ? Ia[a] : 0.0, F);
    }
  }
  for (int o = WN; o < 64; o <<= 1) F += __shfl_xor(F, o);
  if constexpr (RAYS) {   // the rays of a wavenumber: columns mw A .. mw A + A - 1 of row 0, in ray order
    double Ft = 0.0;
#pragma unroll
    for (int a = 0; a < A; a++) Ft += __shfl(F, (mw * A + a) & 63);
    F = Ft;
  }
  if (q == 0 && ray == 0 && col_on && i0 + mw < W) p.spec[(size_t)w * W + i0 + mw] = F;
  if (p.walked_out && lane == 0) {
    const int layers = R * (s + 1) < kend + 1 ? R * (s + 1) : kend + 1;
    p.walked_out[(size_t)w * (4 * p.ntiles) + tile * 4 + (threadIdx.x >> 6)] = layers;
  }
}

}  // namespace bartrt
#include "rt_eclipse_s1.hpp"   // rule 1's single-wave kernel
#include "rt_eclipse_s1s.hpp"  // ... with the `toomuch` cut on each ray's slant depth
