// The host side of the specialised eclipse kernels (rt_eclipse.hpp, rt_eclipse_s1.hpp, rt_eclipse_s1s.hpp,
// rt_eclipse_qadj.hpp): which instantiation a launch runs, where it comes from, and what RtLaunchInfo says of it.
//
//  KernelId          names ONE instantiation of the six kernel templates.  Everything else derives from it: the
//                    ahead-of-time kernel (aot_kernel: the units' registries, rt_eclipse_unit.inc), the template-id
//                    hiprtc compiles where there is none (kernel_expr, kernel_ilp, kernel_rtc_ok), RtLaunchInfo's
//                    label (kernel_label).
//  launch_kernel     runs an id: ahead-of-time if a unit holds it, at run time otherwise.
//  launch_form_*     one per kernel form: fills in the id and the geometry, launches, records the label.
//  launch_rt_spec    chooses the form by shape, batch size and BARTRT_KERNEL.
//
// None of this is device code, and none of it is in the text the library embeds for hiprtc (bart_amd/build.py,
// RTC_HEADERS): an edit here, or a re-tuned kernel_table.inc, leaves the on-disk cache of run-time kernels valid.
#pragma once
#include "rt_eclipse.hpp"
#include "rtc.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

namespace bartrt {

// Kernel choice by 64-wavenumber columns per launch (measured at W = 1e4, L = 100:
// 157 columns per walker; microseconds per launch, quad-layer / split / single-wave,
// round 2, tools/ab_kernels.py):
//   1 walker 19 (8 rows) / 33 / 37   2 walkers 26 (8 rows) / 43 / 38   3: 31 / 43 / 39
//   4 walkers 39 / 45 / 41           5 walkers 48 / 47 / 44            6: 49 / 49 / 47
//   7 walkers 59 / 57 / 62           8 walkers 62 / 61 / 63            9: 68 / 70 / 67
//   10 walkers 76 / 76 / 71  (single-wave from here on)
// i.e. quad-layer while the columns leave SIMDs empty, single-wave while every column
// finds a SIMD of its own (<= 1 024), the producer/consumer pair for the first columns
// that have to share one, single-wave beyond.
// Under rule 1 (round 3, same tool with BARTRT_INTEG=1; quad-layer / split / rt_eclipse_simpson):
//   1 walker 22 (8 rows) / 38 / 38   2: 30 (8 rows) / 49 / 40   3: 39 / 50 / 41   4: 50 / 51 / 43
//   5: 60 / 54 / 47   6: 64 / 58 / 50   7: 78 / 74 / 64   8: 81 / 78 / 68   9: 91 / 79 / 69   10: 103 / 102 / 71
// -- the single-wave kernel from four walkers on, the producer / consumer pair never.
constexpr long kQuadMaxColumns = 640, kQuadMaxColumnsSimpson = 480;
// `cut slant`, rules 0 and 2: one ray per lane (rt_eclipse_quad<..., RAYS>) while the launch is a few thousand (walker,
// wavenumber) pairs -- it redoes the extinction five times over, so on the 1e4-sample grid ONE walker already takes
// what the single-wave kernel takes (63 against 58 us, +35 us per further walker).
constexpr long kQuadRaysMaxColumns = 80;
constexpr long kOctoRaysMaxColumns = 40;
// rule 1 under `cut slant`: all rays per lane in the layer-parallel walk (rt_eclipse_quad<..., ALLR>), R = 32 / 16 / 8
// layers per step by the number of 64-wide columns of the launch: the form holds two waves per SIMD (200 registers),
// 2 048 on the chip, and a launch of more waves than that runs in rounds -- so R <= 2 048 / columns, and the
// single-wave kernel beyond 256 columns.  us per RT launch (tools/ab_small.py, tools/ab_rows.sh):
//   demo shape (W = 2 501, one molecule), walkers 1 .. 5 = 40 .. 200 columns
//     R = 32: 15.3 18.1 23.7 26.7 33.9   R = 16: 18.1 21.5 21.4 25.9 34.2   R = 8: 26.4 26.7 26.9 32.7 32.6
//     one ray per lane, R = 8: 25.1 36.6 48.9 60.3 73.0
//   bench shape at W = 5 000, walkers 1 .. 3 = 79 / 158 / 237 columns
//     R = 32: 29.4 40.8 56.8   R = 16: 25.3 38.6 44.0   R = 8: 29.6 37.4 37.2   single wave: 55.8 56.0 56.0
//   bench shape (W = 1e4), one walker = 157 columns: R = 32 / 16 / 8 / 4 / single wave 42.8 / 40.2 / 37.6 / 47 / 58;
//     two walkers = 314 columns: R = 8 58.4, single wave 58.0
// The preparation folded into these kernels' prologue (every workgroup builds its walker's records itself: 6 us of
// latency-shaped work instead of a prep_profiles launch, 8 us + a boundary) pays while the workgroups run in ONE round
// (round 5, us per step, folded / not: demo shape one walker, 313 workgroups, 25.1 / 27.9, three walkers, 471: 29.4 /
// 32.2; two walkers, 626: 37.9 / 35.4, four, 628: 47.6 / 45.4; W = 1e4 one walker, 625: 48.2 / 47.4, two: 68.5 / 64.0)
constexpr int kFoldMaxWorkgroups = 512;
// (which of these forms serves which launch: kernel_table.inc, below.  The figures above are what its first version
// -- R = 32 to 64 columns, 16 to 128, 8 to 256; with one or two molecules 32 to 96, 16 to 176 -- was read from.)
constexpr long kOctoMaxColumns = 400;  // eight layers per step (R = 8) below this
constexpr long kSplitMinColumns = 1025, kSplitMaxColumns = 1300;
constexpr long kIlpMaxColumns = 20000;  // single-wave kernel: the ILP-scheduled build below this (128 walkers at W = 1e4)

// Rule 1 under `cut slant` (the default conventions): the variant comes from a MEASURED table (kernel_table.inc, written
// by tools/tune_kernels.py from a sweep on the box; round 6 -- until then a thicket of hand-measured column intervals in
// launch_rt_spec).  tests/test_gpu_kernel_choice.py holds the default choice to within 7 % of the best forced variant
// on grids the table was not tuned on.
enum KernelVariant { kVarSingle = 0, kVarRows4 = 4, kVarRows8 = 8, kVarRows16 = 16, kVarRows32 = 32, kVarAdj8 = 108, kVarAdj16 = 116 };
struct KernelChoice { long max_columns; int variant, fallback; };
constexpr long kAllColumns = 0x7fffffffffffffffL;
#include "kernel_table.inc"
inline const KernelChoice &slant_simpson_choice(int M, long columns) {
  static constexpr const KernelChoice *const tables[6] = {kSlantSimpsonM1, kSlantSimpsonM2, kSlantSimpsonM3,
                                                          kSlantSimpsonM4, kSlantSimpsonM5, kSlantSimpsonM6};
  const KernelChoice *t = tables[M < 1 ? 0 : M > 6 ? 5 : M - 1];   // (no table molecules: cross sections only -- the lightest table)
  int i = 0;
  while (columns > t[i].max_columns) i++;   // (the last entry holds kAllColumns)
  return t[i];
}
inline const char *kernel_variant_name(int v) {
  switch (v) {
    case kVarRows4: return "rows4"; case kVarRows8: return "rows8"; case kVarRows16: return "rows16"; case kVarRows32: return "rows32";
    case kVarAdj8: return "adj8"; case kVarAdj16: return "adj16"; default: return "single";
  }
}

// ---------------------------------------------------------------------------
// One instantiation of one of the six kernel templates.  A field a family's template does not have stays at its default.
enum class KFamily { Fast, Simpson, SimpsonSlant, Quad, Qadj, Split };
struct KernelId {
  KFamily family;
  int A, M, C;
  bool sq;
  int integ = 0, sched = 0, rows = 0;
  bool ext = false, slant = false, out = false, rays = false, allr = false;
};
// The id of rt_eclipse_<family><args...>: each maker takes its template's parameter list, defaults included -- the one
// place where the position of a template argument is given its meaning (the registries pass ONE argument list to the
// maker and to the template, rt_eclipse_unit.inc; kernel_expr writes it back out).
constexpr KernelId fast_id(int A, int M, int C, bool sq, int integ, int sched = 0, bool ext = false, bool slant = false) {
  return {KFamily::Fast, A, M, C, sq, integ, sched, 0, ext, slant, false, false, false};
}
constexpr KernelId split_id(int A, int M, int C, bool sq, int integ) {
  return {KFamily::Split, A, M, C, sq, integ, 0, 0, false, false, false, false, false};
}
constexpr KernelId quad_id(int A, int M, int C, bool sq, int rows, int integ, bool rays = false, bool allr = false) {
  return {KFamily::Quad, A, M, C, sq, integ, 0, rows, false, false, false, rays, allr};
}
constexpr KernelId simpson_id(int A, int M, int C, bool sq, int sched = 0, bool ext = false) {
  return {KFamily::Simpson, A, M, C, sq, 0, sched, 0, ext, false, false, false, false};
}
constexpr KernelId simpson_slant_id(int A, int M, int C, bool sq, int sched = 1, bool ext = false, bool out = false) {
  return {KFamily::SimpsonSlant, A, M, C, sq, 0, sched, 0, ext, false, out, false, false};
}
constexpr KernelId qadj_id(int A, int M, int C, bool sq, int rows) {
  return {KFamily::Qadj, A, M, C, sq, 0, 0, rows, false, false, false, false, false};
}
// the id as one integer: what the registries switch on (a byte per count, a bit per flag)
constexpr unsigned long long kernel_key(const KernelId &k) {
  return (unsigned long long)k.family | (unsigned long long)(k.A & 255) << 4 | (unsigned long long)(k.M & 255) << 12 |
         (unsigned long long)(k.C & 255) << 20 | (unsigned long long)(k.rows & 255) << 28 | (unsigned long long)(k.integ & 15) << 36 |
         (unsigned long long)(k.sched & 15) << 40 | (unsigned long long)k.sq << 44 | (unsigned long long)k.ext << 45 |
         (unsigned long long)k.slant << 46 | (unsigned long long)k.out << 47 | (unsigned long long)k.rays << 48 |
         (unsigned long long)k.allr << 49;
}

// The template-id in namespace bartrt, every argument spelled out: what hiprtc is given, and how the instantiation's
// host symbol demangles (tests/test_kernel_inventory.py holds the library's symbols to it).
inline std::string kernel_expr(const KernelId &k) {
  const auto tf = [](bool b) { return b ? "true" : "false"; };
  char s[160];
  switch (k.family) {
    case KFamily::Fast:
      std::snprintf(s, sizeof s, "rt_eclipse_fast<%d, %d, %d, %s, %d, %d, %s, %s>", k.A, k.M, k.C, tf(k.sq), k.integ, k.sched, tf(k.ext), tf(k.slant));
      break;
    case KFamily::Simpson:
      std::snprintf(s, sizeof s, "rt_eclipse_simpson<%d, %d, %d, %s, %d, %s>", k.A, k.M, k.C, tf(k.sq), k.sched, tf(k.ext));
      break;
    case KFamily::SimpsonSlant:
      std::snprintf(s, sizeof s, "rt_eclipse_simpson_slant<%d, %d, %d, %s, %d, %s, %s>", k.A, k.M, k.C, tf(k.sq), k.sched, tf(k.ext), tf(k.out));
      break;
    case KFamily::Quad:
      std::snprintf(s, sizeof s, "rt_eclipse_quad<%d, %d, %d, %s, %d, %d, %s, %s>", k.A, k.M, k.C, tf(k.sq), k.rows, k.integ, tf(k.rays), tf(k.allr));
      break;
    case KFamily::Qadj:
      std::snprintf(s, sizeof s, "rt_eclipse_qadj<%d, %d, %d, %s, %d>", k.A, k.M, k.C, tf(k.sq), k.rows);
      break;
    case KFamily::Split:
      std::snprintf(s, sizeof s, "rt_eclipse_split<%d, %d, %d, %s, %d>", k.A, k.M, k.C, tf(k.sq), k.integ);
      break;
  }
  return s;
}

// Two forms whose run-time build is NOT their ahead-of-time build's twin.  Kept as found (this header only names them);
// each is one line to change once it has been measured.
//  1. the one-walker kernel with the optical-depth / intensity outputs: ahead of time in a max-ILP unit
//     (rt_eclipse_slant_ilp.hip), at run time under the default schedule
constexpr bool rtc_differs_out(const KernelId &k) { return k.family == KFamily::SimpsonSlant && k.out; }
//  2. rule 0's five-angle single-wave kernel under `cut vertical` in its ILP build (SCHED = 1, rt_eclipse_i0_ilp.hip): at
//     run time the SCHED = 0 instantiation under the default schedule
constexpr bool rtc_differs_fast_ilp(const KernelId &k) {
  return k.family == KFamily::Fast && k.A == 5 && k.sched == 1 && !k.ext && !k.slant;
}

// does the run-time build get the max-ILP option (what bart_amd/build.py gives the ahead-of-time twin's unit)?
constexpr bool kernel_ilp(const KernelId &k) {
  switch (k.family) {
    case KFamily::Fast: return k.sched == 1 && !rtc_differs_fast_ilp(k);
    case KFamily::Simpson: return true;
    case KFamily::SimpsonSlant: return !rtc_differs_out(k);
    default: return false;   // (the layer-parallel and producer / consumer kernels: the default schedule)
  }
}
// the id hiprtc is asked for where the ahead-of-time set does not hold `k`
constexpr KernelId kernel_rtc_id(KernelId k) {
  if (rtc_differs_fast_ilp(k)) k.sched = 0;
  return k;
}
// May hiprtc serve the id at all?
//  - engines without an opacity table (cross sections only, the line-by-line hand-off) keep the generic kernel / the
//    EXT builds: the table kernels were never instantiated, let alone tested, for zero molecules
//  - the single-wave kernels keep three slots of 2 M + 2 C loads in flight: beyond 20 loads per layer (the widest shapes
//    of the ahead-of-time list: eight molecules with two slots, six with four) they spill and the generic kernel is as
//    fast or faster at ten walkers and up (round 5, W = 1e4: 7 molecules + 4 slots 507 against 585 us at ten walkers,
//    2 258 / 2 250 at 64; 9 + 2: 448 / 456 and 1 885 / 1 688) -- such shapes are instantiated for the layer-parallel
//    kernels only (one walker: 58 against 245 us), their batches stay with the generic kernel.
constexpr bool kernel_rtc_ok(const KernelId &k) {
  const bool single_wave = k.family == KFamily::Fast || k.family == KFamily::Simpson || k.family == KFamily::SimpsonSlant;
  return k.M >= 1 && (!single_wave || 2 * k.M + 2 * k.C <= 20);
}

// RtLaunchInfo::kernel of the id (static strings: the GPU tests assert them)
inline const char *kernel_label(const KernelId &k) {
  switch (k.family) {
    case KFamily::Qadj: return k.rows == 16 ? "rt_eclipse_qadj<R=16> (rows on adjacent lanes)" : "rt_eclipse_qadj<R=8> (rows on adjacent lanes)";
    case KFamily::Quad:
      if (k.allr)
        return k.rows == 32   ? "rt_eclipse_quad<R=32, all rays per lane>"
               : k.rows == 16 ? "rt_eclipse_quad<R=16, all rays per lane>"
               : k.rows == 8  ? "rt_eclipse_quad<R=8, all rays per lane>"
                              : "rt_eclipse_quad<R=4, all rays per lane>";
      if (k.rays) return k.rows == 8 ? "rt_eclipse_quad<R=8, one ray per lane>" : "rt_eclipse_quad<R=4, one ray per lane>";
      return k.rows == 8 ? "rt_eclipse_quad<R=8>" : "rt_eclipse_quad<R=4>";
    case KFamily::Split: return "rt_eclipse_split";
    default: break;
  }
  // the single-wave families
  const bool simpson = k.family != KFamily::Fast, slant = k.slant || k.family == KFamily::SimpsonSlant;
  if (k.ext) return slant ? "single-wave `cut slant` kernel (line-by-line extinction)" : "rt_eclipse_fast (line-by-line extinction)";
  if (k.out) return "rt_eclipse_simpson_slant (with optical-depth / intensity outputs)";
  if (k.A != 5)
    return slant ? (simpson ? "rt_eclipse_simpson_slant (ray grid of another size)" : "rt_eclipse_fast<SLANT> (ray grid of another size)")
           : simpson ? "rt_eclipse_simpson (ray grid of another size)"
                     : "rt_eclipse_fast (ray grid of another size)";
  if (slant) return simpson ? "rt_eclipse_simpson_slant (ILP-scheduled build)" : "rt_eclipse_fast<SLANT> (ILP-scheduled build)";
  if (simpson) return "rt_eclipse_simpson (ILP-scheduled build)";
  return k.sched ? "rt_eclipse_fast (ILP-scheduled build)" : "rt_eclipse_fast";
}

// ---------------------------------------------------------------------------
// The ahead-of-time set: every unit that instantiates kernels lists them once (rt_eclipse_unit.inc) and answers
//   find_<unit>(id)   the kernel, or nullptr
//   ids_<unit>(&n)    its ids
// Five angles: the units below, the most often asked first.  Other ray-grid sizes: one object of rt_eclipse_angles.hip
// per size (rt_eclipse_a<N>; the list comes from bart_amd/build.py -- empty by default since round 6: every other size
// is instantiated at run time).
typedef void (*RtKernel)(RtArgs);
#define BARTRT_UNITS(X) X(qadj) X(i1) X(slant_ilp) X(i1_ilp) X(i0_ilp) X(i0) X(i2)
#ifndef BARTRT_ANGLE_SIZES
#define BARTRT_ANGLE_SIZES(X)
#endif
#define BARTRT_DECL_UNIT(u) RtKernel find_##u(const KernelId &id); const KernelId *ids_##u(int *n);
#define BARTRT_DECL_ANGLES(N) BARTRT_DECL_UNIT(a##N)
BARTRT_UNITS(BARTRT_DECL_UNIT)
BARTRT_ANGLE_SIZES(BARTRT_DECL_ANGLES)
#undef BARTRT_DECL_ANGLES
#undef BARTRT_DECL_UNIT

inline RtKernel aot_kernel(const KernelId &id) {
  switch (id.A) {
#define BARTRT_CASE_ANGLES(N) case N: return find_a##N(id);
    BARTRT_ANGLE_SIZES(BARTRT_CASE_ANGLES)
#undef BARTRT_CASE_ANGLES
    case 5: break;
    default: return nullptr;
  }
#define BARTRT_ASK_UNIT(u) if (RtKernel k = find_##u(id)) return k;
  BARTRT_UNITS(BARTRT_ASK_UNIT)
#undef BARTRT_ASK_UNIT
  return nullptr;
}

// bartrt_kernel_inventory: one line per ahead-of-time id -- kernel_expr, a tab, kernel_ilp, a tab, the unit's object name.
// false: `out` names an id its unit lists and aot_kernel does not reach.
inline bool kernel_inventory(std::string &out) {
  out.clear();
  bool ok = true;
  const auto unit = [&](const char *object, const KernelId *ids, int n) {
    for (int i = 0; ok && i < n; i++) {
      if (!aot_kernel(ids[i])) { out = kernel_expr(ids[i]); ok = false; return; }
      out += kernel_expr(ids[i]) + (kernel_ilp(ids[i]) ? "\t1\trt_eclipse_" : "\t0\trt_eclipse_") + object + "\n";
    }
  };
  int n = 0;
  const KernelId *ids;
#define BARTRT_LIST_UNIT(u) ids = ids_##u(&n); unit(#u, ids, n);
#define BARTRT_LIST_ANGLES(N) BARTRT_LIST_UNIT(a##N)
  BARTRT_UNITS(BARTRT_LIST_UNIT)
  BARTRT_ANGLE_SIZES(BARTRT_LIST_ANGLES)
#undef BARTRT_LIST_ANGLES
#undef BARTRT_LIST_UNIT
  return ok;
}

// If one ray angle has exactly half the cosine of another (0 and 60 degrees of
// the usual raygrid 0 20 40 60 80), put that pair first and last: the SQ kernels
// take the last transmittance as the square of the first.
inline bool order_angles_for_square(RtArgs &r) {
  for (int i = 0; i < r.A; i++)
    for (int j = 0; j < r.A; j++) {
      if (i == j || std::fabs(r.invmu[j] - 2.0 * r.invmu[i]) > 8.9e-16 * r.invmu[j]) continue;
      auto swap_angles = [&](int x, int y) {
        std::swap(r.invmu[x], r.invmu[y]);
        std::swap(r.wgt[x], r.wgt[y]);
        std::swap(r.wq[x], r.wq[y]);
        std::swap(r.mu[x], r.mu[y]);
        std::swap(r.thr[x], r.thr[y]);
        std::swap(r.drank[x], r.drank[y]);
        std::swap(r.thrb[x], r.thrb[y]);
      };
      swap_angles(0, i);
      if (j == 0) j = i;  // the doubled angle sat in slot 0 and moved to i
      swap_angles(r.A - 1, j);
      return true;
    }
  return false;
}

// ---------------------------------------------------------------------------
// launch_rt_spec (below) chooses a form; each form's launcher owns its id, tiles, workgroups, LDS and RtLaunchInfo, and
// returns false when it launched nothing.
// SpecLaunch: what the forms share -- the launch's arguments (b: with the ray angles ordered for the SQ kernels and the
// table's addressing chosen), the LDS of its walkers' layer records, and the next batch's preparation (RtArgs::nprep):
// every five-angle form carries it at the head of its grid, prep_slots(nprep) more workgroups, LDS for the larger of the
// two jobs.
struct SpecLaunch {
  const RtArgs &a;
  RtArgs b;
  bool sq = false;
  int block;
  hipStream_t st;
  hipError_t &err;
  RtLaunchInfo *info;
  const PrepArgs *fold;   // (launch_rt_spec)
  size_t sh;              // LDS of the layer records (+ rule 1's Simpson weights of the radius grid)
  int nblocks;            // the single-wave grid without the preparation's workgroups
  int nsel;               // the batch the form is chosen for (RtArgs::nsel)
  int pslots = 0;         // the preparation's workgroups
  size_t shp = 0;         // LDS the preparation needs beyond sh
  size_t sh_fold = 0;     // LDS of the preparation of `fold`

  SpecLaunch(const RtArgs &a_, size_t sh_, int block_, hipStream_t st_, hipError_t &err_, RtLaunchInfo *info_,
             const PrepArgs *fold_)
      : a(a_), b(a_), block(block_), st(st_), err(err_), info(info_), fold(fold_), sh(sh_),
        nblocks((a_.ntiles + 7) / 8 * 8 * a_.nwalkers), nsel(a_.nsel > a_.nwalkers ? a_.nsel : a_.nwalkers) {
    if (a.nprep > 0) {
      pslots = prep_slots(a.nprep);
      const size_t need = sizeof(double) * prep_lds_doubles(a.prep_next.L, a.prep_next.S, a.prep_next.Nt, a.prep_next.ncia_temps);
      shp = need > sh ? need - sh : 0;
    }
    if (fold) sh_fold = sizeof(double) * prep_lds_doubles(fold->L, fold->S, fold->Nt, fold->ncia_temps);
  }
  void order_angles(bool allow_sq) { sq = allow_sq && order_angles_for_square(b); }
  // the layer-parallel kernels address the tables with per-lane 32-bit offsets (a grid of 4 GB or more through a window
  // that moves with the step's layers)
  bool addressable(int rows) const { return a.cia_bytes < (1ull << 32) - 4096 && (!b.window || window_fits(a, rows)); }
  // workgroups of `ntiles` tiles per walker (block_to_work: whole rounds of eight), the preparation's included
  int workgroups(int ntiles) const { return (ntiles + 7) / 8 * 8 * a.nwalkers + pslots; }
  // the form launched: what RtLaunchInfo records of it
  // (window: the layer-parallel forms pass their RtArgs::window)
  bool launched(const char *kernel, int wn_per_column, int ncolumns, bool folded = false, bool window = false) const {
    if (info) {
      info->kernel = kernel; info->wn_per_column = wn_per_column; info->ncolumns = ncolumns; info->prep_folded = folded;
      info->window = window;
    }
    return true;
  }
};

// Runs the id on `args`: the ahead-of-time kernel if a unit holds it, else -- where the id allows it -- the same template
// instantiated at run time (rtc.hpp; RtLaunchInfo::rtc).  false: neither (no compiler at hand: the caller falls through to
// the generic kernel); c.err: the launch's status otherwise.
inline bool launch_kernel(const SpecLaunch &c, const KernelId &id, int nwg, int threads, size_t lds, const RtArgs &args) {
  if (const RtKernel kernel = aot_kernel(id)) {
    BARTRT_RT_LAUNCH(kernel, dim3(nwg), dim3(threads), lds, c.st, args);
    c.err = hipGetLastError();
    return true;
  }
  if (!kernel_rtc_ok(id) ||
      !rtc_launch(kernel_expr(kernel_rtc_id(id)), kernel_ilp(id), dim3(nwg), dim3(threads), lds, c.st, args, c.err))
    return false;
  if (c.info) c.info->rtc = true;
  return true;
}

// A layer-parallel launch (rt_eclipse_quad, rt_eclipse_qadj): workgroups of four waves of `wn` wavenumbers, R = rows
// layers per step (from 16 rows on the layer records are padded: NCS).  folds: it prepares its own walkers -- asked to
// (fold), LDS for both jobs, and its workgroups run in one round (kFoldMaxWorkgroups).
struct LpGeom { RtArgs b; int wn, ncolumns, nwg; size_t lds; bool folds; };
inline LpGeom lp_geom(const SpecLaunch &c, int rows, int wn) {
  LpGeom g{c.b, wn, 0, 0, 0, false};
  g.b.ntiles = (c.a.W + 4 * wn - 1) / (4 * wn);
  g.ncolumns = 4 * g.b.ntiles;
  g.nwg = c.workgroups(g.b.ntiles);
  g.lds = c.sh + c.shp + (rows >= 16 ? sizeof(double) * (size_t)c.a.L : 0);
  g.folds = c.fold && g.lds + c.sh_fold <= 64 * 1024 && (g.b.ntiles + 7) / 8 * 8 * c.nsel + c.pslots <= kFoldMaxWorkgroups;
  if (g.folds) { g.b.nprep = -1; g.b.prep_next = *c.fold; g.lds += c.sh_fold; }
  return g;
}

// a single-wave form: one workgroup of c.block lanes per tile and walker, the next batch's preparation at the grid's head
inline bool launch_single_wave(const SpecLaunch &c, const KernelId &id, const RtArgs &args) {
  return launch_kernel(c, id, c.workgroups(args.ntiles), c.block, c.sh + c.shp, args) && c.launched(kernel_label(id), c.block, args.ntiles);
}
// a layer-parallel form: four waves per workgroup
inline bool launch_layer_parallel(const SpecLaunch &c, const KernelId &id, const LpGeom &g) {
  return launch_kernel(c, id, g.nwg, 256, g.lds, g.b) && c.launched(kernel_label(id), g.wn, g.ncolumns, g.folds, g.b.window != 0);
}

// line-by-line hand-off: the single-wave kernel with the extinction array as one more load per layer (no table, 0-2 or 4
// CIA slots, no preparation in the grid)
template <int INTEG>
bool launch_form_ext(const SpecLaunch &c) {
  const RtArgs &b = c.b;
  const KernelId id = b.cut_slant ? (INTEG == kIntegSimpson ? simpson_slant_id(5, b.M, b.C, c.sq, 1, true) : fast_id(5, b.M, b.C, c.sq, INTEG, 1, true, true))
                                  : (INTEG == kIntegSimpson ? simpson_id(5, b.M, b.C, c.sq, 1, true) : fast_id(5, b.M, b.C, c.sq, INTEG, 1, true));
  return launch_kernel(c, id, c.nblocks, c.block, c.sh, b) && c.launched(kernel_label(id), c.block, b.ntiles);
}

// tau.dat / outintens of the default conventions (one walker): the single-wave slant kernel writes them on its way
// (the ray angles in their own order: no squared-transmittance pairing)
inline bool launch_form_slant_out(const SpecLaunch &c) {
  const RtArgs &a = c.a;
  const KernelId id = simpson_slant_id(5, a.M, a.C, false, 0, false, true);
  return launch_kernel(c, id, c.nblocks, c.block, c.sh, a) && c.launched(kernel_label(id), c.block, a.ntiles);
}

// ray grids of other sizes than five, rules 0 / 1: the single-wave kernels (the ray angles in their own order; a ray grid
// of ten and more angles, or a (molecules, slots) pair outside the ahead-of-time list, at run time)
template <int INTEG>
bool launch_form_angles(const SpecLaunch &c) {
  const RtArgs &a = c.a;
  return launch_single_wave(c, a.cut_slant ? (INTEG == kIntegTransmittance ? fast_id(a.A, a.M, a.C, false, 0, 1, false, true)
                                                                           : simpson_slant_id(a.A, a.M, a.C, false, a.A <= 6 ? 1 : 0))
                                           : (INTEG == kIntegTransmittance ? fast_id(a.A, a.M, a.C, false, 0, 1) : simpson_id(a.A, a.M, a.C, false, 1)),
                            a);
}

// rule 1 / `cut slant`: rt_eclipse_qadj, the rows of a column on adjacent lanes (R = 8 / 16; rt_eclipse_qadj.hpp)
inline bool launch_form_qadj(const SpecLaunch &c, const LpGeom &g, int rows) {
  return launch_layer_parallel(c, qadj_id(5, g.b.M, g.b.C, c.sq, rows == 16 ? 16 : 8), g);
}

// rule 1 / `cut slant`: rt_eclipse_quad<..., ALLR>, all rays per lane (R = 4 / 8 / 16 / 32)
template <int INTEG>
bool launch_form_quad_allr(const SpecLaunch &c, const LpGeom &g, int rows) {
  static_assert(INTEG == kIntegSimpson, "the all-rays form: rule 1");
  return launch_layer_parallel(c, quad_id(5, g.b.M, g.b.C, c.sq, rows, INTEG, false, true), g);
}

// rules 0 / 2, `cut slant`: rt_eclipse_quad<..., RAYS>, one ray per lane (R = 4 / 8: three wavenumbers / one x five rays
// per wave)
template <int INTEG>
bool launch_form_quad_rays(const SpecLaunch &c, int rows) {
  static_assert(INTEG != kIntegSimpson, "the one-ray-per-lane form: rules 0 / 2");
  const LpGeom g = lp_geom(c, rows, 64 / rows / 5);   // (c.fold: rule 1 only)
  return launch_layer_parallel(c, quad_id(5, g.b.M, g.b.C, false, rows, INTEG, true), g);
}

// `cut slant`: the single-wave kernels, each ray its own sums in one lane (ILP-scheduled builds, rt_eclipse_slant_ilp.hip)
template <int INTEG>
bool launch_form_slant(const SpecLaunch &c) {
  const RtArgs &b = c.b;
  return launch_single_wave(c, INTEG == kIntegSimpson ? simpson_slant_id(5, b.M, b.C, c.sq, slant_sched(b.M, b.C, 1))
                                                      : fast_id(5, b.M, b.C, c.sq, INTEG, 1, false, true),
                            b);
}

// `cut vertical`: rt_eclipse_quad, R = 4 / 8 rows of 16 / 8 wavenumbers
template <int INTEG>
bool launch_form_quad(const SpecLaunch &c, int rows) {
  const LpGeom g = lp_geom(c, rows, 64 / rows);
  return launch_layer_parallel(c, quad_id(5, g.b.M, g.b.C, c.sq, rows, INTEG), g);
}

// `cut vertical`, rules 0 / 2: rt_eclipse_split, a producer / consumer pair of waves per 64 wavenumbers
template <int INTEG>
bool launch_form_split(const SpecLaunch &c) {
  RtArgs b = c.b;
  b.ntiles = (b.W + 63) / 64;
  const size_t lds = c.sh + sizeof(double) * (1024 + 2 + 64) + c.shp;   // + the hand-off ring, the exit flags, the deck terms
  const KernelId id = split_id(5, b.M, b.C, c.sq, INTEG);
  return launch_kernel(c, id, c.workgroups(b.ntiles), 128, lds, b) && c.launched(kernel_label(id), 64, b.ntiles);
}

// `cut vertical`: the single-wave kernels.  ilp: rule 0 in its ILP-scheduled build (rt_eclipse_i0_ilp.hip).
// Rule 1 has its own single-wave kernel (rt_eclipse_s1.hpp), built under the ILP schedule only: that build is the faster
// one at every batch size (10 walkers 73 against 80 us, 64: 333 / 375, 256: 1 138 / 1 220 -- the default schedule needs
// 182 registers for two resident waves, or drops the record read-ahead for three and waits on LDS instead).
template <int INTEG>
bool launch_form_single(const SpecLaunch &c, bool ilp) {
  const RtArgs &b = c.b;
  return launch_single_wave(c, INTEG == kIntegSimpson ? simpson_id(5, b.M, b.C, c.sq, 1)
                                                      : fast_id(5, b.M, b.C, c.sq, INTEG, ilp && INTEG == kIntegTransmittance ? 1 : 0),
                            b);
}

// Launches the specialised kernel for this shape and batch size under rule INTEG; false: the shape has none (the caller
// falls back to the generic kernel).  mode: the form BARTRT_KERNEL forces (KernelMode::kDefault: the choice by shape and
// batch size).  info (optional): what was launched.
// fold (optional): the preparation of this launch's walkers, NOT yet launched -- only the kernels that can run it in
// their own prologue (the all-rays layer-parallel forms of rule 1 under `cut slant`) are considered then, and false
// means "launch the preparation, then call again without it".
template <int INTEG>
bool launch_rt_spec(const RtArgs &a, int block, hipStream_t st, KernelMode mode, bool force_window, bool allow_sq,
                    hipError_t &err, RtLaunchInfo *info, const PrepArgs *fold = nullptr) {
  if (fold && (INTEG != kIntegSimpson || !a.cut_slant || a.A != 5 || a.ext || a.intens_out || a.tau_out || a.nprep != 0)) return false;
  SpecLaunch c(a,
               sizeof(double) * ((size_t)a.L * coef_stride(a.M, a.C) + integ_lds_doubles<INTEG>(a.L)) +
                   sizeof(idx_t) * (size_t)a.L * idx_stride(a.C),
               block, st, err, info, fold);
  err = hipSuccess;
  // (the specialised kernels rebuild their buffer descriptor per layer, so the
  // table may be of any size; one layer's pair of planes must stay below 4 GB)
  const bool fits = 2ull * a.M * a.W * 8ull < (1ull << 31) && c.sh <= 55 * 1024;

  // line-by-line input: rules 0 and 1, no table (anything else takes the generic kernel)
  if (a.ext) {
    if (!(INTEG != kIntegTrapzTau && a.A == 5 && a.M == 0 && (a.C <= 2 || a.C == 4) && !a.intens_out && !a.tau_out &&
          c.sh <= 55 * 1024))
      return false;
    c.order_angles(allow_sq);
    return launch_form_ext<INTEG>(c);
  }
  // tau / intensity outputs: the default conventions' slant kernel at one walker, the generic kernel otherwise
  if (a.intens_out || a.tau_out)
    return INTEG == kIntegSimpson && a.cut_slant && a.A == 5 && a.slog && a.nwalkers == 1 && a.nprep == 0 && fits &&
           mode == KernelMode::kDefault && launch_form_slant_out(c);
  if (!fits) return false;
  // (the event log serves rule 1's single-wave slant kernels only -- rt_eclipse_s1s.hpp; rule 2 on other ray grids:
  // generic kernel)
  if (a.cut_slant && ((INTEG == kIntegSimpson && !a.slog) || (INTEG == kIntegTrapzTau && a.A != 5))) return false;
  if (info) info->prep_fused = a.nprep > 0;

  // other ray-grid sizes: the single-wave kernel of rule 0 / rule 1 at every batch size
  if (a.A != 5)
    return INTEG != kIntegTrapzTau && a.A >= 1 && a.A <= kMaxAngles && mode != KernelMode::kQuad && mode != KernelMode::kOcto &&
           mode != KernelMode::kSplit && launch_form_angles<INTEG>(c);

  // five ray angles: too few single-wave columns to load the 1 024 SIMDs evenly -> several waves per 64 wavenumbers
  c.order_angles(allow_sq);
  c.b.window = a.kappa_bytes >= (1ull << 32) - 4096 || force_window;
  const bool dflt = mode == KernelMode::kDefault;
  const long columns = (long)c.nsel * (((a.Wfull > 0 ? a.Wfull : a.W) + 63) / 64);   // (of the whole grid: RtArgs::Wfull)
  const bool octo = mode == KernelMode::kOcto || (dflt && columns <= kOctoMaxColumns);
  const bool fits32 = c.addressable(octo ? 8 : 4);
  if (a.cut_slant) {
    if constexpr (INTEG == kIntegSimpson) {
      // rule 1: the layer-parallel walk with all rays per lane, forced or where the measured table (kernel_table.inc) names
      // it -- rows on adjacent lanes (rt_eclipse_qadj; BARTRT_KERNEL=adj8 / adj16 force it, BARTRT_ADJ=0 switches it off),
      // else across lane rows (rt_eclipse_quad<..., ALLR>, the entry's fallback should the adjacent form not launch)
      static const int adj_env = [] { const char *v = std::getenv("BARTRT_ADJ"); return v && *v ? atoi(v) : -1; }();
      const KernelChoice &entry = slant_simpson_choice(a.M, columns);
      const bool adj_named = entry.variant == kVarAdj16 || entry.variant == kVarAdj8;
      const int other = adj_named ? entry.fallback : entry.variant;
      int rows = mode == KernelMode::kQuad ? 4 : mode == KernelMode::kOcto ? 8 : mode == KernelMode::kHexa ? 16
                 : mode == KernelMode::kR32 ? 32 : other == kVarSingle ? 4 : other;
      while (rows > 4 && c.b.window && !window_fits(a, rows)) rows /= 2;
      int adj_rows = mode == KernelMode::kAdj8 ? 8 : mode == KernelMode::kAdj16 ? 16 : 0;
      if (dflt && adj_env != 0 && adj_named) adj_rows = entry.variant == kVarAdj16 ? 16 : 8;
      if (adj_rows && c.addressable(adj_rows)) {
        const LpGeom g = lp_geom(c, adj_rows, 64 / adj_rows);
        if (fold && !g.folds) return false;
        if (launch_form_qadj(c, g, adj_rows)) return true;
      }
      const bool lp_forced = mode == KernelMode::kQuad || mode == KernelMode::kOcto || mode == KernelMode::kHexa ||
                             mode == KernelMode::kR32 || mode == KernelMode::kAdj8 || mode == KernelMode::kAdj16;
      if ((lp_forced || (dflt && other != kVarSingle)) && c.addressable(rows)) {
        const LpGeom g = lp_geom(c, rows, 64 / rows);
        if (fold && !g.folds) return false;
        if (launch_form_quad_allr<INTEG>(c, g, rows)) return true;
      }
      if (fold) return false;   // (no kernel that prepares its own walkers serves this launch: the caller launches prep_profiles)
    } else if ((mode == KernelMode::kQuad || mode == KernelMode::kOcto || (dflt && columns <= kQuadRaysMaxColumns)) && fits32) {
      // rules 0 / 2: one ray per lane for the launches that leave the chip mostly idle, eight rows for the smallest
      if (launch_form_quad_rays<INTEG>(c, mode == KernelMode::kOcto || (dflt && columns <= kOctoRaysMaxColumns) ? 8 : 4)) return true;
    }
    return launch_form_slant<INTEG>(c);
  }
  // `cut vertical`: quad-layer while the columns leave SIMDs empty, the producer / consumer pair (rules 0 / 2) for the first
  // columns that have to share one, single-wave beyond (the measurements at the top of this file)
  constexpr long quad_max = INTEG == kIntegSimpson ? kQuadMaxColumnsSimpson : kQuadMaxColumns;
  if ((mode == KernelMode::kQuad || mode == KernelMode::kOcto || (dflt && columns <= quad_max)) && fits32 &&
      launch_form_quad<INTEG>(c, octo ? 8 : 4))
    return true;
  if constexpr (INTEG != kIntegSimpson) {
    if ((mode == KernelMode::kSplit || (dflt && columns >= kSplitMinColumns && columns <= kSplitMaxColumns)) &&
        launch_form_split<INTEG>(c))
      return true;
  }
  return launch_form_single<INTEG>(c, mode != KernelMode::kMonoOcc && (mode == KernelMode::kMonoIlp || columns < kIlpMaxColumns));
}

}  // namespace bartrt
