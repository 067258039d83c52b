// The single-wave eclipse kernels with the `toomuch` cut on each ray's slant depth (cfg `cut slant`) for the
// usual five-angle ray grid, compiled under the compiler's maximum-ILP scheduling strategy (bart_amd/build.py): rule 1's
// own kernel (rt_eclipse_simpson_slant, rt_eclipse_s1s.hpp), rule 0's (rt_eclipse_fast<..., SLANT = true> with
// ColumnFluxSlant, integ.hpp) and rule 2's (the same kernel with rule 2's masked accumulator); rule 1 with the
// optical-depth / per-ray-intensity outputs of a single walker (OUT; the ray angles in the cfg's order: no
// squared-transmittance pairing); rules 0 / 1 with the line-by-line extinction array as input.
//
// The record read-ahead (SCHED 1: a layer reads the NEXT layer's record while it computes) pays on the shapes it was
// tuned on -- up to twelve table loads per layer -- and drowns wider ones in spills: <5, 6, 2> (sixteen loads) 294
// registers spilled against 22 without it, <5, 4, 4> (BART's usual H2-H2 + H2-He under the spline) 161 against 26;
// measured on six molecules: 762 -> 3xx us at 26 walkers (round 6, slant_sched in rt_eclipse.hpp).
#include "rt_launch.hpp"

#define BARTRT_SLANT(MM, CC)                                                                                                \
  BARTRT_K(simpson_slant, 5, MM, CC, true, slant_sched(MM, CC, 1)) BARTRT_K(simpson_slant, 5, MM, CC, false, slant_sched(MM, CC, 1)) \
  BARTRT_K(fast, 5, MM, CC, true, 0, 1, false, true) BARTRT_K(fast, 5, MM, CC, false, 0, 1, false, true)                    \
  BARTRT_K(fast, 5, MM, CC, true, 2, 1, false, true) BARTRT_K(fast, 5, MM, CC, false, 2, 1, false, true)
#define BARTRT_SLANT_OUT(MM, CC) BARTRT_K(simpson_slant, 5, MM, CC, false, 0, false, true)
#define BARTRT_SLANT_EXT(CC)                                                                              \
  BARTRT_K(simpson_slant, 5, 0, CC, true, 1, true) BARTRT_K(simpson_slant, 5, 0, CC, false, 1, true)      \
  BARTRT_K(fast, 5, 0, CC, true, 0, 1, true, true) BARTRT_K(fast, 5, 0, CC, false, 0, 1, true, true)
#define BARTRT_UNIT slant_ilp
#define BARTRT_UNIT_KERNELS BARTRT_MC_LIST(BARTRT_SLANT) BARTRT_MC_LIST(BARTRT_SLANT_OUT) BARTRT_EXT_C_LIST(BARTRT_SLANT_EXT)
#include "rt_eclipse_unit.inc"
