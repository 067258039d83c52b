// Integration rule 1 (integ.hpp) under the default schedule, five ray angles: the layer-parallel kernel of `cut slant` with
// all rays per lane (R = 32 / 16 / 8 / 4) and of `cut vertical` -- and the rule's launcher (launch_rt_spec<1>,
// rt_launch.hpp; one translation unit per rule keeps the build parallel).  The rule's single-wave kernels are built under
// the ILP schedule: rt_eclipse_i1_ilp.hip, rt_eclipse_slant_ilp.hip.
#include "rt_launch.hpp"

#define BARTRT_QUAD_ALLR_SQ(MM, CC, SQ)                                                                      \
  BARTRT_K(quad, 5, MM, CC, SQ, 8, 1, false, true) BARTRT_K(quad, 5, MM, CC, SQ, 4, 1, false, true)          \
  BARTRT_K(quad, 5, MM, CC, SQ, 16, 1, false, true) BARTRT_K(quad, 5, MM, CC, SQ, 32, 1, false, true)
#define BARTRT_QUAD_ALLR(MM, CC) BARTRT_QUAD_ALLR_SQ(MM, CC, true) BARTRT_QUAD_ALLR_SQ(MM, CC, false)
#define BARTRT_QUAD(MM, CC) \
  BARTRT_K(quad, 5, MM, CC, true, 8, 1) BARTRT_K(quad, 5, MM, CC, true, 4, 1) BARTRT_K(quad, 5, MM, CC, false, 8, 1) BARTRT_K(quad, 5, MM, CC, false, 4, 1)
#define BARTRT_UNIT i1
#define BARTRT_UNIT_KERNELS BARTRT_MC_LIST(BARTRT_QUAD_ALLR) BARTRT_MC_LIST(BARTRT_QUAD)
#include "rt_eclipse_unit.inc"

namespace bartrt {
template bool launch_rt_spec<1>(const RtArgs &, int, hipStream_t, KernelMode, bool, bool, hipError_t &,
                                RtLaunchInfo *, const PrepArgs *);
}  // namespace bartrt
