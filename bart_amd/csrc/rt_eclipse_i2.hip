// Integration rule 2 (integ.hpp) under the default schedule, five ray angles: the layer-parallel kernel of `cut slant` with
// one ray per lane and of `cut vertical`, the producer / consumer pair and the single-wave kernel of `cut vertical` --
// and the rule's launcher (launch_rt_spec<2>, rt_launch.hpp; one translation unit per rule keeps the build parallel).
#include "rt_launch.hpp"

#define BARTRT_QUAD_RAYS(MM, CC) BARTRT_K(quad, 5, MM, CC, false, 8, 2, true) BARTRT_K(quad, 5, MM, CC, false, 4, 2, true)
#define BARTRT_QUAD(MM, CC) \
  BARTRT_K(quad, 5, MM, CC, true, 8, 2) BARTRT_K(quad, 5, MM, CC, true, 4, 2) BARTRT_K(quad, 5, MM, CC, false, 8, 2) BARTRT_K(quad, 5, MM, CC, false, 4, 2)
#define BARTRT_SPLIT(MM, CC) BARTRT_K(split, 5, MM, CC, true, 2) BARTRT_K(split, 5, MM, CC, false, 2)
#define BARTRT_FAST(MM, CC) BARTRT_K(fast, 5, MM, CC, true, 2) BARTRT_K(fast, 5, MM, CC, false, 2)
#define BARTRT_UNIT i2
#define BARTRT_UNIT_KERNELS BARTRT_MC_LIST(BARTRT_QUAD_RAYS) BARTRT_MC_LIST(BARTRT_QUAD) BARTRT_MC_LIST(BARTRT_SPLIT) BARTRT_MC_LIST(BARTRT_FAST)
#include "rt_eclipse_unit.inc"

namespace bartrt {
template bool launch_rt_spec<2>(const RtArgs &, int, hipStream_t, KernelMode, bool, bool, hipError_t &,
                                RtLaunchInfo *, const PrepArgs *);
}  // namespace bartrt
