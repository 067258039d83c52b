// The single-wave eclipse kernel of integration rule 0 for five ray angles (rt_eclipse_fast<..., SCHED = 1>), with the
// table and with the line-by-line extinction array as input, compiled under the compiler's maximum-ILP scheduling strategy
// (bart_amd/build.py passes -mllvm -amdgpu-sched-strategy=max-ilp for this file): see rt_eclipse_fast in rt_eclipse.hpp
// for what that changes, launch_rt_spec (rt_launch.hpp) for when this build is taken.
#include "rt_launch.hpp"

#define BARTRT_FAST_ILP(MM, CC) BARTRT_K(fast, 5, MM, CC, true, 0, 1) BARTRT_K(fast, 5, MM, CC, false, 0, 1)
#define BARTRT_FAST_EXT(CC) BARTRT_K(fast, 5, 0, CC, true, 0, 1, true) BARTRT_K(fast, 5, 0, CC, false, 0, 1, true)
#define BARTRT_UNIT i0_ilp
#define BARTRT_UNIT_KERNELS BARTRT_MC_LIST(BARTRT_FAST_ILP) BARTRT_EXT_C_LIST(BARTRT_FAST_EXT)
#include "rt_eclipse_unit.inc"
