// The single-wave eclipse kernel of integration rule 1 for five ray angles (rt_eclipse_simpson, rt_eclipse_s1.hpp), with
// the table and with the line-by-line extinction array as input, compiled under the compiler's maximum-ILP scheduling
// strategy (bart_amd/build.py passes -mllvm -amdgpu-sched-strategy=max-ilp for this file; launch_form_single in
// rt_launch.hpp has the figures: this is the rule's only single-wave build).
#include "rt_launch.hpp"

#define BARTRT_S1_ILP(MM, CC) BARTRT_K(simpson, 5, MM, CC, true, 1) BARTRT_K(simpson, 5, MM, CC, false, 1)
#define BARTRT_S1_EXT(CC) BARTRT_K(simpson, 5, 0, CC, true, 1, true) BARTRT_K(simpson, 5, 0, CC, false, 1, true)
#define BARTRT_UNIT i1_ilp
#define BARTRT_UNIT_KERNELS BARTRT_MC_LIST(BARTRT_S1_ILP) BARTRT_EXT_C_LIST(BARTRT_S1_EXT)
#include "rt_eclipse_unit.inc"
