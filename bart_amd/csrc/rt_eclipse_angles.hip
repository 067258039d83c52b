// The single-wave eclipse kernels for ONE ray-grid size other than the usual five angles (`raygrid` is free-form,
// examples/demo/BART_eclipse.cfg:135): this file is compiled once per size wanted ahead of time (bart_amd/build.py,
// BARTRT_AOT_ANGLES: -DBARTRT_ANGLES=<n> and the max-ILP scheduling option, object rt_eclipse_a<n>.o) and instantiates
// rt_eclipse_fast (rule 0) and rt_eclipse_simpson (rule 1), each also in its `cut slant` form (rt_eclipse_fast<..., SLANT>,
// rt_eclipse_simpson_slant), for that size over the (molecules, CIA pairs) list -- without the squared-transmittance
// shortcut, which is tied to the 0 / 60 degree pair of the usual grid.  launch_rt_spec (rt_launch.hpp) takes these at
// every batch size; the layer-parallel and producer / consumer kernels exist for five angles only.  Rule 2 runs the
// generic kernel; sizes not built ahead of time are instantiated at run time.
#include "rt_launch.hpp"

#ifndef BARTRT_ANGLES
#error "compile with -DBARTRT_ANGLES=<ray-grid size>"
#endif

#define BARTRT_ANG(MM, CC)                                                                                       \
  BARTRT_K(fast, BARTRT_ANGLES, MM, CC, false, 0, 1, false, true)   /* the cut on each ray's slant depth */ \
  BARTRT_K(simpson_slant, BARTRT_ANGLES, MM, CC, false, (BARTRT_ANGLES <= 6 ? 1 : 0))                            \
  BARTRT_K(fast, BARTRT_ANGLES, MM, CC, false, 0, 1) BARTRT_K(simpson, BARTRT_ANGLES, MM, CC, false, 1)
#define BARTRT_UNIT_NAME2(n) a##n
#define BARTRT_UNIT_NAME(n) BARTRT_UNIT_NAME2(n)
#define BARTRT_UNIT BARTRT_UNIT_NAME(BARTRT_ANGLES)
#define BARTRT_UNIT_KERNELS BARTRT_MC_LIST(BARTRT_ANG)
#include "rt_eclipse_unit.inc"
