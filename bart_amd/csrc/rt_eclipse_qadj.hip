// rt_eclipse_qadj (rt_eclipse_qadj.hpp: rule 1 / `cut slant`, a column's rows on adjacent lanes) for five ray angles,
// R = 16 and 8, under the default schedule.
#include "rt_eclipse_qadj.hpp"
#include "rt_launch.hpp"

#define BARTRT_QADJ(MM, CC) \
  BARTRT_K(qadj, 5, MM, CC, true, 16) BARTRT_K(qadj, 5, MM, CC, false, 16) BARTRT_K(qadj, 5, MM, CC, true, 8) BARTRT_K(qadj, 5, MM, CC, false, 8)
#define BARTRT_UNIT qadj
#define BARTRT_UNIT_KERNELS BARTRT_QADJ_LIST(BARTRT_QADJ)
#include "rt_eclipse_unit.inc"
