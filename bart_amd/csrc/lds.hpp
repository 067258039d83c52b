// Dynamic LDS of a launch: up to 64 kB a kernel takes as it is; above that, up to the 160 kB a gfx950 workgroup can
// hold, HIP asks for the kernel to be opted in (hipFuncAttributeMaxDynamicSharedMemorySize).  Measured on an MI355X
// (MEASUREMENTS.md, round 11): the runtime launched 66-73 kB requests of kernels that were not opted in, so the opt-in
// is kept for what the interface documents, not for a refusal seen.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace bartrt {

constexpr size_t kLdsDefault = 64 * 1024, kLdsMax = 160 * 1024;

// `allowed`: what this kernel has been opted into so far (one static per kernel, starting at or below kLdsDefault),
// so that the attribute is set once per size reached and never on the launches that fit anyway.
template <class K>
inline hipError_t allow_lds(K kernel, size_t bytes, size_t &allowed) {
  if (bytes <= allowed) return hipSuccess;
  if (bytes > kLdsMax) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) allowed = bytes;
  return e;
}

}  // namespace bartrt
