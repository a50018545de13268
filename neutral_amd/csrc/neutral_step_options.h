/*
 * neutral_step_options.h -- the device's copy of a step's optional scoring (StepOptions,
 * neutral_kernels.h) and the choice of a kernel instantiation by it.  Included by each
 * translation unit whose kernels score (neutral_kernels.hip, neutral_tiled.hip): the build is
 * not relocatable device code, so each gets a copy and a setter kernel of its own.
 */
#ifndef NEUTRAL_AMD_STEP_OPTIONS_H
#define NEUTRAL_AMD_STEP_OPTIONS_H

#include "neutral_kernels.h"

#include <type_traits>

namespace neutral {

/* Read by the instantiations with a Score only, and there at the point of use (the collision
 * buffer and the current's meshes at each flush, a scalar load: neutral_history.h). */
static __device__ StepOptions d_options = {};

static __global__ void step_options_kernel(StepOptions o) {
  if (o.periodic.axes != 0u && o.periodic.edges[0] != nullptr) {
    /* (periodic axes: the mesh's extent from its own edges -- see PeriodicParams) */
    o.periodic.width = __dsub_rn(*o.periodic.edges[1], *o.periodic.edges[0]);
    o.periodic.height = __dsub_rn(*o.periodic.edges[3], *o.periodic.edges[2]);
  }
  d_options = o;
}

/* `wanted`: the scores this translation unit's kernels read the options for */
static hipError_t upload_step_options(const StepOptions& o, unsigned wanted, hipStream_t stream) {
  if ((scores_of(o) & wanted) == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(step_options_kernel, dim3(1), dim3(1), 0, stream, o);
  return hipGetLastError();
}

/* f(std::integral_constant<unsigned, value>{}) for a run-time value of kBits bits: what turns
 * the properties a launch asks for into template arguments.  f is instantiated for every value;
 * it says with `if constexpr` which of them it has a kernel for, and returns an error for the
 * others. */
template <int kBits, unsigned kKnown = 0, typename F>
static hipError_t with_constant(unsigned value, const F& f) {
  if constexpr (kBits == 0) {
    return f(std::integral_constant<unsigned, kKnown>{});
  } else {
    constexpr unsigned kBit = 1u << (kBits - 1);
    return (value & kBit) ? with_constant<kBits - 1, (kKnown | kBit)>(value, f)
                          : with_constant<kBits - 1, kKnown>(value, f);
  }
}

}  // namespace neutral
#endif
