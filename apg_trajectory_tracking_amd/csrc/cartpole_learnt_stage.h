// cartpole_learnt_stage.h - how a kernel takes a LearntCartpoleDynamics module
// (ApgCartpoleLearnt: DEVICE pointers to the module's own tensors) in: the six
// physical parameters read when the kernel runs, the residual's 640 weights
// staged once per workgroup into LDS as the packed unit rows of
// cartpole_learnt_math.h.  Device only; shared by cartpole_learnt.hip and the
// learnt controller step of cartpole_train.hip.
#pragma once
#include "cartpole_learnt_math.h"

namespace apg {
namespace {

// the residual's unit rows into LDS (all threads of the workgroup; barrier)
__device__ __forceinline__ void stage_residual(float *rows, const ApgCartpoleLearnt &m) {
  for (int t = threadIdx.x; t < kCartResFloats; t += blockDim.x)
    rows[t] = cart_residual_packed(t, m.w1, m.b1, m.w2);
  __syncthreads();
}

__device__ __forceinline__ CartLearntParams load_params(const ApgCartpoleLearnt &m) {
  return CartLearntParams{*m.max_force_mag, *m.masspole, *m.length,
                          *m.friction,      *m.total_mass, *m.polemass_length};
}

}  // namespace
}  // namespace apg
