// cartpole_rollout_math.h - the controller branch of TrainCartpole.run_epoch
// for ONE trajectory: H steps from s0, cartpole_loss_mpc (neural_control/
// drone_loss.py:136-145) against make_reference (scripts/train_cartpole.py:
// 103-110: ref_k = s0 (1 - k / (H - 1)), the last row zero) and the reverse
// sweep, the gradient flowing through the reference as well.  Shared by the
// rollout kernels of cartpole.hip / cartpole_learnt.hip and their host twins
// (cpu_twins.hip), which bring the step, its adjoint and where things live:
//   action(k); ST(k, i) -> float &, component i of the state BEFORE step k;
//   step(s, a) in place; emit_state(k, s), the state after step k;
//   adjoint(lam, pre, a): lam from dL/dnext to dL/dstate of the step from
//   `pre`, returns dL/da without the action cost; emit_grad_action(k, g).
// Two functions: the device writes its wave's loss partial between them.
#pragma once
#include "cartpole_math.h"

namespace apg {
namespace {

// Returns the trajectory's loss; s: the state after the last step.
template <class Action, class Stash, class Step, class EmitState>
__host__ __device__ __forceinline__ float cart_rollout_forward(
    int H, const float (&s0)[4], float (&s)[4], Action &&action, Stash &&ST, Step &&step,
    EmitState &&emit_state) {
  const float wq[4] = {0.f, 3.f, 10.f, 1.f};  // drone_loss.py:136
  const double inv = H > 1 ? 1.0 / (double)(H - 1) : 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = s0[i];
  float loss = 0.f;
  for (int k = 0; k < H; ++k) {
    const float a = action(k);
#pragma unroll
    for (int i = 0; i < 4; ++i) ST(k, i) = s[i];
    step(s, a);
    emit_state(k, s);
    const float f = k < H - 1 ? (float)(1.0 - inv * (double)k) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float d = s[i] - s0[i] * f;
      loss += (d * d) * wq[i];
    }
    loss += 0.01f * a * a;
  }
  return loss;
}

// s: the state cart_rollout_forward left; lam: dL/dstate0 on return
template <class Action, class Stash, class Adjoint, class EmitGrad>
__host__ __device__ __forceinline__ void cart_rollout_reverse(
    int H, const float (&s0)[4], const float (&s)[4], float (&lam)[4], Action &&action,
    Stash &&ST, Adjoint &&adjoint, EmitGrad &&emit_grad_action) {
  const float wq[4] = {0.f, 3.f, 10.f, 1.f};
  const double inv = H > 1 ? 1.0 / (double)(H - 1) : 0.0;
  float g0[4] = {0.f, 0.f, 0.f, 0.f}, nxt[4] = {s[0], s[1], s[2], s[3]};
#pragma unroll
  for (int i = 0; i < 4; ++i) lam[i] = 0.f;
  for (int k = H - 1; k >= 0; --k) {
    const float a = action(k);
    const float f = k < H - 1 ? (float)(1.0 - inv * (double)k) : 0.f;
    float pre[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pre[i] = ST(k, i);
      const float seed = 2.f * wq[i] * (nxt[i] - s0[i] * f);
      lam[i] += seed;
      g0[i] -= seed * f;  // gradient through make_reference
    }
    emit_grad_action(k, adjoint(lam, pre, a) + 0.02f * a);
#pragma unroll
    for (int i = 0; i < 4; ++i) nxt[i] = pre[i];  // after step k - 1 = before step k
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) lam[i] += g0[i];
}

// cart_step's aux of the step from `pre`, recomputed for its adjoint
__host__ __device__ __forceinline__ CartAux cart_step_aux(const float (&pre)[4], float a,
                                                          const CartConst &c) {
  float tmp[4] = {pre[0], pre[1], pre[2], pre[3]};
  return cart_step(tmp, a, c);
}

}  // namespace
}  // namespace apg
