// wing_rollout_math.h - the plain fixed-wing controller rollout for ONE
// trajectory: H steps, fixed_wing_mpc_loss (neural_control/drone_loss.py:72-82)
// and the reverse sweep, every pre-step state stashed.  Shared by
// wing_learnt_rollout_kernel (wing_learnt.hip) and the host twins of both
// fixed-wing rollouts (cpu_twins.hip) - NOT by wing_rollout_lds_kernel
// (wing.hip): checkpointed, software-pipelined.  The callbacks are those of
// cartpole_rollout_math.h with action(k, a[4]), ref(k, rp[3]) and
// adjoint(lam, ga, pre, a): ga from the action cost's gradient to dL/da.
#pragma once

namespace apg {
namespace {

// s: the initial state in, the state after the last step out; returns the loss
template <class Action, class Ref, class Stash, class Step, class EmitState>
__host__ __device__ __forceinline__ float wing_rollout_forward(
    int H, float (&s)[12], float w_pos, float w_act, Action &&action, Ref &&ref, Stash &&ST,
    Step &&step, EmitState &&emit_state) {
  float loss = 0.f;
  for (int k = 0; k < H; ++k) {
    float a[4], rp[3];
    action(k, a);
    ref(k, rp);
#pragma unroll
    for (int i = 0; i < 12; ++i) ST(k, i) = s[i];
    step(s, a);
    emit_state(k, s);
    float lp = 0.f, la = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float dp = s[i] - rp[i], d = a[1 + i] - 0.5f;
      lp += dp * dp, la += d * d;
    }
    loss += w_pos * lp + w_act * la;
  }
  return loss;
}

// s: the state wing_rollout_forward left; lam: dL/dstate0 on return
template <class Action, class Ref, class Stash, class Adjoint, class EmitGrad>
__host__ __device__ __forceinline__ void wing_rollout_reverse(
    int H, const float (&s)[12], float (&lam)[12], float w_pos, float w_act, Action &&action,
    Ref &&ref, Stash &&ST, Adjoint &&adjoint, EmitGrad &&emit_grad_action) {
#pragma unroll
  for (int i = 0; i < 12; ++i) lam[i] = 0.f;
  float nxt[3] = {s[0], s[1], s[2]};   // position after step k
  for (int k = H - 1; k >= 0; --k) {
    float a[4], rp[3], pre[12];
    action(k, a);
    ref(k, rp);
#pragma unroll
    for (int i = 0; i < 12; ++i) pre[i] = ST(k, i);
#pragma unroll
    for (int i = 0; i < 3; ++i) lam[i] += 2.f * w_pos * (nxt[i] - rp[i]);
    float ga[4] = {0.f, 2.f * w_act * (a[1] - 0.5f), 2.f * w_act * (a[2] - 0.5f),
                   2.f * w_act * (a[3] - 0.5f)};
    adjoint(lam, ga, pre, a);
    emit_grad_action(k, ga);
#pragma unroll
    for (int i = 0; i < 3; ++i) nxt[i] = pre[i];  // after step k - 1 = before step k
  }
}

}  // namespace
}  // namespace apg
