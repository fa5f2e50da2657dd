// quad_learnt_mpc_math.h - the LEARNT simulator (LearntDynamics,
// neural_control/dynamics/quad_dynamics_trained.py:10-69) as a model of the
// shooting solver of quad_mpc_math.h - the role of the reference's
// LearntDynamicsMPC (neural_control/dynamics/learnt_dynamics.py:5-55: "for using
// the dynamics model in MPC"), one trajectory per lane:
//   a' = A a
//   s' = quad_step(s, a') + W2 relu(W1 [s, a'] + b1) + b2
// on the packed block of learnt_pack.h (device: in LDS; host twin: an array).
// The cost stays the solver's, on the policy's action a (not on a'), as in
// apg_quad_learnt_rollout_fwd_bwd; the simulator's own parameters are frozen:
// nothing is produced for them.
#pragma once
#include "learnt_pack.h"
#include "quad_mpc_math.h"

namespace apg {
namespace {

// a' = A a, the fmaf chain of learnt_residual.h (forward and adjoint form the
// same bits)
template <class P>
__host__ __device__ __forceinline__ void learnt_action(P lr, const float (&act)[4],
                                                       float (&at)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    P a = lr + kLrA + 4 * i;
    at[i] = fmaf(a[3], act[3], fmaf(a[2], act[2], fmaf(a[1], act[1], a[0] * act[0])));
  }
}

// LearntDynamics.forward for ONE trajectory per lane (learnt_residual.h has the
// half-wave form of the policy kernels): a' = A a, the analytic step on a',
// plus W2 relu(W1 [s, a'] + b1) + b2; `lr`: the packed weights
template <class P>
__host__ __device__ __forceinline__ void learnt_quad_step_lane(float (&s)[12],
                                                               const float (&act)[4],
                                                               const QuadConst &c, const Trig &t,
                                                               P lr) {
  float x[16], at[4], add[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = s[i], add[i] = lr[kLrB2 + i];
  learnt_action(lr, act, at);
#pragma unroll
  for (int i = 0; i < 4; ++i) x[12 + i] = at[i];
  quad_step(s, at, c, t);
#pragma unroll 2
  for (int m = 0; m < 64; ++m) {
    float h = lr[kLrB1 + m];
#pragma unroll
    for (int j = 0; j < 16; ++j) h = fmaf(lr[kLrW1 + m * 16 + j], x[j], h);
    h = fmaxf(h, 0.f);
#pragma unroll
    for (int o = 0; o < 12; ++o) add[o] = fmaf(lr[kLrW2 + m * 12 + o], h, add[o]);
  }
#pragma unroll
  for (int o = 0; o < 12; ++o) s[o] += add[o];
}

// Its adjoint.  lam = dL/d(next state) on entry, dL/d(state) on exit; ga +=
// dL/d(action) through linear_at^T; `pre`: the state the step started from, `at`
// the TRANSFORMED action, t the sin / cos of pre's attitude.  All 64 hidden
// pre-activations are recomputed from [pre, at]: per unit gh = relu'(z) (W2^T
// lam), gx += W1 row . gh - the unit's W1 row is read once for both products.
template <class P>
__host__ __device__ __forceinline__ void learnt_quad_step_lane_adjoint(
    float (&lam)[12], float (&ga)[4], const float (&pre)[12], const float (&at)[4],
    const QuadConst &c, const Trig &t, P lr) {
  float x[16], gx[16];
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = pre[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) x[12 + i] = at[i];
#pragma unroll
  for (int i = 0; i < 16; ++i) gx[i] = 0.f;
#pragma unroll 2
  for (int m = 0; m < 64; ++m) {
    float h = lr[kLrB1 + m], wr[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      wr[j] = lr[kLrW1 + m * 16 + j];
      h = fmaf(wr[j], x[j], h);
    }
    float gh = 0.f;
#pragma unroll
    for (int o = 0; o < 12; ++o) gh = fmaf(lr[kLrW2 + m * 12 + o], lam[o], gh);
    gh = h > 0.f ? gh : 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) gx[j] = fmaf(wr[j], gh, gx[j]);
  }
  float gap[4] = {0.f, 0.f, 0.f, 0.f};
  const float w[3] = {pre[9], pre[10], pre[11]};
  quad_step_adjoint(lam, gap, at[0], w, c, t);   // (after gx: it overwrites lam)
#pragma unroll
  for (int i = 0; i < 12; ++i) lam[i] += gx[i];
#pragma unroll
  for (int r = 0; r < 4; ++r) gap[r] += gx[12 + r];
#pragma unroll
  for (int i = 0; i < 4; ++i) {   // linear_at^T
    P a = lr + kLrA;
    ga[i] += fmaf(a[12 + i], gap[3], fmaf(a[8 + i], gap[2], fmaf(a[4 + i], gap[1], a[i] * gap[0])));
  }
}

// The stride between two floats of one trajectory's stash: on the device the
// stash is LDS, [row][64 lanes], so that a wave's access is one conflict-free
// row; on the host a plain array
#if defined(__HIP_DEVICE_COMPILE__)
constexpr int kMpcPreStride = 64;
#else
constexpr int kMpcPreStride = 1;
#endif
constexpr int kMpcPreRow = 12;   // floats per step and trajectory

// The learnt model of the solver.  Of the forward sweep its adjoint keeps the
// state before every step, in `pre` ([H][12] floats kMpcPreStride apart, the
// caller's: on the device the unknowns, the momentum, the window and the loss
// residuals already take half of the unified register file); the transformed
// action and the sin / cos are formed again from u[k] and that state.  Inside
// the horizon the sin / cos is the solver's software pair (mpc_trig).
template <class P>
struct MpcLearnt {
  const QuadConst &c;
  P lr;         // the packed block (learnt_pack.h)
  float *pre;
  template <int H>
  struct Stash {};
  template <bool STASH, int H>
  __host__ __device__ __forceinline__ void step(int k, float (&s)[12], const float (&u)[4],
                                                Stash<H> &) const {
    if (STASH) {
#pragma unroll
      for (int i = 0; i < 12; ++i) pre[(k * kMpcPreRow + i) * kMpcPreStride] = s[i];
    }
    learnt_quad_step_lane(s, u, c, mpc_trig(&s[3]), lr);
  }
  template <int H>
  __host__ __device__ __forceinline__ void adjoint(int k, float (&lam)[12], float (&ga)[4],
                                                   const float (&u)[4], const float[3],
                                                   const Stash<H> &) const {
    float s[12], at[4];
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = pre[(k * kMpcPreRow + i) * kMpcPreStride];
    learnt_action(lr, u, at);
    learnt_quad_step_lane_adjoint(lam, ga, s, at, c, mpc_trig(&s[3]), lr);
  }
};

// argument rule shared by the device entry points and the twins; NULL: fine.
// There is no falling back to the analytic model: that one has its own entry
// points.
inline const char *learnt_mpc_check_model(const ApgLearntResidual *m) {
  if (!m) return "model_learnt is NULL (the analytic model is apg_quad_mpc_*)";
  if (!m->linear_at || !m->w1 || !m->b1 || !m->w2 || !m->b2)
    return "model_learnt: weight pointer is NULL";
  return nullptr;
}

}  // namespace
}  // namespace apg
