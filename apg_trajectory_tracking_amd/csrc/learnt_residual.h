// learnt_residual.h - LearntDynamics (neural_control/dynamics/
// quad_dynamics_trained.py:10-69) inside the closed-loop evaluation kernels
// (VERDICT r4 missing #2: the reference's train_dynamics() flow flies the
// LEARNT simulator in evaluate_model, scripts/train_drone.py:44-45, 205-238):
//   a' = A a                                  4 x 4 action transform (:62-64)
//   s' = flightmare(s, a') + W2 relu(W1 [s, a'] + b1) + b2     (:52-58, 66-69)
// with the kinv / inertia of construction time in the step (the reference's
// torch.diag copies, :48-50: the parameter struct the caller hands over).
// The weights sit in LDS behind the policy tables, re-ordered so that a hidden
// unit's 16 input weights and its 12 output weights are 16-byte rows: both
// half-waves of a trajectory take 32 of the 64 hidden units each and exchange
// the 12 sums (one wave = 32 trajectories, policy_mfma.h).
#pragma once
#include "learnt_pack.h"
#include "policy_mfma.h"
#include "quad_math.h"

namespace apg {

// the block of learnt_pack.h at dst:
// [W1 [64][16] | b1 [64] | W2^T [64][12] | b2 [12] | A [4][4]]
static __global__ __launch_bounds__(256) void learnt_pack_kernel(ApgLearntResidual m, float *dst) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 1024) dst[kLrW1 + t] = m.w1[t];
  if (t < 64) dst[kLrB1 + t] = m.b1[t];
  if (t < 768) dst[kLrW2 + t] = m.w2[(t % 12) * 64 + t / 12];
  if (t < 12) dst[kLrB2 + t] = m.b2[t];
  if (t < 16) dst[kLrA + t] = m.linear_at ? m.linear_at[t] : (t % 5 == 0 ? 1.f : 0.f);
  if (t >= kLrA + 16 && t < kLearntFloats) dst[t] = 0.f;
}

// s += W2 relu(W1 x + b1) + b2 for x = [state before the step, action]: the 64
// hidden units split between the two half-waves of a trajectory
__device__ __forceinline__ void learnt_residual_add(float (&s)[12], const float (&x)[16],
                                                    const float *lr, int hi) {
  typedef float f32x4_lr __attribute__((ext_vector_type(4)));
  float add[12];
#pragma unroll
  for (int o = 0; o < 12; ++o) add[o] = 0.f;
  // (opaque half-wave offset: the unit loop's LDS addresses are base + immediate)
  int u0 = 32 * hi;
  asm volatile("" : "+v"(u0));
  const float *w1 = lr + kLrW1 + u0 * 16, *b1 = lr + kLrB1 + u0, *w2 = lr + kLrW2 + u0 * 12;
#pragma unroll 2
  for (int m = 0; m < 32; ++m) {
    float h = b1[m];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4_lr w = *reinterpret_cast<const f32x4_lr *>(w1 + m * 16 + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) h = fmaf(w[j], x[4 * q + j], h);
    }
    h = fmaxf(h, 0.f);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const f32x4_lr w = *reinterpret_cast<const f32x4_lr *>(w2 + m * 12 + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) add[4 * q + j] = fmaf(w[j], h, add[4 * q + j]);
    }
  }
#pragma unroll
  for (int o = 0; o < 12; ++o) s[o] += add[o] + other_half(add[o]) + lr[kLrB2 + o];
}

// one environment step through the learnt quadrotor simulator; `lr`: the packed
// weights in LDS; both half-waves of a trajectory end with the same state
__device__ __forceinline__ void learnt_quad_step(float (&s)[12], const float (&act)[4],
                                                 const QuadConst &c, const Trig &t,
                                                 const float *lr, int hi) {
  typedef float f32x4_lr __attribute__((ext_vector_type(4)));
  float x[16];
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = s[i];
  float at[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4_lr a = *reinterpret_cast<const f32x4_lr *>(lr + kLrA + 4 * i);
    x[12 + i] = at[i] =
        fmaf(a[3], act[3], fmaf(a[2], act[2], fmaf(a[1], act[1], a[0] * act[0])));
  }
  quad_step(s, at, c, t);
  learnt_residual_add(s, x, lr, hi);
}

// The mirror of learnt_residual_add: gx = W1^T (relu' . W2^T lam) for the
// cotangent lam of the step's result, in the same half-wave split.  Each half
// recomputes its 32 hidden pre-activations from x = [state before the step,
// transformed action], forms gh_m = sum_q W2^T[m][q] lam_q under the relu's
// mask and accumulates gx_i += W1[m][i] gh_m; the halves exchange the 16 sums
// (own + other: the same bits in both).  The packed rows serve as they are:
// a unit's W1 row of 16 is read once for both products.
__device__ __forceinline__ void learnt_residual_adjoint(float (&gx)[16], const float (&lam)[12],
                                                        const float (&x)[16], const float *lr,
                                                        int hi) {
  typedef float f32x4_lr __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int i = 0; i < 16; ++i) gx[i] = 0.f;
  int u0 = 32 * hi;
  asm volatile("" : "+v"(u0));
  const float *w1 = lr + kLrW1 + u0 * 16, *b1 = lr + kLrB1 + u0, *w2 = lr + kLrW2 + u0 * 12;
#pragma unroll 2
  for (int m = 0; m < 32; ++m) {
    float h = b1[m], wr[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4_lr w = *reinterpret_cast<const f32x4_lr *>(w1 + m * 16 + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wr[4 * q + j] = w[j];
        h = fmaf(w[j], x[4 * q + j], h);
      }
    }
    float gh = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const f32x4_lr w = *reinterpret_cast<const f32x4_lr *>(w2 + m * 12 + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) gh = fmaf(w[j], lam[4 * q + j], gh);
    }
    gh = h > 0.f ? gh : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) gx[i] = fmaf(wr[i], gh, gx[i]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) gx[i] += other_half(gx[i]);
}

// Adjoint of learnt_quad_step: lam = dL/d(next state) on entry, dL/d(state) on
// exit; ga += dL/d(action) through linear_at^T; `pre` = the state the step
// started from, `act` the policy's action (before the transform).  The
// simulator's own parameters are frozen: nothing is produced for them.
__device__ __forceinline__ void learnt_quad_step_adjoint(float (&lam)[12], float (&ga)[4],
                                                         const float (&pre)[12],
                                                         const float (&act)[4],
                                                         const QuadConst &c, const float *lr,
                                                         int hi) {
  typedef float f32x4_lr __attribute__((ext_vector_type(4)));
  float x[16], gx[16];
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = pre[i];
  f32x4_lr a[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = *reinterpret_cast<const f32x4_lr *>(lr + kLrA + 4 * i);
    x[12 + i] =
        fmaf(a[i][3], act[3], fmaf(a[i][2], act[2], fmaf(a[i][1], act[1], a[i][0] * act[0])));
  }
  learnt_residual_adjoint(gx, lam, x, lr, hi);   // (before lam is overwritten)
  const Trig t = make_trig(&pre[3]);
  float gap[4] = {0.f, 0.f, 0.f, 0.f};
  const float w[3] = {pre[9], pre[10], pre[11]};
  quad_step_adjoint(lam, gap, x[12], w, c, t);
#pragma unroll
  for (int i = 0; i < 12; ++i) lam[i] += gx[i];
#pragma unroll
  for (int r = 0; r < 4; ++r) gap[r] += gx[12 + r];
#pragma unroll
  for (int i = 0; i < 4; ++i)   // linear_at^T
    ga[i] += fmaf(a[3][i], gap[3], fmaf(a[2][i], gap[2], fmaf(a[1][i], gap[1], a[0][i] * gap[0])));
}

}  // namespace apg
