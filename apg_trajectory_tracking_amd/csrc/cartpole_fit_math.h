// cartpole_fit_math.h - per-lane arithmetic and the row layout of the fused
// simulator-fit step of the learnt cart-pole (cartpole_fit.hip:
// apg_cartpole_learnt_fit_fwd_bwd; host twin in cpu_twins.hip):
// TrainBase.train_dynamics_model (scripts/train_base.py:160-186) with
// LearntCartpoleDynamics as train dynamics,
//   pred = simulate_cartpole(s, a) + W2 relu(W1 [s; a] + b1)
//   loss = sum (pred - target)^2,   lam = 2 (pred - target)
// The step, the parameter cotangents and a unit's weight cotangents are those
// of cartpole_learnt_math.h; this header adds their composition for one sample
// and where a column of a workgroup's partial row lands in the flat gradient.
#pragma once
#include "cartpole_learnt_math.h"

namespace apg {
namespace {

// A partial row: [6 physical cotangents, padded to 32 | 10 planes of 64: plane
// j = element j of every hidden unit's row [dW1[m][0..4], db1[m], dW2[0..3][m]]]
constexpr int kCartFitHead = 32;
constexpr int kCartFitRow = kCartFitHead + kCartResRow * kCartResHidden;   // 672
static_assert(kCartFitRow == 672 && kCartPhysGrads <= kCartFitHead, "row layout");

// where column c of a row goes in the gradient of apg_cartpole_learnt_step_bwd
// ([6 physical | W1 [64][5] | b1 [64] | W2 [4][64]]); -1: padding
__host__ __device__ __forceinline__ int cart_fit_dest(int c) {
  if (c < kCartFitHead) return c < kCartPhysGrads ? c : -1;
  const int j = (c - kCartFitHead) / kCartResHidden;
  const int m = (c - kCartFitHead) - j * kCartResHidden;
  if (j < 5) return kCartGW1 + m * 5 + j;
  if (j == 5) return kCartGB1 + m;
  return kCartGW2 + (j - 6) * kCartResHidden + m;
}

// One sample of the fit: the learnt step from s, the squared error against tgt
// (returned), lam = 2 (pred - tgt) and the six physical cotangents ADDED to g.
// rows: the residual's packed unit rows (cart_residual_packed).
__host__ __device__ __forceinline__ float cart_fit_sample(const float (&s)[4], float a,
                                                          const float (&tgt)[4],
                                                          const CartLearntParams &p,
                                                          const CartConst &c, float dt,
                                                          const float *rows,
                                                          float (&lam)[4], float (&g)[6]) {
  float pred[4] = {s[0], s[1], s[2], s[3]};
  const CartAux x = cart_learnt_step(pred, a, c, rows);
  float loss = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float d = pred[i] - tgt[i];
    loss = fmaf(d, d, loss);
    lam[i] = 2.f * d;
  }
  cart_param_adjoint(lam, a, s[1], s[3], x, p, dt, g);
  return loss;
}

}  // namespace
}  // namespace apg
