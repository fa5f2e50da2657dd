// cartpole_fit_math.h - per-lane arithmetic and the row layout of the fused
// simulator-fit step of the learnt cart-pole (cartpole_fit.hip:
// apg_cartpole_learnt_fit_fwd_bwd; host twin in cpu_twins.hip):
// TrainBase.train_dynamics_model (scripts/train_base.py:160-186) with
// LearntCartpoleDynamics as train dynamics,
//   pred = simulate_cartpole(s, a) + W2 relu(W1 [s; a] + b1)
//   loss = sum (pred - target)^2,   lam = 2 (pred - target)
// The step, the parameter cotangents and a unit's weight cotangents are those
// of cartpole_learnt_math.h; this header adds their composition for one sample,
// where a column of a workgroup's partial row lands in the flat gradient, and
// CartFit: what the fit's skeleton (residual_fit.h) reads of this system.
#pragma once
#include "cartpole_learnt_math.h"
#include "residual_fit.h"

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

// What residual_fit.h's shared fit reads of this system.  The model: the six
// live parameters, their step constants and the packed unit rows (device: the
// LDS copy every workgroup stages itself; host: plain).  No regulariser: the
// network has no output bias for the reference's norm term to read.
struct CartFitModel {
  CartLearntParams p;
  CartConst c;
  float dt;
  const float *rows;
};

#if defined(__HIPCC__)
// the fit kernel's arguments (residual_fit.h fills the common ones)
struct CartFitArgs {
  const float *state, *action, *target;   // target NULL: the analytic step on `eval`
  float *loss_partials, *rows;
  ApgCartpoleLearnt m;
  CartConst eval;
  float dt;
  int B;
};
#endif

struct CartFit {
  static constexpr int S = 4, A = 1, IN = 5, OUT = 4;
  static constexpr int RES_ROW = kCartResRow, RW2 = 6, RB1 = 5;
  static constexpr int UNIT = kCartResRow, UW2 = 6, UB1 = 5;   // the row's own order
  static constexpr int HEAD = kCartFitHead, USED = kCartPhysGrads, ROW = kCartFitRow;
  static constexpr int GRADS = kCartLearntGrads;
  static constexpr bool REG = false;
  static constexpr int ROWS_AT = 0;
  typedef CartConst Eval;
  typedef FitNoScale Scale;

  static __host__ __device__ __forceinline__ int dest(int c) { return cart_fit_dest(c); }
  static __host__ __device__ __forceinline__ float value(int, float v, const Scale &) {
    return v;
  }

  // the head: the six physical cotangents
  static __host__ __device__ __forceinline__ float sample(const CartFitModel &m,
                                                          const float (&s)[4],
                                                          const float (&a)[1], float (&tgt)[4],
                                                          const CartConst *eval, float (&lam)[4],
                                                          float (&z)[5], float (&hd)[USED]) {
    if (eval) {
#pragma unroll
      for (int i = 0; i < 4; ++i) tgt[i] = s[i];
      cart_step(tgt, a[0], *eval);
    }
#pragma unroll
    for (int i = 0; i < USED; ++i) hd[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = s[i];
    z[4] = a[0];
    return cart_fit_sample(s, a[0], tgt, m.p, m.c, m.dt, m.rows, lam, hd);
  }

#if defined(__HIPCC__)
  typedef CartFitArgs Args;
  static constexpr int UNROLL = 4;
  typedef CartFitModel Model;

  // no pack launch: the 640 residual floats are staged into LDS as unit rows by
  // every workgroup (the kernel's threads all arrive here)
  static __device__ __forceinline__ Model model(const Args &A) {
    __shared__ float unit[kCartResFloats];
    for (int t = threadIdx.x; t < kCartResFloats; t += kFitBlock)
      unit[t] = cart_residual_packed(t, A.m.w1, A.m.b1, A.m.w2);
    __syncthreads();
    const CartLearntParams p{*A.m.max_force_mag, *A.m.masspole,   *A.m.length,
                             *A.m.friction,      *A.m.total_mass, *A.m.polemass_length};
    return Model{p, make_learnt_const(p, A.dt), A.dt, unit};
  }
  static __device__ __forceinline__ void unit_row(const Args &, const Model &m, int lane,
                                                  float (&w)[RES_ROW]) {
#pragma unroll
    for (int j = 0; j < kCartResRow; ++j) w[j] = m.rows[lane * kCartResRow + j];
  }
#endif
};

}  // namespace
}  // namespace apg
