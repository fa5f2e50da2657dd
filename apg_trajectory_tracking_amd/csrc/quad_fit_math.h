// quad_fit_math.h - per-lane arithmetic of the simulator-fit step of the learnt
// quadrotor (TrainBase.train_dynamics_model, scripts/train_base.py:160-186, on
// LearntDynamics, neural_control/dynamics/quad_dynamics_trained.py:10-69):
//   a'   = linear_at a
//   pred = quad_step(s, a') + W2 relu(W1 [s; a'] + b1) + b2
//   loss = sum (pred - target)^2,  lam = 2 (pred - target)
// and what one sample adds to the cotangent of every parameter.  The physics is
// quad_step / quad_step_adjoint of quad_math.h on the constants of construction
// time (the reference's torch.diag copies, :48-50); the residual's weights are
// read from packed unit rows; the fit's skeleton, a hidden unit's cotangents,
// the regulariser and the reduction are residual_fit.h, which reads this system
// through QuadFit below.  Called per lane by quad_fit.hip and per sample by its
// host twin (csrc/cpu_twins.hip).
#pragma once
#include "quad_math.h"
#include "residual_fit.h"

namespace apg {
namespace {

// The packed model: 64 unit rows of 29 floats [W1[m][0..15] | b1[m] |
// W2[0..11][m]], then b2 [12] (padded to 16) and linear_at [4][4].  A unit's
// weights are wave-uniform and contiguous: on the device they arrive as scalar
// operands.
constexpr int kQuadResRow = 29, kQuadResB1 = 16, kQuadResW2 = 17;
constexpr int kQuadResB2 = kResHidden * kQuadResRow;       // 1856
constexpr int kQuadResLin = kQuadResB2 + 16;               // 1872
constexpr int kQuadPackFloats = kQuadResLin + 16;          // 1888

// element t of the packed model (t < kQuadPackFloats)
__host__ __device__ __forceinline__ float quad_fit_packed(int t, const ApgLearntResidual &m) {
  if (t >= kQuadResLin) return m.linear_at[t - kQuadResLin];
  if (t >= kQuadResB2) return t - kQuadResB2 < 12 ? m.b2[t - kQuadResB2] : 0.f;
  const int u = t / kQuadResRow, j = t - u * kQuadResRow;
  if (j < kQuadResB1) return m.w1[u * 16 + j];
  if (j == kQuadResB1) return m.b1[u];
  return m.w2[(j - kQuadResW2) * kResHidden + u];
}

// The flat gradient (apg.h: APG_QUAD_FIT_*), in the order of
// LearntDynamics.parameters()
constexpr int kQuadFitGLin = 0, kQuadFitGMass = 16, kQuadFitGInertia = 17, kQuadFitGKinv = 20;
constexpr int kQuadFitGW1 = 23;                                  // [64][16]
constexpr int kQuadFitGB1 = kQuadFitGW1 + kResHidden * 16;       // 1047
constexpr int kQuadFitGW2 = kQuadFitGB1 + kResHidden;            // 1111
constexpr int kQuadFitGB2 = kQuadFitGW2 + 12 * kResHidden;       // 1879
constexpr int kQuadFitGrads = kQuadFitGB2 + 12;                  // 1891
// A partial row as the kernel sums it: head [dlinear_at (16) | dkinv (3) | sum
// lam_w' (3) | db2 (12) | zeros to 64], then 29 planes of 64: plane j < 16 =
// dW1[.][j], plane 16 + o = dW2[o][.], plane 28 = db1 - hidden unit m owns
// element m of every plane.
constexpr int kQuadFitHKinv = 16, kQuadFitHLamW = 19, kQuadFitHB2 = 22, kQuadFitHUsed = 34;
constexpr int kQuadFitHead = 64;
constexpr int kQuadFitRow = kQuadFitHead + kResFitUnit * kResHidden;   // 1920

// element c of a partial row -> its place in the flat gradient (-1: padding).
// The first padding element stands for the mass, whose gradient is exactly 0.
__host__ __device__ __forceinline__ int quad_fit_dest(int c) {
  if (c < kQuadFitHKinv) return kQuadFitGLin + c;
  if (c < kQuadFitHLamW) return kQuadFitGKinv + (c - kQuadFitHKinv);
  if (c < kQuadFitHB2) return kQuadFitGInertia + (c - kQuadFitHLamW);
  if (c < kQuadFitHUsed) return kQuadFitGB2 + (c - kQuadFitHB2);
  if (c == kQuadFitHUsed) return kQuadFitGMass;
  if (c < kQuadFitHead) return -1;
  const int j = (c - kQuadFitHead) / kResHidden, m = (c - kQuadFitHead) % kResHidden;
  if (j < 16) return kQuadFitGW1 + m * 16 + j;
  if (j < 28) return kQuadFitGW2 + (j - 16) * kResHidden + m;
  return kQuadFitGB1 + m;
}

// what the reduction needs of the construction-time constants:
// dL/dJ_i = -(sum_b lam_w'_i) dt d_r,i / J_i^2
struct QuadFitInertia {
  float dt, rot_drag[3], inertia[3];
};
inline QuadFitInertia make_fit_inertia(const ApgQuadParams &p, float dt) {
  QuadFitInertia q;
  q.dt = dt;
  for (int i = 0; i < 3; ++i) q.rot_drag[i] = p.rot_drag[i], q.inertia[i] = p.inertia[i];
  return q;
}

// the summed element c of a partial row -> the gradient at quad_fit_dest(c),
// without the regulariser
__host__ __device__ __forceinline__ float quad_fit_value(int c, float v, const QuadFitInertia &q) {
  if (c >= kQuadFitHLamW && c < kQuadFitHB2) {
    const int i = c - kQuadFitHLamW;
    return -v * q.dt * q.rot_drag[i] / (q.inertia[i] * q.inertia[i]);
  }
  return c == kQuadFitHUsed ? 0.f : v;
}

// One sample of the fit.  s, a: state and RAW action; tgt: the target; c: the
// step's constants; pack: the packed model (host: const float *, device: the
// constant address space).  Returns sum (pred - tgt)^2; lam = 2 (pred - tgt);
// x = [s; a'], the residual's input; head[0..33] = the sample's part of the
// row head (the caller keeps the padding zero).
template <typename P>
__host__ __device__ __forceinline__ float quad_learnt_fit_sample(
    const float (&s)[12], const float (&a)[4], const float (&tgt)[12], const QuadConst &c,
    const Trig &t, P pack, float (&lam)[12], float (&x)[16], float (&head)[kQuadFitHUsed]) {
  P L = pack + kQuadResLin;
  float ap[4], r[12], nxt[12];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    ap[i] = L[i * 4] * a[0] + L[i * 4 + 1] * a[1] + L[i * 4 + 2] * a[2] + L[i * 4 + 3] * a[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = nxt[i] = s[i], r[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) x[12 + i] = ap[i];
  // r = W2 relu(W1 x + b1) + b2
#pragma unroll 2
  for (int m = 0; m < kResHidden; ++m) {
    P w = pack + m * kQuadResRow;
    float h = w[kQuadResB1];
#pragma unroll
    for (int j = 0; j < 16; ++j) h = fmaf(w[j], x[j], h);
    h = fmaxf(h, 0.f);
#pragma unroll
    for (int o = 0; o < 12; ++o) r[o] = fmaf(w[kQuadResW2 + o], h, r[o]);
  }
  quad_step(nxt, ap, c, t);
  float loss = 0.f, lp[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const float d = (nxt[i] + (r[i] + pack[kQuadResB2 + i])) - tgt[i];
    loss = fmaf(d, d, loss);
    lam[i] = lp[i] = 2.f * d;
  }
  // the residual's gradient for its last four inputs, the hidden layer
  // recomputed unit by unit: W1[:, 12:16]^T (relu' o W2^T lam)
  float gap[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int m = 0; m < kResHidden; ++m) {
    P w = pack + m * kQuadResRow;
    float h = w[kQuadResB1];
#pragma unroll
    for (int j = 0; j < 16; ++j) h = fmaf(w[j], x[j], h);
    float dh = 0.f;
#pragma unroll
    for (int o = 0; o < 12; ++o) dh = fmaf(w[kQuadResW2 + o], lam[o], dh);
    dh = h > 0.f ? dh : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) gap[j] = fmaf(w[12 + j], dh, gap[j]);
  }
  const float w0[3] = {s[9], s[10], s[11]};
  quad_step_adjoint(lp, gap, ap[0], w0, c, t);   // gap += the step's action cotangent
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) head[i * 4 + j] = gap[i] * a[j];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    head[kQuadFitHKinv + i] = lam[9 + i] * (c.dt * ((ap[1 + i] - 0.5f) - s[9 + i]));
    head[kQuadFitHLamW + i] = lam[9 + i];
  }
#pragma unroll
  for (int o = 0; o < 12; ++o) head[kQuadFitHB2 + o] = lam[o];
  return loss;
}

// What residual_fit.h's shared fit reads of this system.  The model: the step's
// constants and the packed model, which starts with the unit rows (device: the
// pack in the workspace through the constant address space; host: plain).
template <class P>
struct QuadFitModel {
  const QuadConst &c;
  P rows;
};

#if defined(__HIPCC__)
// the fit kernel's arguments (residual_fit.h fills the common ones)
struct QuadFitArgs {
  const float *state, *action, *target;   // target NULL: the analytic step on `eval`
  const float *ws;                        // the pack
  float *loss_partials, *rows;
  QuadConst c, eval;
  int B;
};
#endif

struct QuadFit {
  static constexpr int S = 12, A = 4, IN = 16, OUT = 12;
  static constexpr int RES_ROW = kQuadResRow, RW2 = kQuadResW2, RB1 = kQuadResB1;
  static constexpr int UNIT = kResFitUnit, UW2 = 16, UB1 = 28;
  static constexpr int HEAD = kQuadFitHead, USED = kQuadFitHUsed, ROW = kQuadFitRow;
  static constexpr int GRADS = kQuadFitGrads;
  static constexpr bool REG = true;
  static constexpr int G_W1 = kQuadFitGW1, G_B1 = kQuadFitGB1, G_W2 = kQuadFitGW2,
                       G_B2 = kQuadFitGB2;
  static constexpr int NORMS_AT = kQuadPackFloats, ROWS_AT = NORMS_AT + 16;
  typedef QuadConst Eval;
  typedef QuadFitInertia Scale;

  static __host__ __device__ __forceinline__ int dest(int c) { return quad_fit_dest(c); }
  static __host__ __device__ __forceinline__ float value(int c, float v, const Scale &q) {
    return quad_fit_value(c, v, q);
  }

  // (the eval dynamics takes the RAW action; z = [s; a'], the transformed one)
  template <class M>
  static __host__ __device__ __forceinline__ float sample(const M &m, const float (&s)[12],
                                                          const float (&a)[4], float (&tgt)[12],
                                                          const QuadConst *eval,
                                                          float (&lam)[12], float (&z)[16],
                                                          float (&hd)[USED]) {
    const Trig t = make_trig(&s[3]);
    if (eval) {
#pragma unroll
      for (int i = 0; i < 12; ++i) tgt[i] = s[i];
      quad_step(tgt, a, *eval, t);
    }
    return quad_learnt_fit_sample(s, a, tgt, m.c, t, m.rows, lam, z, hd);
  }

#if defined(__HIPCC__)
  typedef QuadFitArgs Args;
  static constexpr int UNROLL = 2;
  typedef __attribute__((address_space(4))) const float *cfloat_ptr;
  typedef QuadFitModel<cfloat_ptr> Model;

  static __device__ __forceinline__ Model model(const Args &A) {
    return Model{A.c, (cfloat_ptr)A.ws};
  }
  static __device__ __forceinline__ void unit_row(const Args &A, const Model &, int lane,
                                                  float (&w)[RES_ROW]) {
#pragma unroll
    for (int j = 0; j < kQuadResRow; ++j) w[j] = A.ws[lane * kQuadResRow + j];
  }
#endif
};

}  // namespace
}  // namespace apg
