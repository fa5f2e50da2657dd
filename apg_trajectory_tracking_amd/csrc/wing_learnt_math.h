// wing_learnt_math.h - per-lane arithmetic of LearntFixedWingDynamics.forward
// (reference: neural_control/dynamics/fixed_wing_dynamics.py:270-326):
//   s' = simulate_fixed_wing(s, a) + W2 relu(W1 [s; a] + b1) + b2
// The physics is wing_rates / wing_step_adjoint of wing_math.h on the table of
// a general 3x3 inertia matrix (WingGeneralConst), unchanged; this header adds
// the table built from the module's live tensors, the 16 -> 64 -> 12 residual
// network on the PRE-step state and the raw action, and the step's adjoint
// down to dL/dstate and dL/daction (the simulator is frozen where this is
// used: NoWingParamGrads).  Called per lane by wing_learnt.hip's fused rollout
// and per trajectory by its host twin (csrc/cpu_twins.hip).
#pragma once
#include "residual_fit.h"
#include "wing_math.h"

namespace apg {
namespace {

// The residual as packed unit rows: row m = [W1[m][0..15] | W2[0..11][m] |
// b1[m] | 0 0 0] (32 floats, one 128-byte line per hidden unit), b2 behind
// the 64 rows.  A unit's weights are wave-uniform and contiguous: on the
// device they arrive as scalar operands (two 64-byte scalar loads per unit).
constexpr int kWingResHidden = 64, kWingResRow = 32;
constexpr int kWingResW2 = 16, kWingResB1 = 28;
constexpr int kWingResB2 = kWingResHidden * kWingResRow;   // 2048
constexpr int kWingResFloats = kWingResB2 + 16;            // b2[12], padded
// The packed model the rollout reads: [table | rows | b2]
constexpr int kWingLearntTableFloats = 128;
constexpr int kWingLearntPackFloats = kWingLearntTableFloats + kWingResFloats;
static_assert(sizeof(WingGeneralConst) <= kWingLearntTableFloats * sizeof(float),
              "the step table outgrew its slot");

// make_general_const's content (wing_math.h) from the module's tensors, callable
// on the device: theta = the 41 entries of ApgWingParams (the I_* slots are not
// read - the general table takes the inertia from the matrix), inertia = the
// 3x3 parameter row-major.  Same folding as make_const: the double-precision
// products with c and b, 1 / mass, g mass, the 3x3 inverse in double.  A
// singular matrix gives a non-finite table.
__host__ __device__ inline WingGeneralConst wing_learnt_table(const float *theta,
                                                              const float *inertia,
                                                              float dt) {
  ApgWingParams p;
  float *f = reinterpret_cast<float *>(&p);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(ApgWingParams) / sizeof(float)); ++i) f[i] = theta[i];
  WingGeneralConst k;
  k.dt = dt;
  k.half_rho = (float)(0.5 * (double)p.rho);
  k.S = p.S, k.c = p.c, k.b = p.b;
  k.inv_mass = (float)(1.0 / (double)p.mass);
  k.g_m = (float)((double)p.g * (double)p.mass);
#if defined(__HIP_DEVICE_COMPILE__)
  sincos_fast(p.epsilon, &k.sin_eps, &k.cos_eps);   // (no libm tables on the device)
#else
  k.cos_eps = cosf(p.epsilon), k.sin_eps = sinf(p.epsilon);
#endif
  k.alpha_bound = (float)(10.0 / 180.0 * 3.14159265358979323846);
  const double c = p.c, b = p.b;
  k.CL0 = p.CL0, k.CL_a = p.CL_alpha, k.CL_qc = (float)(p.CL_q * c), k.CL_de = p.CL_del_e;
  k.CD0 = p.CD0, k.CD_a = p.CD_alpha, k.CD_qc = (float)(p.CD_q * c), k.CD_de = p.CD_del_e;
  k.CY0 = p.CY0, k.CY_b = p.CY_beta, k.CY_pb = (float)(p.CY_p * b);
  k.CY_rb = (float)(p.CY_r * b), k.CY_da = p.CY_del_a, k.CY_dr = p.CY_del_r;
  k.Cl0 = p.Cl0, k.Cl_b = p.Cl_beta, k.Cl_pb = (float)(p.Cl_p * b);
  k.Cl_rb = (float)(p.Cl_r * b), k.Cl_da = p.Cl_del_a, k.Cl_dr = p.Cl_del_r;
  k.Cm0 = p.Cm0, k.Cm_a = p.Cm_alpha, k.Cm_qc = (float)(p.Cm_q * c), k.Cm_de = p.Cm_del_e;
  k.Cn0 = p.Cn0, k.Cn_b = p.Cn_beta, k.Cn_pb = (float)(p.Cn_p * b);
  k.Cn_rb = (float)(p.Cn_r * b), k.Cn_da = p.Cn_del_a, k.Cn_dr = p.Cn_del_r;
  // the sparse-inertia fields are not read through a general table
  k.Ixx = k.Iyy = k.Izz = k.a13 = 0.f;
  k.i00 = k.i02 = k.i11 = k.i22 = 0.f;
  const double m00 = inertia[0], m01 = inertia[1], m02 = inertia[2], m10 = inertia[3],
               m11 = inertia[4], m12 = inertia[5], m20 = inertia[6], m21 = inertia[7],
               m22 = inertia[8];
  const double det = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) +
                     m02 * (m10 * m21 - m11 * m20);
  k.I[0][0] = (float)m00, k.I[0][1] = (float)m01, k.I[0][2] = (float)m02;
  k.I[1][0] = (float)m10, k.I[1][1] = (float)m11, k.I[1][2] = (float)m12;
  k.I[2][0] = (float)m20, k.I[2][1] = (float)m21, k.I[2][2] = (float)m22;
  k.Iinv[0][0] = (float)((m11 * m22 - m12 * m21) / det);   // adjugate / det
  k.Iinv[0][1] = (float)((m02 * m21 - m01 * m22) / det);
  k.Iinv[0][2] = (float)((m01 * m12 - m02 * m11) / det);
  k.Iinv[1][0] = (float)((m12 * m20 - m10 * m22) / det);
  k.Iinv[1][1] = (float)((m00 * m22 - m02 * m20) / det);
  k.Iinv[1][2] = (float)((m02 * m10 - m00 * m12) / det);
  k.Iinv[2][0] = (float)((m10 * m21 - m11 * m20) / det);
  k.Iinv[2][1] = (float)((m01 * m20 - m00 * m21) / det);
  k.Iinv[2][2] = (float)((m00 * m11 - m01 * m10) / det);
  return k;
}

// element t of the packed residual (t < kWingResFloats)
__host__ __device__ __forceinline__ float wing_residual_packed(int t, const float *w1,
                                                               const float *b1,
                                                               const float *w2,
                                                               const float *b2) {
  if (t >= kWingResB2) return t - kWingResB2 < 12 ? b2[t - kWingResB2] : 0.f;
  const int m = t / kWingResRow, j = t - m * kWingResRow;
  if (j < kWingResW2) return w1[m * 16 + j];
  if (j < kWingResB1) return w2[(j - kWingResW2) * kWingResHidden + m];
  return j == kWingResB1 ? b1[m] : 0.f;
}

// The table seen through the constant address space (the device reads it with
// scalar loads where it is used); it carries the full inertia matrix like the
// plain type.
typedef __attribute__((address_space(4))) const WingGeneralConst WingGeneralConstK;
template <>
struct wing_general_inertia<WingGeneralConstK> : std::true_type {};

// out += W2 relu(W1 z + b1) + b2, z = [state; action]; P: pointer to the packed
// rows (host: const float *, device: the constant address space)
template <typename P>
__host__ __device__ __forceinline__ void wing_residual_add(float (&out)[12],
                                                           const float (&z)[16], P rows) {
#pragma unroll 2
  for (int m = 0; m < kWingResHidden; ++m) {
    P w = rows + m * kWingResRow;
    float h = w[kWingResB1];
#pragma unroll
    for (int j = 0; j < 16; ++j) h = fmaf(w[j], z[j], h);
    h = fmaxf(h, 0.f);
#pragma unroll
    for (int o = 0; o < 12; ++o) out[o] = fmaf(w[kWingResW2 + o], h, out[o]);
  }
#pragma unroll
  for (int o = 0; o < 12; ++o) out[o] += rows[kWingResB2 + o];
}

// dz = dL/dz of the residual for dL/dr = lam, the hidden layer recomputed unit
// by unit (relu'(0) = 0, as torch's threshold backward)
template <typename P>
__host__ __device__ __forceinline__ void wing_residual_adjoint(const float (&lam)[12],
                                                               const float (&z)[16], P rows,
                                                               float (&dz)[16]) {
#pragma unroll
  for (int j = 0; j < 16; ++j) dz[j] = 0.f;
#pragma unroll 2
  for (int m = 0; m < kWingResHidden; ++m) {
    P w = rows + m * kWingResRow;
    float h = w[kWingResB1];
#pragma unroll
    for (int j = 0; j < 16; ++j) h = fmaf(w[j], z[j], h);
    float dh = 0.f;
#pragma unroll
    for (int o = 0; o < 12; ++o) dh = fmaf(w[kWingResW2 + o], lam[o], dh);
    dh = h > 0.f ? dh : 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) dz[j] = fmaf(w[j], dh, dz[j]);
  }
}

// s <- LearntFixedWingDynamics.forward(s, a)
template <typename KT, typename P>
__host__ __device__ __forceinline__ void wing_learnt_step(float (&s)[12], const float (&a)[4],
                                                          KT &k, P rows) {
  float z[16], r[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) z[i] = s[i], r[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) z[12 + i] = a[i];
  wing_residual_add(r, z, rows);
  wing_step(s, a, k);
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] += r[i];
}

// lam: dL/dnext on entry -> dL/dstate on exit; ga += dL/daction.  `pre`, `a`:
// the PRE-step state and the action.
template <typename KT, typename P>
__host__ __device__ __forceinline__ void wing_learnt_step_adjoint(float (&lam)[12],
                                                                  float (&ga)[4],
                                                                  const float (&pre)[12],
                                                                  const float (&a)[4], KT &k,
                                                                  P rows) {
  float z[16], dz[16], sd[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) z[i] = pre[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) z[12 + i] = a[i];
  wing_residual_adjoint(lam, z, rows, dz);
  WingAux x;
  wing_rates(pre, a, k, x, sd);
  NoWingParamGrads none;
  wing_step_adjoint(lam, ga, pre, x, sd, k, none);
#pragma unroll
  for (int i = 0; i < 12; ++i) lam[i] += dz[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) ga[i] += dz[12 + i];
}

// ------------------------------------------------- the simulator fit's step --
// TrainBase.train_dynamics_model (scripts/train_base.py:160-186) on this
// module: loss = sum (forward(s, a) - target)^2 and the cotangent of EVERY
// parameter.  The flat gradient (apg.h: APG_WING_FIT_*): the 41 + 9 physical
// cotangents in apg_wing_learnt_step_bwd's layout, then dW1 [64][16], db1
// [64], dW2 [12][64], db2 [12].
constexpr int kWingFitGW1 = kWingParamGrads;                        // 50
constexpr int kWingFitGB1 = kWingFitGW1 + kWingResHidden * 16;      // 1074
constexpr int kWingFitGW2 = kWingFitGB1 + kWingResHidden;           // 1138
constexpr int kWingFitGB2 = kWingFitGW2 + 12 * kWingResHidden;      // 1906
constexpr int kWingFitGrads = kWingFitGB2 + 12;                     // 1918
// A partial row as the kernel sums it: [50 physical | db2 (12) | 0 0 | 29
// planes of 64: plane j < 16 = dW1[.][j], plane 16 + o = dW2[o][.], plane 28 =
// db1] - hidden unit m owns element m of every plane.
constexpr int kWingFitUnit = kResFitUnit;                           // a unit's cotangents
constexpr int kWingFitHead = 64;
constexpr int kWingFitRow = kWingFitHead + kWingFitUnit * kWingResHidden;   // 1920

// element c of a partial row -> its place in the flat gradient (-1: padding)
__host__ __device__ __forceinline__ int wing_fit_dest(int c) {
  if (c < kWingParamGrads) return c;
  if (c < kWingParamGrads + 12) return kWingFitGB2 + (c - kWingParamGrads);
  if (c < kWingFitHead) return -1;
  const int j = (c - kWingFitHead) / kWingResHidden, m = (c - kWingFitHead) % kWingResHidden;
  if (j < 16) return kWingFitGW1 + m * 16 + j;
  if (j < 28) return kWingFitGW2 + (j - 16) * kWingResHidden + m;
  return kWingFitGB1 + m;
}

// One sample of the fit: pred = forward(s, a) on the live table and rows,
// returns sum (pred - tgt)^2; lam = 2 (pred - tgt) (the seed of the reverse
// sweep, which the residual's cotangents need as it stands); pg += the
// physical cotangents.  dL/dstate and dL/daction are not produced.
template <typename KT, typename P>
__host__ __device__ __forceinline__ float wing_learnt_fit_sample(const float (&s)[12],
                                                                 const float (&a)[4],
                                                                 const float (&tgt)[12],
                                                                 KT &k, P rows,
                                                                 float (&lam)[12],
                                                                 WingParamGrads &pg) {
  float z[16], r[12], sd[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) z[i] = s[i], r[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) z[12 + i] = a[i];
  wing_residual_add(r, z, rows);
  WingAux x;
  wing_rates(s, a, k, x, sd);
  float loss = 0.f, lp[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const float d = ((s[i] + k.dt * sd[i]) + r[i]) - tgt[i];   // wing_learnt_step's sum
    loss = fmaf(d, d, loss);
    lam[i] = lp[i] = 2.f * d;
  }
  float ga[4] = {0.f, 0.f, 0.f, 0.f};
  wing_step_adjoint(lp, ga, s, x, sd, k, pg);
  return loss;
}

// What residual_fit.h's shared fit reads of this system.  The model: the step
// table and the packed rows (device: both in the constant address space, from
// the pack in the workspace; host: plain).
template <class KT, class P>
struct WingFitModel {
  KT *k;
  P rows;
};

#if defined(__HIPCC__)
// the fit kernel's arguments (residual_fit.h fills the common ones)
struct WingFitArgs {
  const float *state, *action, *target;   // target NULL: the analytic step on `eval`
  const float *ws;                        // the pack
  float *loss_partials, *rows;
  WingConst eval;
  int B;
};
#endif

struct WingFit {
  static constexpr int S = 12, A = 4, IN = 16, OUT = 12;
  static constexpr int RES_ROW = kWingResRow, RW2 = kWingResW2, RB1 = kWingResB1;
  static constexpr int UNIT = kWingFitUnit, UW2 = 16, UB1 = 28;
  static constexpr int HEAD = kWingFitHead, USED = kWingParamGrads + 12, ROW = kWingFitRow;
  static constexpr int GRADS = kWingFitGrads;
  static constexpr bool REG = true;
  static constexpr int G_W1 = kWingFitGW1, G_B1 = kWingFitGB1, G_W2 = kWingFitGW2,
                       G_B2 = kWingFitGB2;
  static constexpr int NORMS_AT = kWingLearntPackFloats, ROWS_AT = NORMS_AT + 16;
  typedef WingConst Eval;
  typedef FitNoScale Scale;

  static __host__ __device__ __forceinline__ int dest(int c) { return wing_fit_dest(c); }
  static __host__ __device__ __forceinline__ float value(int, float v, const Scale &) {
    return v;
  }

  // the head: the 50 physical cotangents, then db2 = lam
  template <class M>
  static __host__ __device__ __forceinline__ float sample(const M &m, const float (&s)[12],
                                                          const float (&a)[4], float (&tgt)[12],
                                                          const WingConst *eval,
                                                          float (&lam)[12], float (&z)[16],
                                                          float (&hd)[USED]) {
    if (eval) {
#pragma unroll
      for (int i = 0; i < 12; ++i) tgt[i] = s[i];
      wing_step(tgt, a, *eval);
    }
    WingParamGrads pg;
#pragma unroll
    for (int i = 0; i < kWingParamGrads; ++i) pg.v[i] = 0.f;
    const float loss = wing_learnt_fit_sample(s, a, tgt, *m.k, m.rows, lam, pg);
#pragma unroll
    for (int i = 0; i < 12; ++i) z[i] = s[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) z[12 + i] = a[i];
#pragma unroll
    for (int i = 0; i < kWingParamGrads; ++i) hd[i] = pg.v[i];
#pragma unroll
    for (int o = 0; o < 12; ++o) hd[kWingParamGrads + o] = lam[o];
    return loss;
  }

#if defined(__HIPCC__)
  typedef WingFitArgs Args;
  static constexpr int UNROLL = 2;
  typedef __attribute__((address_space(4))) const float *cfloat_ptr;
  typedef WingFitModel<WingGeneralConstK, cfloat_ptr> Model;

  static __device__ __forceinline__ Model model(const Args &A) {
    return Model{(WingGeneralConstK *)A.ws, (cfloat_ptr)(A.ws + kWingLearntTableFloats)};
  }
  // (vector loads: one 128-byte line per lane)
  static __device__ __forceinline__ void unit_row(const Args &A, const Model &, int lane,
                                                  float (&w)[RES_ROW]) {
    const float4 *src =
        reinterpret_cast<const float4 *>(A.ws + kWingLearntTableFloats + lane * kWingResRow);
#pragma unroll
    for (int q = 0; q < kWingResRow / 4; ++q) {
      const float4 v = src[q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
  }
#endif
};

}  // namespace
}  // namespace apg
