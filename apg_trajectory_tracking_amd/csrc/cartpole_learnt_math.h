// cartpole_learnt_math.h - per-lane arithmetic of LearntCartpoleDynamics
// (reference: neural_control/dynamics/cartpole_dynamics.py:122-140 with
// learnt_dynamics.py:58-98):
//   s' = simulate_cartpole(s, a) + W2 relu(W1 [s; a] + b1)
// where simulate_cartpole (:53-119) reads six LIVE parameters: max_force_mag,
// masspole, length, friction, total_mass and polemass_length.  After training
// they are independent (total_mass is no longer masspole + masscart), so the
// step constants are built from all six (make_const of cartpole_math.h derives
// two of them).  gravity is the module constant 9.81.  The step itself is
// cart_step / cart_step_adjoint of cartpole_math.h, unchanged; this header adds
// the parameter cotangents and the residual network.  Host-callable as well
// (csrc/cpu_twins.hip).
#pragma once
#include <math.h>

#include "cartpole_math.h"
#include "residual_fit.h"

namespace apg {
namespace {

constexpr int kCartResHidden = 64;             // linear_state_1: 5 -> 64
constexpr int kCartResRow = 10;                // packed unit row, see below
constexpr int kCartResFloats = kCartResHidden * kCartResRow;   // 640
constexpr int kCartPhysGrads = 6;              // order of ApgCartpoleLearnt
// grad_params: [6 physical | W1 [64][5] | b1 [64] | W2 [4][64]]
constexpr int kCartGW1 = kCartPhysGrads, kCartGB1 = kCartGW1 + 320,
              kCartGW2 = kCartGB1 + 64, kCartLearntGrads = kCartGW2 + 256;   // 646
static_assert(kCartLearntGrads == 646, "parameter count");

// The six physical parameters, in the order of ApgCartpoleLearnt.
struct CartLearntParams {
  float F, mp, l, mu, tm, pml;
};

__host__ __device__ __forceinline__ CartConst make_learnt_const(const CartLearntParams &p,
                                                                float dt) {
  const float g = 9.81f;
  CartConst c;
  c.dt = dt;
  c.force_scale = p.F * 0.5f;
  c.mu = p.mu;
  c.pml = p.pml;
  c.mp_g3 = 3.f * p.mp * g;
  c.tm4 = 4.f * p.tm;
  c.mp3 = 3.f * p.mp;
  c.tm_g6 = 6.f * p.tm * g;
  c.l_tm4 = 4.f * p.l * p.tm;
  c.pml3 = 3.f * p.pml;
  return c;
}

// Cotangents of the six parameters for one step (added to g[0..5]); lam =
// dL/dnext (call BEFORE cart_step_adjoint overwrites it), (a, xd, thd) the
// step's action and pre-step velocities, x its aux.  With gx = dt lam[1],
// gt = dt lam[3] and Dx / Dt the two denominators:
//   dF   = (4 gx/Dx + 6 c gt/Dt) a / 2        dmu = -4 xd gx/Dx - 6 xd c gt/Dt
//   dpml = -2 thd^2 s gx/Dx + (3 c^2 thacc - 3 thd^2 s c) gt/Dt
//   dmp  = (3 g s c + 3 c^2 xacc) gx/Dx       dl  = -4 tm thacc gt/Dt
//   dtm  = -4 xacc gx/Dx + (6 g s - 4 l thacc) gt/Dt
__host__ __device__ __forceinline__ void cart_param_adjoint(const float (&lam)[4], float a,
                                                            float xd, float thd,
                                                            const CartAux &x,
                                                            const CartLearntParams &p,
                                                            float dt, float (&g)[6]) {
  const float gx = dt * lam[1] / x.den_x, gt = dt * lam[3] / x.den_t;
  const float s = x.s, c = x.co, c2 = c * c, th2 = thd * thd, grav = 9.81f;
  g[0] += (4.f * gx + 6.f * c * gt) * a * 0.5f;
  g[1] += (3.f * grav * s * c + 3.f * c2 * x.xacc) * gx;
  g[2] += -4.f * p.tm * x.thacc * gt;
  g[3] += -4.f * xd * gx - 6.f * xd * c * gt;
  g[4] += -4.f * x.xacc * gx + (6.f * grav * s - 4.f * p.l * x.thacc) * gt;
  g[5] += -2.f * th2 * s * gx + (3.f * c2 * x.thacc - 3.f * th2 * s * c) * gt;
}

// The pointer rule of ApgCartpoleLearnt, shared by the device entry points and
// the twins; NULL: fine.  need_residual: w1 / b1 / w2 are all given; otherwise
// all or none (none: the physics alone).
inline const char *cart_learnt_check(const ApgCartpoleLearnt *m, bool need_residual) {
  if (!m) return "model is NULL";
  if (!m->max_force_mag || !m->masspole || !m->length || !m->friction || !m->total_mass ||
      !m->polemass_length)
    return "a physical parameter pointer is NULL";
  const bool any = m->w1 || m->b1 || m->w2, all = m->w1 && m->b1 && m->w2;
  if (any != all || (need_residual && !all))
    return need_residual ? "w1 / b1 / w2 must be all given"
                         : "w1 / b1 / w2 must be all given or all NULL";
  return nullptr;
}

// element t of the packed residual (t < kCartResFloats): unit row t / 10, see
// below
__host__ __device__ __forceinline__ float cart_residual_packed(int t, const float *w1,
                                                               const float *b1,
                                                               const float *w2) {
  const int u = t / kCartResRow, j = t - u * kCartResRow;
  return j < 5 ? w1[u * 5 + j] : j == 5 ? b1[u] : w2[(j - 6) * kCartResHidden + u];
}

// Residual network on packed unit rows: row m = [W1[m][0..4], b1[m],
// W2[0..3][m]] (10 floats; `rows` in LDS on the device).  The units
// [m0, m1) of r = W2 relu(W1 z + b1) are added to out, z = [state; action].
__host__ __device__ __forceinline__ void cart_residual_add(float (&out)[4], const float (&z)[5],
                                                           const float *rows, int m0, int m1) {
  for (int m = m0; m < m1; ++m) {
    const float *w = rows + m * kCartResRow;
    float h = w[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) h = fmaf(w[j], z[j], h);
    h = fmaxf(h, 0.f);
#pragma unroll
    for (int o = 0; o < 4; ++o) out[o] = fmaf(w[6 + o], h, out[o]);
  }
}

// dL/dz of the residual for dL/dr = lam, the hidden layer recomputed
// (relu'(0) = 0, as torch's threshold backward).
__host__ __device__ __forceinline__ void cart_residual_adjoint(const float (&lam)[4],
                                                               const float (&z)[5],
                                                               const float *rows,
                                                               float (&dz)[5]) {
#pragma unroll
  for (int j = 0; j < 5; ++j) dz[j] = 0.f;
  for (int m = 0; m < kCartResHidden; ++m) {
    const float *w = rows + m * kCartResRow;
    float h = w[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) h = fmaf(w[j], z[j], h);
    float dh = 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o) dh = fmaf(w[6 + o], lam[o], dh);
    dh = h > 0.f ? dh : 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) dz[j] = fmaf(w[j], dh, dz[j]);
  }
}

// Weight cotangents of ONE unit row for one sample (added to gw[0..9] in the
// row's own order: dW1[m][0..4], db1[m], dW2[0..3][m]): residual_fit.h
__host__ __device__ __forceinline__ void cart_residual_unit_grads(const float *w,
                                                                  const float (&z)[5],
                                                                  const float (&lam)[4],
                                                                  float (&gw)[10]) {
  residual_unit_grads<5, 4, 6, 5, 6, 5>(w, z, lam, gw);
}

// One learnt step in place: physics on the live parameters, then the residual
// (all 64 units) on the PRE-step state and the raw action.  rows NULL: physics
// only (simulate_cartpole).  WRAP = false: the physics' angle is advanced
// without the atan2 wrap (cart_step<false>: the planning model of
// cartpole_mpc_math.h); the residual is added to it all the same.
template <bool WRAP = true>
__host__ __device__ __forceinline__ CartAux cart_learnt_step(float (&s)[4], float a,
                                                             const CartConst &c,
                                                             const float *rows) {
  const float z[5] = {s[0], s[1], s[2], s[3], a};
  const CartAux x = cart_step<WRAP>(s, a, c);
  if (rows) {
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    cart_residual_add(r, z, rows, 0, kCartResHidden);
#pragma unroll
    for (int o = 0; o < 4; ++o) s[o] += r[o];
  }
  return x;
}

// lam: dL/dnext on entry, dL/dstate on exit; returns dL/daction.  `pre` = the
// pre-step state, x = its aux.  Physics adjoint plus the residual's (rows NULL:
// physics only).
__host__ __device__ __forceinline__ float cart_learnt_step_adjoint(float (&lam)[4],
                                                                   const float (&pre)[4],
                                                                   float a, const CartAux &x,
                                                                   const CartConst &c,
                                                                   const float *rows) {
  float dz[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (rows) {
    const float z[5] = {pre[0], pre[1], pre[2], pre[3], a};
    cart_residual_adjoint(lam, z, rows, dz);
  }
  float ga = cart_step_adjoint(lam, pre[1], pre[3], x, c);
#pragma unroll
  for (int i = 0; i < 4; ++i) lam[i] += dz[i];
  return ga + dz[4];
}

}  // namespace
}  // namespace apg
