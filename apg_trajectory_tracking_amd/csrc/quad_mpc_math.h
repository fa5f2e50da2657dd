// quad_mpc_math.h - single-shooting MPC for ONE quadrotor trajectory by
// projected heavy-ball descent, shared by the kernels of quad_mpc.hip (one
// trajectory per lane, everything in registers) and their host twins
// (cpu_twins.hip).  The comparator the reference judges its controllers
// against is neural_control/controllers/mpc.py (CasADi + IPOPT, multiple
// shooting); kept here: the stage cost (quad_mpc_loss = that cost / 10), the
// action box [0, 1], the model (quad_step), the warm start by shifting.  The
// method differs and is named as such: first-order shooting with a fixed number
// of iterations, so that every lane does the same work and the result is a
// deterministic function of its inputs.
//
// One iteration on the unknowns u[H][4]:
//   forward   H x quad_step from state0, cost J = quad_mpc_loss of the H states
//             (all H rows: position, velocity, body rates, action terms - the
//             arithmetic of the fused rollout's loss)
//   reverse   H x quad_step_adjoint with the loss seeds -> g = dJ/du
//   update    m = beta m + alpha_c g,  u = clamp(u - m, 0, 1)   (c = column:
//             alpha_thrust for column 0, alpha_rate for 1..3), inside the
//             reverse sweep: step k's adjoint is the last reader of u[k]
// m = 0 at the start of every solve.  After the last update one more forward
// sweep gives the cost that belongs to the returned u.
// The solver is generic over the MODEL (below): quad_step here (MpcAnalytic),
// the learnt simulator in quad_learnt_mpc_math.h.
#pragma once
#include "quad_flight_rule.h"
#include "quad_math.h"

namespace apg {
namespace {

// The solver's sin / cos is the software pair (1.6 ulp) on the device as well,
// not make_trig's hardware pair (absolute error 1.5e-7): a solve runs the model
// (2 iters + 1) H times and, where the fixed step sits close to the stability
// limit of a trajectory's curvature, carries rounding noise from iteration to
// iteration with a gain above one (measured over 65 543 windows, 20 iterations:
// the worst trajectory's u ends 500 x the median error away from float64).
// With the hardware pair that trajectory missed the 1e-4 parity bar (1.2e-4;
// float32 torch 7.7e-5); the median error was 2.4 x float32's, with this pair
// it is float32's.  Kernel and host twin then run the same arithmetic.
__host__ __device__ __forceinline__ Trig mpc_trig(const float att[3]) {
  Trig t;
  sincos_fast(att[0], &t.sr, &t.cr);
  sincos_fast(att[1], &t.sp, &t.cp);
  sincos_fast(att[2], &t.sy, &t.cy);
  return t;
}

// A MODEL is what one step of the horizon and its adjoint are.  The solver asks
// of it:
//   Stash<H>                         what its adjoint keeps of the forward sweep
//   step<STASH>(k, s, u, st)         s <- f(s, u), row k of the stash filled
//   adjoint(k, lam, ga, u, w, st)    lam <- (df/ds)^T lam, ga += (df/du)^T lam;
//                                    u: the step's action, w: the body rates
//                                    before it
// The cost is the solver's, on the states the model returns and on u itself.
//
// The analytic model: FlightmareDynamics' step on the constants `c`; of the
// forward sweep it keeps the sin / cos of the attitude before every step.
struct MpcAnalytic {
  const QuadConst &c;
  template <int H>
  struct Stash {
    Trig trig[H];
  };
  template <bool STASH, int H>
  __host__ __device__ __forceinline__ void step(int k, float (&s)[12], const float (&u)[4],
                                                Stash<H> &st) const {
    const Trig t = mpc_trig(&s[3]);
    if (STASH) st.trig[k] = t;
    quad_step(s, u, c, t);
  }
  template <int H>
  __host__ __device__ __forceinline__ void adjoint(int k, float (&lam)[12], float (&ga)[4],
                                                   const float (&u)[4], const float w[3],
                                                   const Stash<H> &st) const {
    quad_step_adjoint(lam, ga, u[0], w, c, st.trig[k]);
  }
};

// what the reverse sweep needs of the forward one: the model's own stash, the
// body rates before and after every step, and the position / velocity
// residuals of the loss
template <int H, class Model>
struct MpcStash {
  typename Model::template Stash<H> model;
  float w[H + 1][3];
  float dp[H][3], dv[H][3];
};

// ref[k] = (position, velocity) of window row k.  Returns J.
template <int H, bool STASH, class Model>
__host__ __device__ __forceinline__ float mpc_forward(const float (&s0)[12],
                                                      const float (&ref)[H][6],
                                                      const float (&u)[H][4],
                                                      const Model &model,
                                                      const ApgQuadLossWeights &w,
                                                      MpcStash<H, Model> &st) {
  float s[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = s0[i];
  float J = 0.f;
#pragma unroll
  for (int k = 0; k < H; ++k) {
    if (STASH) {
#pragma unroll
      for (int i = 0; i < 3; ++i) st.w[k][i] = s[9 + i];
    }
    model.template step<STASH>(k, s, u[k], st.model);
    float lp = 0.f, lv = 0.f, lw = 0.f, lr = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float dp = s[i] - ref[k][i], dv = s[6 + i] - ref[k][3 + i];
      lp += dp * dp, lv += dv * dv, lw += s[9 + i] * s[9 + i];
      const float d = u[k][1 + i] - 0.5f;
      lr += d * d;
      if (STASH) st.dp[k][i] = dp, st.dv[k][i] = dv;
    }
    const float da0 = u[k][0] - 0.5f;
    J += w.pos * lp + w.vel * lv + w.av * lw + w.rates * lr + w.thrust * da0 * da0;
  }
  if (STASH) {
#pragma unroll
    for (int i = 0; i < 3; ++i) st.w[H][i] = s[9 + i];
  }
  return J;
}

// reverse sweep + update of u and m
template <int H, class Model>
__host__ __device__ __forceinline__ void mpc_reverse_update(const MpcStash<H, Model> &st,
                                                            float (&u)[H][4],
                                                            float (&m)[H][4],
                                                            const Model &model,
                                                            const ApgQuadLossWeights &w,
                                                            const ApgQuadMpcOptions &o) {
  float lam[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) lam[i] = 0.f;
#pragma unroll
  for (int k = H - 1; k >= 0; --k) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      lam[i] += 2.f * w.pos * st.dp[k][i];
      lam[6 + i] += 2.f * w.vel * st.dv[k][i];
      lam[9 + i] += 2.f * w.av * st.w[k + 1][i];
    }
    float ga[4];
    ga[0] = 2.f * w.thrust * (u[k][0] - 0.5f);
#pragma unroll
    for (int j = 1; j < 4; ++j) ga[j] = 2.f * w.rates * (u[k][j] - 0.5f);
    model.adjoint(k, lam, ga, u[k], st.w[k], st.model);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      m[k][j] = o.beta * m[k][j] + (j == 0 ? o.alpha_thrust : o.alpha_rate) * ga[j];
      u[k][j] = fminf(fmaxf(u[k][j] - m[k][j], 0.f), 1.f);
    }
  }
}

// o.iters iterations from u (in: start, out: solution); trace(i, J) is called
// with the cost before iteration i and, for i = iters, with the returned cost
template <int H, class Model, class Trace>
__host__ __device__ __forceinline__ float mpc_solve(const float (&s0)[12],
                                                    const float (&ref)[H][6],
                                                    float (&u)[H][4], const Model &model,
                                                    const ApgQuadLossWeights &w,
                                                    const ApgQuadMpcOptions &o,
                                                    Trace &&trace) {
  float m[H][4];
#pragma unroll
  for (int k = 0; k < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) m[k][j] = 0.f;
  MpcStash<H, Model> st;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int it = 0; it < o.iters; ++it) {
    trace(it, mpc_forward<H, true>(s0, ref, u, model, w, st));
    mpc_reverse_update<H>(st, u, m, model, w, o);
  }
  const float J = mpc_forward<H, false>(s0, ref, u, model, w, st);
  trace(o.iters, J);
  return J;
}

// warm start of the next control step: rows move up, the last one is repeated
template <int H>
__host__ __device__ __forceinline__ void mpc_shift(float (&u)[H][4]) {
#pragma unroll
  for (int k = 0; k + 1 < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) u[k][j] = u[k + 1][j];
}

// The log of one flight of a [..][B] batch: a NULL output drops its writes
struct MpcFlightLog {
  float *div, *drone, *actions, *start, *cost;   // ApgQuadFlight's, cost [T][B]
  size_t B, b;
  template <int N>
  __host__ __device__ __forceinline__ void put(float *out, int row, const float (&v)[N]) const {
    if (!out) return;
#pragma unroll
    for (int i = 0; i < N; ++i) out[((size_t)row * N + i) * B + b] = v[i];
  }
};

// One closed-loop flight (quad_flight_rule.h) with the controller "shift the warm
// start, solve on the model `model`, apply u[0]" (first step: from u = 0.5; the
// warm start is kept through a reset).  row(r, col): the flight's reference;
// plant(s, u0): the environment's step.  Returns the iterations executed.
template <class Row, class Plant, class Model>
__host__ __device__ __forceinline__ int mpc_flight(Row &&row, Plant &&plant, const Model &model,
                                                   const ApgQuadLossWeights &w,
                                                   const ApgQuadMpcOptions &o,
                                                   const QuadFlightRule &rule,
                                                   const MpcFlightLog &log) {
  constexpr int H = kFlightH;
  float s[12], win[H][6], u[H][4];
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = i < 3 ? row(0, i) : 0.f;  // zero_reset
  const auto window_row = [&](int r, float (&x)[6]) {   // (position, velocity)
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = row(r, i), x[3 + i] = row(r, 6 + i);
  };
#pragma unroll
  for (int r = 0; r < H; ++r) window_row(1 + r, win[r]);
#pragma unroll
  for (int k = 0; k < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) u[k][j] = 0.5f;
  log.put(log.drone, 0, s);
  int steps = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int k = 0; k < rule.T; ++k) {
    log.put(log.start, k, s);
    if (k > 0) mpc_shift<H>(u);
    const float J[1] = {mpc_solve<H>(s, win, u, model, w, o, [](int, float) {})};
    log.put(log.cost, k, J);
    log.put(log.actions, k, u[0]);
    plant(s, u[0]);
    // window row 0 is reference[cur] after get_ref_traj: project_on_ref
    const float ref[3] = {win[0][0], win[0][1], win[0][2]};
    const float dv[1] = {flight_divergence(ref, s)};
    log.put(log.drone, k + 1, s);
    log.put(log.div, k, dv);
    steps = k + 1;
    if (rule.failed(s, dv[0])) {
      if (rule.test_time) break;
      const int cur = rule.reset_row(k);   // get_current_full_state: zero rates
#pragma unroll
      for (int i = 0; i < 12; ++i) s[i] = i < 9 ? row(cur, i) : 0.f;
    }
    if (rule.window_advances(k)) {
#pragma unroll
      for (int r = 0; r + 1 < H; ++r)
#pragma unroll
        for (int i = 0; i < 6; ++i) win[r][i] = win[r + 1][i];
      window_row(k + 1 + H, win[H - 1]);
    }
  }
  return steps;
}

// argument rules shared by the device entry points and the twins; NULL: fine
inline const char *mpc_check_options(const ApgQuadMpcOptions *o) {
  if (!o) return "options is NULL";
  if (o->iters < 0 || o->iters > 100000) return "iters must be in [0, 100000]";
  if (!(o->beta >= 0.f && o->beta < 1.f)) return "beta must be in [0, 1)";
  if (!(o->alpha_thrust > 0.f) || !(o->alpha_rate > 0.f))
    return "alpha_thrust / alpha_rate must be positive";
  return nullptr;
}

}  // namespace
}  // namespace apg
