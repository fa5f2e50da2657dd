// wing_mpc_math.h - single-shooting MPC for ONE fixed-wing trajectory by
// projected heavy-ball descent, shared by the kernels of wing_mpc.hip (one
// trajectory per lane) and their host twins (cpu_twins.hip).  The comparator of
// the reference's fixed-wing evaluation is MPC(..., dynamics="fixed_wing_3D")
// (scripts/evaluate_fixed_wing.py:232-243; neural_control/controllers/mpc.py:
// 135-150 _initParamsFixedWing_3D).  Kept here: the action box [0, 1], an
// action cost on the three control surfaces only (its _Q_u = diag(0, 10, 10,
// 10)), the model (wing_step), the warm start by shifting.  The method is that
// of quad_mpc_math.h and cartpole_mpc_math.h: first-order shooting with a fixed
// number of iterations.
//
// The cost is the training loss on the training reference, so that the optimum
// and a policy's loss are the same quantity:
//   J = w.pos sum_k |p_{k+1} - ref_k|^2 + w.action sum_k sum_{j=1..3} (u_kj - 1/2)^2
//       (fixed_wing_mpc_loss, neural_control/drone_loss.py:72-82)
//   ref_k = p_0 + n (12 dt) (k + 1), n = (target - p_0) / |target - p_0|
//       (WingDataset._compute_target_pos, neural_control/dataset.py:309-320)
//
// One iteration on the unknowns u[H][4]:
//   forward   wing_rollout_forward (wing_rollout_math.h) from s0: H x wing_step,
//             every pre-step state stashed, the cost J
//   reverse   wing_rollout_reverse: H x wing_step_adjoint, each recomputing its
//             step from the stashed pre-step state -> g = dJ/du
//   update    m = beta m + alpha_c g,  u = clamp(u - m, 0, 1)   (c = column:
//             alpha_thrust for column 0, alpha_surface for 1..3), inside the
//             reverse sweep: step k's adjoint is the last reader of u[k]
// m = 0 at the start of every solve, a fixed number of iterations, one more
// forward sweep for the cost of the returned u.
//
// The attitude's sin / cos is the software pair on the device as well
// (wing_step<true>, wing_rates<true>), for the reason quad_mpc_math.h gives: a
// solve runs the model (2 iters + 1) H times and carries rounding noise from
// iteration to iteration; kernel and host twin then run the same arithmetic.
//
// Kinks: the model clamps tan(alpha), tan(beta) at tan(10 deg) (atan_clamped)
// and the update projects onto the box.  Where an iterate lies within rounding
// of a kink a float32 evaluation may take the other branch and descend
// elsewhere from then on - any float32 evaluation, a plain torch one as much as
// this one.
//
// Defaults iters 10, beta 0.5, alpha_thrust = alpha_surface = 0.03, from a
// float64 sweep on the CPU (torch autograd over oracle.torch_port.WingOracle,
// 256 starts of synthetic.wing_batch, H = 10, dt = 0.05, start cost 21.44):
//   alpha 0.01   J 11.31 after 10 iterations, 10.03 after 20
//   alpha 0.03   J  9.72,  9.45
//   alpha 0.1    J  9.36,  9.29
//   (alpha_thrust, alpha_surface) = (0.3, 0.1): 9.32, 9.27; (1.0, 0.3): 10.29,
//   10.24 and 12 to 13 trajectories end above their start cost; none does for
//   alpha in [1e-3, 0.1] nor for (0.3, 0.1).
// 0.03 is a factor 3 to 10 below where the method misbehaves; with it the
// float32 restatement of the tests' 200 starts stays within 1.8e-6 of float64
// after 20 iterations (tests/test_wing_mpc_cpu.py).
#pragma once
#include "wing_flight_rule.h"
#include "wing_math.h"
#include "wing_rollout_math.h"

namespace apg {
namespace {

// Row k of u: the sweeps of wing_rollout_math.h hand k over as a loop
// variable; stated as selects over the H rows, u stays in registers whether
// the compiler unrolls those loops or not.
template <int H>
__host__ __device__ __forceinline__ void wing_mpc_row(const float (&u)[H][4], int k,
                                                      float (&a)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = u[0][j];
#pragma unroll
  for (int r = 1; r < H; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = k == r ? u[r][j] : a[j];
}

template <int H>
__host__ __device__ __forceinline__ void wing_mpc_set_row(float (&u)[H][4], int k,
                                                          const float (&a)[4]) {
#pragma unroll
  for (int r = 0; r < H; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) u[r][j] = k == r ? a[j] : u[r][j];
}

// ST(k, i): the stash of the forward sweep's pre-step states (LDS on the
// device); ref(k, rp[3]): reference row k.  o.iters iterations from u (in:
// start, out: solution); trace(i, J) is called with the cost before iteration i
// and, for i = iters, with the returned cost.  Returns that cost.
template <int H, class Ref, class Stash, class Trace>
__host__ __device__ __forceinline__ float wing_mpc_solve(const float (&s0)[12], Ref &&ref,
                                                         float (&u)[H][4],
                                                         const WingConst &model,
                                                         const ApgWingLossWeights &w,
                                                         const ApgWingMpcOptions &o,
                                                         Stash &&ST, Trace &&trace) {
  float m[H][4];
#pragma unroll
  for (int k = 0; k < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) m[k][j] = 0.f;
  const auto action = [&](int k, float (&a)[4]) { wing_mpc_row<H>(u, k, a); };
  const auto step = [&](float (&x)[12], const float (&a)[4]) { wing_step<true>(x, a, model); };
  const auto no_states = [](int, const float (&)[12]) {};
  float s[12];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int it = 0; it < o.iters; ++it) {
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = s0[i];
    trace(it, wing_rollout_forward(H, s, w.pos, w.action, action, ref, ST, step, no_states));
    float lam[12];
    wing_rollout_reverse(
        H, s, lam, w.pos, w.action, action, ref, ST,
        [&](float (&l)[12], float (&ga)[4], const float (&pre)[12], const float (&a)[4]) {
          WingAux x;
          float sd[12];
          wing_rates<true>(pre, a, model, x, sd);
          wing_step_adjoint(l, ga, pre, x, sd, model);
        },
        [&](int k, const float (&ga)[4]) {
          float mk[4], uk[4];
          wing_mpc_row<H>(m, k, mk);
          wing_mpc_row<H>(u, k, uk);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            mk[j] = o.beta * mk[j] + (j == 0 ? o.alpha_thrust : o.alpha_surface) * ga[j];
            uk[j] = fminf(fmaxf(uk[j] - mk[j], 0.f), 1.f);
          }
          wing_mpc_set_row<H>(m, k, mk);
          wing_mpc_set_row<H>(u, k, uk);
        });
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = s0[i];
  float sink = 0.f;   // the last sweep stashes nothing
  const float J = wing_rollout_forward(
      H, s, w.pos, w.action, action, ref, [&](int, int) -> float & { return sink; }, step,
      no_states);
  trace(o.iters, J);
  return J;
}

// warm start of the next control step: rows move up, the last one is repeated
template <int H>
__host__ __device__ __forceinline__ void wing_mpc_shift(float (&u)[H][4]) {
#pragma unroll
  for (int k = 0; k + 1 < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) u[k][j] = u[k + 1][j];
}

// the start of a cold solve: a quarter of the thrust, neutral surfaces
template <int H>
__host__ __device__ __forceinline__ void wing_mpc_cold_start(float (&u)[H][4]) {
#pragma unroll
  for (int k = 0; k < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) u[k][j] = j == 0 ? 0.25f : 0.5f;
}

// The log of one flight of a [..][B] batch: a NULL output drops its writes
struct WingMpcFlightLog {
  float *div_linear, *div_pass, *div_fail;   // [T][B]
  float *drone, *seen, *cost;                // [T][16][B], [T][15][B], [T][B]
  size_t B, b;
  __host__ __device__ __forceinline__ void put(float *out, int row, int N, int i,
                                               float v) const {
    if (out) out[((size_t)row * N + i) * B + b] = v;
  }
};

// One closed-loop flight (wing_flight_rule.h) with the controller "shift the
// warm start, build the reference rows from the state the controller sees and
// the current target, solve on `model`, apply u[0]" (first step: from the cold
// start; the warm start is kept through a reset).  target(ti, tg[3]): the
// flight's target ti; plant(s, a): the environment's step; go_on(alive): false
// ends the loop - the wave's vote on the device, the flight's own flag on the
// host.  Returns len(drone_traj).
template <int H, class Start, class Target, class Plant, class Stash, class GoOn>
__host__ __device__ __forceinline__ int wing_mpc_flight(
    bool given, Start &&start, Target &&target, Plant &&plant, const WingConst &model,
    const ApgWingLossWeights &w, const ApgWingMpcOptions &o, const WingFlightRule &rule,
    const WingMpcFlightLog &log, Stash &&ST, GoOn &&go_on, bool live) {
  WingFlightBook f;
  wing_flight_start(f, given, start, live);
  float u[H][4];
  wing_mpc_cold_start<H>(u);
  const float vec_len = 12.f * model.dt;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int k = 0; k < rule.T; ++k) {
    float tg[3];
    target(f.ti, tg);
    if (f.alive) {
#pragma unroll
      for (int i = 0; i < 12; ++i) log.put(log.seen, k, 15, i, f.obs[i]);
#pragma unroll
      for (int j = 0; j < 3; ++j) log.put(log.seen, k, 15, 12 + j, tg[j]);
    }
    if (k > 0) wing_mpc_shift<H>(u);
    // WingDataset._compute_target_pos from the state the controller sees (no
    // contraction into fma, here and in the rows below: the rows are then the
    // ones functional.wing_mpc_reference builds from the same state, bit for
    // bit, and MPC.predict_actions repeats this loop's solves)
    float p0[3], nv[3];
    {
#pragma clang fp contract(off)
      const float rel[3] = {tg[0] - f.obs[0], tg[1] - f.obs[1], tg[2] - f.obs[2]};
      const float nrm = sqrtf(rel[0] * rel[0] + rel[1] * rel[1] + rel[2] * rel[2]);
#pragma unroll
      for (int j = 0; j < 3; ++j) p0[j] = f.obs[j], nv[j] = rel[j] / nrm * vec_len;
    }
    const float J = wing_mpc_solve<H>(
        f.obs,
        [&](int r, float (&rp)[3]) {
#pragma clang fp contract(off)
#pragma unroll
          for (int j = 0; j < 3; ++j) rp[j] = p0[j] + nv[j] * (float)(r + 1);
        },
        u, model, w, o, ST, [](int, float) {});
    const float act[4] = {u[0][0], u[0][1], u[0][2], u[0][3]};
    plant(f.s, act);
    const bool rec = f.alive;
    if (rec) {
#pragma unroll
      for (int i = 0; i < 12; ++i) log.put(log.drone, k, 16, i, f.s[i]);
#pragma unroll
      for (int j = 0; j < 4; ++j) log.put(log.drone, k, 16, 12 + j, act[j]);
    }
    const WingFlightStep st = wing_flight_book(rule, f, k, tg);
    if (rec) {
      log.put(log.cost, k, 1, 0, J);
      log.put(log.div_linear, k, 1, 0, st.div);
      log.put(log.div_pass, k, 1, 0, st.d_pass);
      log.put(log.div_fail, k, 1, 0, st.d_fail);
    }
    if (!go_on(f.alive)) break;
  }
  return f.steps;
}

// argument rules shared by the device entry points and the twins; NULL: fine
inline const char *wing_mpc_check(const ApgWingParams *model, const ApgWingLossWeights *weights,
                                  const ApgWingMpcOptions *o, int B, int H) {
  if (B < 0) return "B must be >= 0";
  if (!model || !weights) return "model / weights is NULL";
  if (!o) return "options is NULL";
  if (o->iters < 0 || o->iters > 100000) return "iters must be in [0, 100000]";
  if (!(o->beta >= 0.f && o->beta < 1.f)) return "beta must be in [0, 1)";
  if (!(o->alpha_thrust > 0.f) || !(o->alpha_surface > 0.f))
    return "alpha_thrust / alpha_surface must be positive";
  if (H != 10) return "H must be 10";
  return nullptr;
}

// the closed loop's plant and flight (wing_flight_check, and this loop's own
// rule: at least one step); NULL: fine, and `rule` is filled in
inline const char *wing_mpc_check_flight(const ApgWingParams *plant, const ApgWingFlight *f,
                                         int B, WingFlightRule *rule) {
  if (!plant) return "plant is NULL";
  if (const char *e = wing_flight_check(f, B, rule)) return e;
  if (f->max_steps < 1) return "max_steps must be >= 1";
  return nullptr;
}

}  // namespace
}  // namespace apg
