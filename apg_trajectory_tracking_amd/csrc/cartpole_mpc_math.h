// cartpole_mpc_math.h - single-shooting MPC for ONE cart-pole trajectory by
// projected heavy-ball descent, shared by the kernels of cartpole_mpc.hip (one
// trajectory per lane, everything in registers) and their host twins
// (cpu_twins.hip).  The comparator of the reference's cart-pole evaluation is
// MPC(horizon=10, dt=0.05, dynamics="cartpole") (scripts/evaluate_cartpole.py:
// 399-407; neural_control/controllers/mpc.py:87-100 _initParamsCartpole).  Kept
// here: the action box [-1, 1], the start u = 0, the warm start by shifting and
// the MODEL of its CasADi twin (CartpoleDynamicsMPC.simulate_cartpole,
// cartpole_dynamics.py:239-278): cart_step's arithmetic with the angle advanced
// as theta + dt theta_dot - no atan2 wrap inside the horizon (cart_step<false>).
// With the wrapped step the cost jumps where the angle crosses +-pi and the
// gradient does not see it: of 512 swing-up starts in float64, 81-88 % ended
// ABOVE their start cost at every step size tried; with the unwrapped step 0 %.
//
// The cost is the training loss on the training reference, so that the optimum
// and a policy's loss are the same quantity:
//   J = sum_k (s_k - ref_k)^2 . [0, 3, 10, 1] + 0.01 sum_k u_k^2
//       (cartpole_loss_mpc, neural_control/drone_loss.py:136-145)
//   ref_k = s0 (1 - k / (H - 1)) for k < H - 1, the last row 0
//       (make_reference, scripts/train_cartpole.py:103-110)
// (the reference's NLP has no action cost, takes a linspace reference over H + 2
// points and drops the last stage's state cost).
//
// One iteration on the unknowns u[H]:
//   forward   H x cart_step<false> from s0, the cost J
//   reverse   H x cart_step_adjoint with the loss seeds -> g = dJ/du
//   update    m = beta m + alpha g,  u = clamp(u - m, -1, 1), inside the reverse
//             sweep: step k's adjoint is the last reader of u[k]
// m = 0 at the start of every solve, a fixed number of iterations, one more
// forward sweep for the cost of the returned u.
//
// Defaults iters 10, beta 0.5, alpha 5e-4, from a float64 sweep on the CPU
// (torch autograd over oracle.torch_port.CartpoleOracle, B = 512):
//   near-upright starts (rand - .5) [.6, .6, .4, .6]:
//     alpha 2e-3  diverges  (mean cost 48 -> 138)
//     alpha 1e-3  converges (48.3 -> 3.28 in 10 iterations)
//     alpha 5e-4  converges (48.3 -> 3.40)
//   full-range and swing-up starts, alpha 5e-4: no trajectory ends above its
//   start cost.
// 5e-4 is a factor 2-4 below the stability limit.
//
// The solver is stated once, generic over the MODEL inside the horizon:
//   CartMpcAnalytic  cart_step<false> on ApgCartpoleParams' constants
//   CartMpcLearnt    LearntCartpoleDynamics with the same unwrapped step
//                    (cart_learnt_step<false>): the physics on the module's six
//                    live parameters plus W2 relu(W1 [s; a] + b1) on the pre-step
//                    state and the raw action, added to all four components.
//                    The role of the reference's LearntDynamicsMPC
//                    (neural_control/dynamics/learnt_dynamics.py:5-55).
// A model has step(s, a) -> CartAux, adjoint(lam, pre, a, x) -> dJ/da and
// kPre: whether the adjoint reads the pre-step x and theta (the residual's
// hidden layer is recomputed from them in the reverse sweep, by
// cart_learnt_step_adjoint as the rollout kernels have it); they join the
// stash then, 14 floats per step instead of 12.  Cost, reference, update rule,
// box, warm start and defaults are the same for both (float64 restatement with
// the fitted module of tests/golden/cartpole_learnt.npz, 256 starts in thirds:
// no trajectory ends above its start cost after 1, 10 or 20 iterations).
#pragma once
#include "cart_flight_rule.h"
#include "cartpole_learnt_math.h"

namespace apg {
namespace {

// what the reverse sweep needs of the forward one, per step: cart_step's aux,
// the two pre-step velocities and the three weighted residuals (2 w_i d_i for
// x_dot, theta, theta_dot; the cart position carries no cost) - 12 floats;
// PRE: the pre-step x and theta as well
template <int H, bool PRE>
struct CartMpcStash {
  CartAux x[H];
  float xd[H], thd[H];
  float seed[H][3];
  float px[PRE ? H : 1], pth[PRE ? H : 1];
};

struct CartMpcAnalytic {
  static constexpr bool kPre = false;
  CartConst c;
  __host__ __device__ __forceinline__ CartAux step(float (&s)[4], float a) const {
    return cart_step<false>(s, a, c);
  }
  __host__ __device__ __forceinline__ float adjoint(float (&lam)[4], const float (&pre)[4],
                                                    float, const CartAux &x) const {
    return cart_step_adjoint(lam, pre[1], pre[3], x, c);
  }
};

// rows: the residual's 640 packed floats (cart_residual_packed; LDS on the
// device), c: make_learnt_const of the module's six parameters
struct CartMpcLearnt {
  static constexpr bool kPre = true;
  CartConst c;
  const float *rows;
  __host__ __device__ __forceinline__ CartAux step(float (&s)[4], float a) const {
    return cart_learnt_step<false>(s, a, c, rows);
  }
  __host__ __device__ __forceinline__ float adjoint(float (&lam)[4], const float (&pre)[4],
                                                    float a, const CartAux &x) const {
    return cart_learnt_step_adjoint(lam, pre, a, x, c, rows);
  }
};

// make_reference's fade of row k (a compile-time constant once unrolled)
template <int H>
__host__ __device__ __forceinline__ float cart_mpc_fade(int k) {
  return k < H - 1 ? (float)(1.0 - (double)k / (double)(H - 1)) : 0.f;
}

// Returns J of the plan u from s0.
template <int H, bool STASH, class Model>
__host__ __device__ __forceinline__ float cart_mpc_forward(const float (&s0)[4],
                                                           const float (&u)[H],
                                                           const Model &c,
                                                           CartMpcStash<H, Model::kPre> &st) {
  const float wq[3] = {3.f, 10.f, 1.f};
  float s[4] = {s0[0], s0[1], s0[2], s0[3]};
  float J = 0.f;
#pragma unroll
  for (int k = 0; k < H; ++k) {
    if (STASH) st.xd[k] = s[1], st.thd[k] = s[3];
    if (STASH && Model::kPre) st.px[k] = s[0], st.pth[k] = s[2];
    const CartAux x = c.step(s, u[k]);
    if (STASH) st.x[k] = x;
    const float f = cart_mpc_fade<H>(k);
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float d = s[1 + i] - s0[1 + i] * f;
      l += (d * d) * wq[i];
      if (STASH) st.seed[k][i] = 2.f * wq[i] * d;
    }
    J += l + 0.01f * (u[k] * u[k]);
  }
  return J;
}

// reverse sweep + update of u and m
template <int H, class Model>
__host__ __device__ __forceinline__ void cart_mpc_reverse_update(
    const CartMpcStash<H, Model::kPre> &st, float (&u)[H], float (&m)[H], const Model &c,
    const ApgCartpoleMpcOptions &o) {
  float lam[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = H - 1; k >= 0; --k) {
#pragma unroll
    for (int i = 0; i < 3; ++i) lam[1 + i] += st.seed[k][i];
    const float pre[4] = {Model::kPre ? st.px[k] : 0.f, st.xd[k],
                          Model::kPre ? st.pth[k] : 0.f, st.thd[k]};
    const float g = c.adjoint(lam, pre, u[k], st.x[k]) + 0.02f * u[k];
    m[k] = o.beta * m[k] + o.alpha * g;
    u[k] = fminf(fmaxf(u[k] - m[k], -1.f), 1.f);
  }
}

// o.iters iterations from u (in: start, out: solution); trace(i, J) is called
// with the cost before iteration i and, for i = iters, with the returned cost
template <int H, class Model, class Trace>
__host__ __device__ __forceinline__ float cart_mpc_solve(const float (&s0)[4], float (&u)[H],
                                                         const Model &c,
                                                         const ApgCartpoleMpcOptions &o,
                                                         Trace &&trace) {
  float m[H];
#pragma unroll
  for (int k = 0; k < H; ++k) m[k] = 0.f;
  CartMpcStash<H, Model::kPre> st;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int it = 0; it < o.iters; ++it) {
    trace(it, cart_mpc_forward<H, true>(s0, u, c, st));
    cart_mpc_reverse_update<H>(st, u, m, c, o);
  }
  const float J = cart_mpc_forward<H, false>(s0, u, c, st);
  trace(o.iters, J);
  return J;
}

// warm start of the next control step: rows move up, the last one is repeated
template <int H>
__host__ __device__ __forceinline__ void cart_mpc_shift(float (&u)[H]) {
#pragma unroll
  for (int k = 0; k + 1 < H; ++k) u[k] = u[k + 1];
}

// The log of one flight of a [..][B] batch: a NULL output drops its writes
struct CartMpcFlightLog {
  float *states, *actions, *cost;   // [T][4][B], [T][B], [T][B]
  size_t B, b;
  template <int N>
  __host__ __device__ __forceinline__ void put(float *out, int row, const float (&v)[N]) const {
    if (!out) return;
#pragma unroll
    for (int i = 0; i < N; ++i) out[((size_t)row * N + i) * B + b] = v[i];
  }
};

// One closed-loop episode (cart_flight_rule.h) with the controller "shift the
// warm start, solve on the model `cm` (CartMpcAnalytic / CartMpcLearnt), apply
// u[0]" (first step: from u = 0).
// plant(s, a): the environment's step, before the theta wrap.  The cart
// position is NOT zeroed between steps (that is Net.forward's side effect in
// the network controller's loop).  go_on(alive): false ends the loop - the
// wave's vote on the device, the flight's own flag on the host.
template <int H, class Plant, class GoOn, class Model>
__host__ __device__ __forceinline__ CartFlightBook cart_mpc_flight(
    const float (&s0)[4], Plant &&plant, GoOn &&go_on, const Model &cm,
    const ApgCartpoleMpcOptions &o, const CartFlightRule &rule, const CartMpcFlightLog &log,
    bool live) {
  float s[4] = {s0[0], s0[1], s0[2], s0[3]}, u[H];
#pragma unroll
  for (int k = 0; k < H; ++k) u[k] = 0.f;
  CartFlightBook f;
  f.alive = live;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int k = 0; k < rule.T; ++k) {
    if (k > 0) cart_mpc_shift<H>(u);
    const float J[1] = {cart_mpc_solve<H>(s, u, cm, o, [](int, float) {})};
    const float a[1] = {u[0]};
    plant(s, a[0]);
    s[2] = CartFlightRule::wrap(s[2]);
    if (f.alive) {
      log.put(log.states, k, s);
      log.put(log.actions, k, a);
      log.put(log.cost, k, J);
    }
    rule.book(k, s, f);
    if (!go_on(f.alive)) break;
  }
  return f;
}

// argument rules shared by the device entry points and the twins; NULL: fine
inline const char *cart_mpc_check_options(const ApgCartpoleMpcOptions *o, int H) {
  if (!o) return "options is NULL";
  if (o->iters < 0 || o->iters > 100000) return "iters must be in [0, 100000]";
  if (!(o->beta >= 0.f && o->beta < 1.f)) return "beta must be in [0, 1)";
  if (!(o->alpha > 0.f)) return "alpha must be positive";
  if (H != 5 && H != 10) return "H must be 5 or 10";
  return nullptr;
}

inline const char *cart_mpc_check(const ApgCartpoleParams *model,
                                  const ApgCartpoleMpcOptions *o, int H) {
  if (!model) return "model is NULL";
  return cart_mpc_check_options(o, H);
}

// the learnt model: its residual must be given
inline const char *cart_mpc_check(const ApgCartpoleLearnt *model,
                                  const ApgCartpoleMpcOptions *o, int H) {
  if (const char *e = cart_learnt_check(model, true)) return e;
  return cart_mpc_check_options(o, H);
}

// the optional learnt plant: NULL is "none", a given one carries its residual
inline const char *cart_mpc_check_learnt(const ApgCartpoleLearnt *m) {
  return m && cart_learnt_check(m, true)
             ? "learnt plant pointer is NULL (the residual must be given)"
             : nullptr;
}

}  // namespace
}  // namespace apg
