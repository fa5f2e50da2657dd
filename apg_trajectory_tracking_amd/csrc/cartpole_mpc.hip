// cartpole_mpc.hip - batched shooting MPC for the cart-pole (include/apg.h:
// apg_cartpole_mpc_solve, apg_cartpole_mpc_closed_loop): the solver of
// cartpole_mpc_math.h, one trajectory per lane, one wave per workgroup.  Plain
// per-lane fp32 like the rollout kernel of cartpole.hip - there is no matrix
// product in it, so no MFMA.  Between the iterations of a solve nothing leaves
// the lane's registers: the unknowns (H), the momentum (H) and the forward
// sweep's stash for the reverse one (12 H) are 140 floats at H = 10 -
// kernel_resources.json must show no scratch and no spill for every
// instantiation (tests/test_cartpole_mpc_cpu.py).
#include "cartpole_mpc_math.h"

namespace apg {
namespace {

constexpr int kCartMpcThreads = 64;

struct CartMpcSolveArgs {
  const float *state0, *u0;            // [4][B], [H][B] or NULL
  float *u, *cost_out, *cost_trace;    // [H][B], [B], [iters + 1][B]; NULL: dropped
  CartConst c;
  ApgCartpoleMpcOptions o;
  int B;
};

template <int H>
__global__ __launch_bounds__(kCartMpcThreads) void cart_mpc_solve_kernel(CartMpcSolveArgs A) {
  const int b = blockIdx.x * kCartMpcThreads + threadIdx.x;
  if (b >= A.B) return;
  const size_t B = (size_t)A.B;
  float s0[4], u[H];
#pragma unroll
  for (int i = 0; i < 4; ++i) s0[i] = A.state0[i * B + b];
#pragma unroll
  for (int k = 0; k < H; ++k) u[k] = A.u0 ? A.u0[k * B + b] : 0.f;
  float *trace = A.cost_trace;
  const float J = cart_mpc_solve<H>(s0, u, A.c, A.o, [&](int i, float Ji) {
    if (trace) trace[(size_t)i * B + b] = Ji;
  });
  if (A.cost_out) A.cost_out[b] = J;
  if (A.u) {
#pragma unroll
    for (int k = 0; k < H; ++k) A.u[k * B + b] = u[k];
  }
}

struct CartMpcLoopArgs {
  const float *state0;   // [4][B]
  int *steps, *upright;  // [B]
  double *vel_sum, *vel_sq;
  CartMpcFlightLog log;  // B, b: set per lane
  ApgCartpoleLearnt m;   // the learnt plant's tensors (LEARNT)
  CartConst cp, cm;      // plant (analytic; LEARNT: dt only), model
  ApgCartpoleMpcOptions o;
  CartFlightRule rule;
  int B;
};

// cart_mpc_flight (cartpole_mpc_math.h), one episode per lane.  LEARNT: the
// plant is LearntCartpoleDynamics.forward - its residual's unit rows sit in
// LDS (as cart_closed_loop_kernel<true> stages them), every lane evaluates all
// 64 units for its own episode; the six physical parameters are read here.
template <int H, bool LEARNT>
__global__ __launch_bounds__(kCartMpcThreads) void cart_mpc_closed_loop_kernel(CartMpcLoopArgs A) {
  __shared__ float rows[LEARNT ? kCartResFloats : 1];
  CartConst cp = A.cp;
  if constexpr (LEARNT) {
    for (int t = threadIdx.x; t < kCartResFloats; t += kCartMpcThreads)
      rows[t] = cart_residual_packed(t, A.m.w1, A.m.b1, A.m.w2);
    cp = make_learnt_const(CartLearntParams{*A.m.max_force_mag, *A.m.masspole, *A.m.length,
                                            *A.m.friction, *A.m.total_mass,
                                            *A.m.polemass_length},
                           A.cp.dt);
    __syncthreads();
  }
  const int b = blockIdx.x * kCartMpcThreads + threadIdx.x;
  const bool live = b < A.B;
  const size_t B = (size_t)A.B;
  float s0[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) s0[i] = live ? A.state0[i * B + b] : 0.f;
  CartMpcFlightLog log = A.log;
  log.B = B, log.b = (size_t)b;
  // a lane past the batch, or an episode that has stopped, keeps stepping with
  // its wave (no writes); the wave leaves when none of its episodes is alive
  const CartFlightBook f = cart_mpc_flight<H>(
      s0,
      [&](float (&s)[4], float a) {
        if constexpr (LEARNT) cart_learnt_step(s, a, cp, rows);
        else cart_step(s, a, cp);
      },
      [](bool alive) { return __any(alive) != 0; }, A.cm, A.o, A.rule, log, live);
  if (live) {
    A.steps[b] = f.steps;
    A.upright[b] = f.upright ? 1 : 0;
    A.vel_sum[b] = f.vel_sum;
    A.vel_sq[b] = f.vel_sq;
  }
}

int fail_arg(const char *e) {
  set_error("%s", e);
  return APG_ERR_ARG;
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_cartpole_mpc_solve(const float *state0, const float *u0, float dt,
                           const ApgCartpoleParams *model, const ApgCartpoleMpcOptions *opt,
                           int B, int H, float *u, float *cost_out, float *cost_trace,
                           apg_stream_t stream) {
  if (B < 0) return fail_arg("B must be >= 0");
  if (const char *e = cart_mpc_check(model, opt, H)) return fail_arg(e);
  if (B == 0) return APG_OK;
  if (!state0) return fail_arg("state0 is NULL");
  CartMpcSolveArgs A;
  A.state0 = state0, A.u0 = u0, A.u = u, A.cost_out = cost_out, A.cost_trace = cost_trace;
  A.c = make_const(*model, dt);
  A.o = *opt, A.B = B;
  const dim3 grid((B + kCartMpcThreads - 1) / kCartMpcThreads);
  hipStream_t st = (hipStream_t)stream;
  if (H == 5)
    hipLaunchKernelGGL(cart_mpc_solve_kernel<5>, grid, dim3(kCartMpcThreads), 0, st, A);
  else
    hipLaunchKernelGGL(cart_mpc_solve_kernel<10>, grid, dim3(kCartMpcThreads), 0, st, A);
  return check_launch("cartpole_mpc_solve");
}

int apg_cartpole_mpc_closed_loop(const float *state0, float dt, const ApgCartpoleParams *plant,
                                 const ApgCartpoleLearnt *plant_learnt,
                                 const ApgCartpoleParams *model,
                                 const ApgCartpoleMpcOptions *opt, int B, int H, int max_steps,
                                 int mode, float thresh_div, int burn_in, int *steps,
                                 int *upright, double *vel_sum, double *vel_sq, float *states,
                                 float *actions, float *cost, apg_stream_t stream) {
  if (const char *e = cart_mpc_check(model, opt, H)) return fail_arg(e);
  if (!plant && !plant_learnt) return fail_arg("plant is NULL");
  if (const char *e = cart_mpc_check_learnt(plant_learnt)) return fail_arg(e);
  if (const char *e = cart_flight_check(B, max_steps, mode)) return fail_arg(e);
  if (!state0 || !steps || !upright || !vel_sum || !vel_sq) return fail_arg("NULL buffer");
  CartMpcLoopArgs A = {};
  A.state0 = state0, A.steps = steps, A.upright = upright;
  A.vel_sum = vel_sum, A.vel_sq = vel_sq;
  A.log = {states, actions, cost, 0, 0};
  if (plant_learnt) {
    A.m = *plant_learnt;
    A.cp.dt = dt;          // (the rest is built in the kernel from the tensors)
  } else {
    A.cp = make_const(*plant, dt);
  }
  A.cm = make_const(*model, dt);
  A.o = *opt, A.B = B;
  A.rule = CartFlightRule{max_steps, mode, burn_in, thresh_div};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((B + kCartMpcThreads - 1) / kCartMpcThreads), block(kCartMpcThreads);
  if (H == 5) {
    if (plant_learnt)
      hipLaunchKernelGGL((cart_mpc_closed_loop_kernel<5, true>), grid, block, 0, st, A);
    else
      hipLaunchKernelGGL((cart_mpc_closed_loop_kernel<5, false>), grid, block, 0, st, A);
  } else {
    if (plant_learnt)
      hipLaunchKernelGGL((cart_mpc_closed_loop_kernel<10, true>), grid, block, 0, st, A);
    else
      hipLaunchKernelGGL((cart_mpc_closed_loop_kernel<10, false>), grid, block, 0, st, A);
  }
  return check_launch("cartpole_mpc_closed_loop");
}

}  // extern "C"
