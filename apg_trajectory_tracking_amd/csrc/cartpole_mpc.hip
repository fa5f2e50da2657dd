// cartpole_mpc.hip - batched shooting MPC for the cart-pole (include/apg.h:
// apg_cartpole_mpc_solve, apg_cartpole_mpc_closed_loop): the solver of
// cartpole_mpc_math.h, one trajectory per lane, one wave per workgroup.  Plain
// per-lane fp32 like the rollout kernel of cartpole.hip - there is no matrix
// product in it, so no MFMA.  Between the iterations of a solve nothing leaves
// the lane's registers: the unknowns (H), the momentum (H) and the forward
// sweep's stash for the reverse one (12 H) are 140 floats at H = 10 -
// kernel_resources.json must show no scratch and no spill for every
// instantiation (tests/test_cartpole_mpc_cpu.py).
//
// The cart_mpc_learnt_* kernels run the same solver on the LEARNT model
// (CartMpcLearnt; apg_cartpole_learnt_mpc_solve, _closed_loop): the module's
// 640 packed residual floats are staged once per workgroup in LDS (2.5 KB; all
// lanes read the same address), its six parameters are read from the module's
// device tensors here - no device-to-host read, a captured launch sees the
// values of the moment it is replayed.  The stash grows by the pre-step x and
// theta (14 H floats): still no scratch and no spill
// (tests/test_cartpole_learnt_mpc_cpu.py).
#include "cartpole_learnt_stage.h"
#include "cartpole_mpc_math.h"
#include "static_dispatch.h"

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

// one lane's solve on the model `cm`; Args: state0, u0, u, cost_out, cost_trace, o, B
template <int H, class Args, class Model>
__device__ __forceinline__ void cart_mpc_solve_lane(const Args &A, const Model &cm) {
  const int b = blockIdx.x * kCartMpcThreads + threadIdx.x;
  if (b >= A.B) return;
  const size_t B = (size_t)A.B;
  float s0[4], u[H];
#pragma unroll
  for (int i = 0; i < 4; ++i) s0[i] = A.state0[i * B + b];
#pragma unroll
  for (int k = 0; k < H; ++k) u[k] = A.u0 ? A.u0[k * B + b] : 0.f;
  float *trace = A.cost_trace;
  const float J = cart_mpc_solve<H>(s0, u, cm, A.o, [&](int i, float Ji) {
    if (trace) trace[(size_t)i * B + b] = Ji;
  });
  if (A.cost_out) A.cost_out[b] = J;
  if (A.u) {
#pragma unroll
    for (int k = 0; k < H; ++k) A.u[k * B + b] = u[k];
  }
}

template <int H>
__global__ __launch_bounds__(kCartMpcThreads) void cart_mpc_solve_kernel(CartMpcSolveArgs A) {
  cart_mpc_solve_lane<H>(A, CartMpcAnalytic{A.c});
}

struct CartLearntMpcSolveArgs {
  const float *state0, *u0;            // as CartMpcSolveArgs
  float *u, *cost_out, *cost_trace;
  ApgCartpoleLearnt model;             // the module's tensors
  float dt;
  ApgCartpoleMpcOptions o;
  int B;
};

template <int H>
__global__ __launch_bounds__(kCartMpcThreads) void cart_mpc_learnt_solve_kernel(
    CartLearntMpcSolveArgs A) {
  __shared__ float rows[kCartResFloats];
  const CartConst c = make_learnt_const(load_params(A.model), A.dt);
  stage_residual(rows, A.model);
  cart_mpc_solve_lane<H>(A, CartMpcLearnt{c, rows});
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

// cart_mpc_flight (cartpole_mpc_math.h), one episode per lane, on the plant
// `plant(s, a)` with the solver's model `cm`; Args: state0, steps, upright,
// vel_sum, vel_sq, log, o, rule, B
template <int H, class Args, class Plant, class Model>
__device__ __forceinline__ void cart_mpc_loop_lane(const Args &A, Plant &&plant,
                                                   const Model &cm) {
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
      s0, plant, [](bool alive) { return __any(alive) != 0; }, cm, A.o, A.rule, log, live);
  if (live) {
    A.steps[b] = f.steps;
    A.upright[b] = f.upright ? 1 : 0;
    A.vel_sum[b] = f.vel_sum;
    A.vel_sq[b] = f.vel_sq;
  }
}

// The solver plans with the analytic model A.cm.  LEARNT: the plant is
// LearntCartpoleDynamics.forward - its residual's unit rows sit in LDS (as
// cart_closed_loop_kernel<true> stages them), every lane evaluates all 64
// units for its own episode; the six physical parameters are read here.
template <int H, bool LEARNT>
__global__ __launch_bounds__(kCartMpcThreads) void cart_mpc_closed_loop_kernel(CartMpcLoopArgs A) {
  __shared__ float rows[LEARNT ? kCartResFloats : 1];
  CartConst cp = A.cp;
  if constexpr (LEARNT) {
    // (the plant's rows by a loop of the compile-time stride, here and below:
    // stage_residual strides by blockDim.x and compiles to other instructions)
    for (int t = threadIdx.x; t < kCartResFloats; t += kCartMpcThreads)
      rows[t] = cart_residual_packed(t, A.m.w1, A.m.b1, A.m.w2);
    cp = make_learnt_const(load_params(A.m), A.cp.dt);
    __syncthreads();
  }
  cart_mpc_loop_lane<H>(
      A,
      [&](float (&s)[4], float a) {
        if constexpr (LEARNT) cart_learnt_step(s, a, cp, rows);
        else cart_step(s, a, cp);
      },
      CartMpcAnalytic{A.cm});
}

struct CartLearntMpcLoopArgs {
  const float *state0;      // as CartMpcLoopArgs
  int *steps, *upright;
  double *vel_sum, *vel_sq;
  CartMpcFlightLog log;
  ApgCartpoleLearnt m;      // the learnt plant's tensors (LEARNT_PLANT)
  ApgCartpoleLearnt model;  // the solver's model
  CartConst cp;             // the analytic plant (LEARNT_PLANT: not read)
  float dt;
  ApgCartpoleMpcOptions o;
  CartFlightRule rule;
  int B;
};

// The solver plans through the module A.model.  LEARNT_PLANT: the plant is the
// module A.m (the same one or another): both row tables are staged, 5 KB.
template <int H, bool LEARNT_PLANT>
__global__ __launch_bounds__(kCartMpcThreads) void cart_mpc_learnt_closed_loop_kernel(
    CartLearntMpcLoopArgs A) {
  __shared__ float model_rows[kCartResFloats];
  __shared__ float rows[LEARNT_PLANT ? kCartResFloats : 1];
  const CartConst cm = make_learnt_const(load_params(A.model), A.dt);
  CartConst cp = A.cp;
  if constexpr (LEARNT_PLANT) {
    cp = make_learnt_const(load_params(A.m), A.dt);
    for (int t = threadIdx.x; t < kCartResFloats; t += kCartMpcThreads)
      rows[t] = cart_residual_packed(t, A.m.w1, A.m.b1, A.m.w2);
  }
  stage_residual(model_rows, A.model);   // (its barrier covers `rows` as well)
  cart_mpc_loop_lane<H>(
      A,
      [&](float (&s)[4], float a) {
        if constexpr (LEARNT_PLANT) cart_learnt_step(s, a, cp, rows);
        else cart_step(s, a, cp);
      },
      CartMpcLearnt{cm, model_rows});
}

int fail_arg(const char *e) {
  set_error("%s", e);
  return APG_ERR_ARG;
}

// the solver's model into a kernel's arguments: the analytic one as its
// constants, the learnt one as the module's tensors and dt
void set_model(CartMpcSolveArgs &A, const ApgCartpoleParams &m, float dt) {
  A.c = make_const(m, dt);
}
void set_model(CartMpcLoopArgs &A, const ApgCartpoleParams &m, float dt) {
  A.cm = make_const(m, dt);
}
template <class Args>
void set_model(Args &A, const ApgCartpoleLearnt &m, float dt) {
  A.model = m, A.dt = dt;
}

// The solve behind both entry points; Args / Model: CartMpcSolveArgs with the
// analytic model's parameters, CartLearntMpcSolveArgs with a learnt module.
template <class Args, class Model>
int cart_mpc_solve_launch(const char *name, const float *state0, const float *u0, float dt,
                          const Model *model, const ApgCartpoleMpcOptions *opt, int B, int H,
                          float *u, float *cost_out, float *cost_trace, apg_stream_t stream) {
  if (B < 0) return fail_arg("B must be >= 0");
  if (const char *e = cart_mpc_check(model, opt, H)) return fail_arg(e);
  if (B == 0) return APG_OK;
  if (!state0) return fail_arg("state0 is NULL");
  Args A;
  A.state0 = state0, A.u0 = u0, A.u = u, A.cost_out = cost_out, A.cost_trace = cost_trace;
  set_model(A, *model, dt);
  A.o = *opt, A.B = B;
  const dim3 grid((B + kCartMpcThreads - 1) / kCartMpcThreads), block(kCartMpcThreads);
  hipStream_t st = (hipStream_t)stream;
  with_horizon(H, [&](auto h) {
    if constexpr (std::is_same<Model, ApgCartpoleLearnt>::value)
      hipLaunchKernelGGL(cart_mpc_learnt_solve_kernel<h()>, grid, block, 0, st, A);
    else
      hipLaunchKernelGGL(cart_mpc_solve_kernel<h()>, grid, block, 0, st, A);
  });
  return check_launch(name);
}

// The closed loop behind both entry points, Args / Model as above.
template <class Args, class Model>
int cart_mpc_loop_launch(const char *name, const ApgCartpoleFlight *flight, float dt,
                         const ApgCartpoleParams *plant, const ApgCartpoleLearnt *plant_learnt,
                         const Model *model, const ApgCartpoleMpcOptions *opt, int B, int H,
                         float *cost, apg_stream_t stream) {
  Args A = {};
  if (const char *e = cart_mpc_check(model, opt, H)) return fail_arg(e);
  if (!plant && !plant_learnt) return fail_arg("plant is NULL");
  if (const char *e = cart_mpc_check_learnt(plant_learnt)) return fail_arg(e);
  if (const char *e = cart_flight_check(flight, B, &A.rule)) return fail_arg(e);
  A.state0 = flight->state0, A.steps = flight->steps, A.upright = flight->upright;
  A.vel_sum = flight->vel_sum, A.vel_sq = flight->vel_sq;
  A.log = {flight->states, flight->actions, cost, 0, 0};
  if (plant_learnt) {
    A.m = *plant_learnt;
    A.cp.dt = dt;          // (the rest is built in the kernel from the tensors)
  } else {
    A.cp = make_const(*plant, dt);
  }
  set_model(A, *model, dt);
  A.o = *opt, A.B = B;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((B + kCartMpcThreads - 1) / kCartMpcThreads), block(kCartMpcThreads);
  with_horizon(H, [&](auto h) {
    with_flag(plant_learnt != nullptr, [&](auto learnt_plant) {
      constexpr int kH = decltype(h)::value;
      constexpr bool kPlant = decltype(learnt_plant)::value;
      if constexpr (std::is_same<Model, ApgCartpoleLearnt>::value)
        hipLaunchKernelGGL((cart_mpc_learnt_closed_loop_kernel<kH, kPlant>), grid, block, 0, st,
                           A);
      else
        hipLaunchKernelGGL((cart_mpc_closed_loop_kernel<kH, kPlant>), grid, block, 0, st, A);
    });
  });
  return check_launch(name);
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_cartpole_mpc_solve(const float *state0, const float *u0, float dt,
                           const ApgCartpoleParams *model, const ApgCartpoleMpcOptions *opt,
                           int B, int H, float *u, float *cost_out, float *cost_trace,
                           apg_stream_t stream) {
  return cart_mpc_solve_launch<CartMpcSolveArgs>("cartpole_mpc_solve", state0, u0, dt, model,
                                                 opt, B, H, u, cost_out, cost_trace, stream);
}

int apg_cartpole_mpc_closed_loop(const ApgCartpoleFlight *flight, float dt,
                                 const ApgCartpoleParams *plant,
                                 const ApgCartpoleLearnt *plant_learnt,
                                 const ApgCartpoleParams *model,
                                 const ApgCartpoleMpcOptions *opt, int B, int H,
                                 float *cost, apg_stream_t stream) {
  return cart_mpc_loop_launch<CartMpcLoopArgs>("cartpole_mpc_closed_loop", flight, dt, plant,
                                               plant_learnt, model, opt, B, H, cost, stream);
}

int apg_cartpole_learnt_mpc_solve(const float *state0, const float *u0, float dt,
                                  const ApgCartpoleLearnt *model,
                                  const ApgCartpoleMpcOptions *opt, int B, int H, float *u,
                                  float *cost_out, float *cost_trace, apg_stream_t stream) {
  return cart_mpc_solve_launch<CartLearntMpcSolveArgs>("cartpole_learnt_mpc_solve", state0, u0,
                                                       dt, model, opt, B, H, u, cost_out,
                                                       cost_trace, stream);
}

int apg_cartpole_learnt_mpc_closed_loop(const ApgCartpoleFlight *flight, float dt,
                                        const ApgCartpoleParams *plant,
                                        const ApgCartpoleLearnt *plant_learnt,
                                        const ApgCartpoleLearnt *model,
                                        const ApgCartpoleMpcOptions *opt, int B, int H,
                                        float *cost, apg_stream_t stream) {
  return cart_mpc_loop_launch<CartLearntMpcLoopArgs>("cartpole_learnt_mpc_closed_loop", flight,
                                                     dt, plant, plant_learnt, model, opt, B, H,
                                                     cost, stream);
}

}  // extern "C"
