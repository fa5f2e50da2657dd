// quad_mpc.hip - batched shooting MPC for the quadrotor (include/apg.h:
// apg_quad_mpc_solve, apg_quad_mpc_closed_loop): the solver of quad_mpc_math.h,
// one trajectory per lane, one wave per workgroup.  Plain per-lane fp32 like
// the rollout kernels of quad.hip - there is no matrix product in it, so no
// MFMA.  Between the iterations of a solve nothing leaves the lane's registers:
// the unknowns (40), the momentum (40), the window rows (60) and the forward
// sweep's stash for the reverse one (153) are more than the 256 architectural
// VGPRs of a lane, which is why the kernels ask for ONE wave per SIMD
// (__launch_bounds__(64): the unified 512-entry file, the compiler parks what
// does not fit in the accumulation half) - kernel_resources.json must show no
// scratch and no spill for them (tests/test_quad_mpc_cpu.py).
#include "learnt_residual.h"
#include "quad_mpc_math.h"

namespace apg {
namespace {

constexpr int kMpcThreads = 64;

struct MpcSolveArgs {
  const float *state0, *ref;
  float *u, *cost_out, *cost_trace;
  QuadConst c;
  ApgQuadLossWeights w;
  ApgQuadMpcOptions o;
  int B, ref_cols;
};

template <int H>
__global__ __launch_bounds__(kMpcThreads) void quad_mpc_solve_kernel(MpcSolveArgs A) {
  const int b = blockIdx.x * kMpcThreads + threadIdx.x;
  if (b >= A.B) return;
  const size_t B = (size_t)A.B;
  const int rc = A.ref_cols, vc = rc == 9 ? 6 : 3;
  float s0[12], ref[H][6], u[H][4];
#pragma unroll
  for (int i = 0; i < 12; ++i) s0[i] = A.state0[i * B + b];
#pragma unroll
  for (int k = 0; k < H; ++k) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ref[k][i] = A.ref[((size_t)k * rc + i) * B + b];
      ref[k][3 + i] = A.ref[((size_t)k * rc + vc + i) * B + b];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) u[k][j] = A.u[((size_t)k * 4 + j) * B + b];
  }
  float *trace = A.cost_trace;
  const float J = mpc_solve<H>(s0, ref, u, A.c, A.w, A.o, [&](int i, float Ji) {
    if (trace) trace[(size_t)i * B + b] = Ji;
  });
  A.cost_out[b] = J;
#pragma unroll
  for (int k = 0; k < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) A.u[((size_t)k * 4 + j) * B + b] = u[k][j];
}

// LearntDynamics.forward for ONE trajectory per lane (learnt_residual.h has the
// half-wave form of the policy kernels): a' = A a, the analytic step on a',
// plus W2 relu(W1 [s, a'] + b1) + b2; `lr`: the packed weights in LDS
__device__ __forceinline__ void learnt_quad_step_lane(float (&s)[12], const float (&act)[4],
                                                      const QuadConst &c, const Trig &t,
                                                      const float *lr) {
  float x[16], at[4], add[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = s[i], add[i] = lr[kLrB2 + i];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float *a = lr + kLrA + 4 * i;
    x[12 + i] = at[i] = fmaf(a[3], act[3], fmaf(a[2], act[2], fmaf(a[1], act[1], a[0] * act[0])));
  }
  quad_step(s, at, c, t);
#pragma unroll 2
  for (int m = 0; m < 64; ++m) {
    float h = lr[kLrB1 + m];
#pragma unroll
    for (int j = 0; j < 16; ++j) h = fmaf(lr[kLrW1 + m * 16 + j], x[j], h);
    h = fmaxf(h, 0.f);
#pragma unroll
    for (int o = 0; o < 12; ++o) add[o] = fmaf(lr[kLrW2 + m * 12 + o], h, add[o]);
  }
#pragma unroll
  for (int o = 0; o < 12; ++o) s[o] += add[o];
}

struct MpcLoopArgs {
  const float *traj;  // [L][9][B]
  int *steps;         // [B]
  MpcFlightLog log;   // B, b: set per lane
  const float *learnt;  // packed plant residual (learnt_pack_kernel) or NULL
  QuadConst cp, cm;   // plant, model
  ApgQuadLossWeights w;
  ApgQuadMpcOptions o;
  QuadFlightRule rule;
  int B;
};

// mpc_flight (quad_mpc_math.h), one flight per lane
template <bool LEARNT>
__global__ __launch_bounds__(kMpcThreads) void quad_mpc_closed_loop_kernel(MpcLoopArgs A) {
  __shared__ float lr[LEARNT ? kLearntFloats : 1];
  if (LEARNT) {
    for (int i = threadIdx.x; i < kLearntFloats; i += kMpcThreads) lr[i] = A.learnt[i];
    __syncthreads();
  }
  const int b = blockIdx.x * kMpcThreads + threadIdx.x;
  if (b >= A.B) return;
  const size_t B = (size_t)A.B;
  const float *tr = A.traj + b;
  MpcFlightLog log = A.log;
  log.B = B, log.b = (size_t)b;
  A.steps[b] = mpc_flight(
      [&](int r, int col) { return tr[((size_t)r * 9 + col) * B]; },
      [&](float (&s)[12], const float (&u0)[4]) {
        const Trig t = make_trig(&s[3]);
        if (LEARNT) learnt_quad_step_lane(s, u0, A.cp, t, lr);
        else quad_step(s, u0, A.cp, t);
      },
      A.cm, A.w, A.o, A.rule, log);
}

int check_mpc(const ApgQuadParams *model, const ApgQuadLossWeights *weights,
              const ApgQuadMpcOptions *opt, int B) {
  if (B < 0) {
    set_error("B must be >= 0 (got %d)", B);
    return APG_ERR_ARG;
  }
  if (!model || !weights) {
    set_error("model / weights is NULL");
    return APG_ERR_ARG;
  }
  if (const char *e = mpc_check_options(opt)) {
    set_error("%s", e);
    return APG_ERR_ARG;
  }
  return APG_OK;
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_quad_mpc_solve(const float *state0, const float *ref, int ref_cols, float dt,
                       const ApgQuadParams *model, const ApgQuadLossWeights *weights,
                       const ApgQuadMpcOptions *opt, int B, int H, float *u,
                       float *cost_out, float *cost_trace, apg_stream_t stream) {
  if (int e = check_mpc(model, weights, opt, B)) return e;
  if (H != 5 && H != 10) {
    set_error("H must be 5 or 10 (got %d)", H);
    return APG_ERR_ARG;
  }
  if (ref_cols != 9 && ref_cols != 6) {
    set_error("ref_cols must be 9 ([pos, euler, vel]) or 6 ([pos, vel])");
    return APG_ERR_ARG;
  }
  if (B == 0) return APG_OK;
  if (!state0 || !ref || !u || !cost_out) {
    set_error("NULL buffer");
    return APG_ERR_ARG;
  }
  MpcSolveArgs A;
  A.state0 = state0, A.ref = ref, A.u = u, A.cost_out = cost_out, A.cost_trace = cost_trace;
  A.c = make_const(*model, dt);
  A.w = *weights, A.o = *opt;
  A.B = B, A.ref_cols = ref_cols;
  const dim3 grid((B + kMpcThreads - 1) / kMpcThreads);
  hipStream_t st = (hipStream_t)stream;
  if (H == 5)
    hipLaunchKernelGGL(quad_mpc_solve_kernel<5>, grid, dim3(kMpcThreads), 0, st, A);
  else
    hipLaunchKernelGGL(quad_mpc_solve_kernel<10>, grid, dim3(kMpcThreads), 0, st, A);
  return check_launch("quad_mpc_solve");
}

int apg_quad_mpc_workspace_floats(void) { return kLearntFloats; }

int apg_quad_mpc_closed_loop(const ApgQuadFlight *flight, float dt, const ApgQuadParams *plant,
                             const ApgLearntResidual *plant_learnt, const ApgQuadParams *model,
                             const ApgQuadLossWeights *weights, const ApgQuadMpcOptions *opt,
                             int B, int H, float *cost, float *workspace, apg_stream_t stream) {
  if (int e = check_mpc(model, weights, opt, B)) return e;
  if (!plant) {
    set_error("plant is NULL");
    return APG_ERR_ARG;
  }
  if (H != kFlightH) {
    set_error("H must be %d (got %d)", kFlightH, H);
    return APG_ERR_ARG;
  }
  MpcLoopArgs A;
  if (const char *e = quad_flight_check(flight, plant_learnt, B, &A.rule)) {
    set_error("%s", e);
    return APG_ERR_ARG;
  }
  if (B == 0) return APG_OK;
  if (plant_learnt && !workspace) {
    set_error("NULL buffer");
    return APG_ERR_ARG;
  }
  A.traj = flight->traj, A.steps = flight->steps;
  A.log = {flight->div, flight->drone, flight->actions, flight->start_states, cost, 0, 0};
  A.learnt = plant_learnt ? workspace : nullptr;
  A.cp = make_const(*plant, dt), A.cm = make_const(*model, dt);
  A.w = *weights, A.o = *opt, A.B = B;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((B + kMpcThreads - 1) / kMpcThreads);
  if (plant_learnt) {
    hipLaunchKernelGGL(learnt_pack_kernel, dim3((kLearntFloats + 255) / 256), dim3(256), 0, st,
                       *plant_learnt, workspace);
    hipLaunchKernelGGL(quad_mpc_closed_loop_kernel<true>, grid, dim3(kMpcThreads), 0, st, A);
  } else {
    hipLaunchKernelGGL(quad_mpc_closed_loop_kernel<false>, grid, dim3(kMpcThreads), 0, st, A);
  }
  return check_launch("quad_mpc_closed_loop");
}

}  // extern "C"
