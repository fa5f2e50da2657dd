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
  float *div;         // [T][B]
  int *steps;         // [B]
  float *drone;       // [T+1][12][B] or NULL
  float *actions;     // [T][4][B] or NULL
  float *start;       // [T][12][B] or NULL
  float *cost;        // [T][B] or NULL
  const float *learnt;  // packed plant residual (learnt_pack_kernel) or NULL
  QuadConst cp, cm;   // plant, model
  ApgQuadLossWeights w;
  ApgQuadMpcOptions o;
  int B, L, T, test_time;
  float thresh_div, thresh_stable;
};

// The loop of mlp_closed_loop_kernel (mlp_rollout.hip) with the policy replaced
// by "shift, solve, apply u[0]"; one flight per lane.
template <bool LEARNT>
__global__ __launch_bounds__(kMpcThreads) void quad_mpc_closed_loop_kernel(MpcLoopArgs A) {
  constexpr int H = 10;
  __shared__ float lr[LEARNT ? kLearntFloats : 1];
  if (LEARNT) {
    for (int i = threadIdx.x; i < kLearntFloats; i += kMpcThreads) lr[i] = A.learnt[i];
    __syncthreads();
  }
  const int b = blockIdx.x * kMpcThreads + threadIdx.x;
  if (b >= A.B) return;
  const size_t B = (size_t)A.B;
  const int T = A.T, L = A.L;
  const float *tr = A.traj + b;
  float s[12], win[H][6], u[H][4];
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = i < 3 ? tr[i * B] : 0.f;  // zero_reset
#pragma unroll
  for (int r = 0; r < H; ++r)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      win[r][i] = tr[((size_t)(1 + r) * 9 + i) * B];
      win[r][3 + i] = tr[((size_t)(1 + r) * 9 + 6 + i) * B];
    }
#pragma unroll
  for (int k = 0; k < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) u[k][j] = 0.5f;
  if (A.drone) {
#pragma unroll
    for (int i = 0; i < 12; ++i) A.drone[i * B + b] = s[i];
  }
  bool alive = true;
  int steps = 0;

#pragma unroll 1
  for (int k = 0; k < T; ++k) {
    if (A.start && alive) {
#pragma unroll
      for (int i = 0; i < 12; ++i) A.start[((size_t)k * 12 + i) * B + b] = s[i];
    }
    if (k > 0) mpc_shift<H>(u);
    const float J = mpc_solve<H>(s, win, u, A.cm, A.w, A.o, [](int, float) {});
    if (alive) {
      if (A.cost) A.cost[(size_t)k * B + b] = J;
      if (A.actions) {
#pragma unroll
        for (int j = 0; j < 4; ++j) A.actions[((size_t)k * 4 + j) * B + b] = u[0][j];
      }
    }
    const Trig t = make_trig(&s[3]);
    if (LEARNT) learnt_quad_step_lane(s, u[0], A.cp, t, lr);
    else quad_step(s, u[0], A.cp, t);
    // window row 0 is reference[cur] after get_ref_traj: project_on_ref
    float d2 = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float e = win[0][q] - s[q];
      d2 = fmaf(e, e, d2);
    }
    const float dv = sqrtf(d2);
    const bool stable = fabsf(s[3]) < A.thresh_stable && fabsf(s[4]) < A.thresh_stable;
    const bool failed = dv > A.thresh_div || !stable;
    if (alive) {
      if (A.drone) {
#pragma unroll
        for (int i = 0; i < 12; ++i) A.drone[((size_t)(k + 1) * 12 + i) * B + b] = s[i];
      }
      A.div[(size_t)k * B + b] = dv;
      steps = k + 1;
    }
    if (A.test_time) {
      alive = alive && !failed;
      if (!__any(alive)) break;
    } else if (failed) {  // get_current_full_state: row cur, zero rates
      const int cur = k + 1 < L - H ? k + 1 : L - H;
#pragma unroll
      for (int i = 0; i < 9; ++i) s[i] = tr[((size_t)cur * 9 + i) * B];
#pragma unroll
      for (int i = 9; i < 12; ++i) s[i] = 0.f;
    }
    if (k + 2 <= L - H) {  // get_ref_traj advanced: slide, fetch row k+1+H
#pragma unroll
      for (int r = 0; r + 1 < H; ++r)
#pragma unroll
        for (int i = 0; i < 6; ++i) win[r][i] = win[r + 1][i];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        win[H - 1][i] = tr[((size_t)(k + 1 + H) * 9 + i) * B];
        win[H - 1][3 + i] = tr[((size_t)(k + 1 + H) * 9 + 6 + i) * B];
      }
    }
  }
  A.steps[b] = steps;
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

int apg_quad_mpc_closed_loop(const float *traj, int L, float dt,
                             const ApgQuadParams *plant,
                             const ApgLearntResidual *plant_learnt,
                             const ApgQuadParams *model,
                             const ApgQuadLossWeights *weights,
                             const ApgQuadMpcOptions *opt, int B, int H,
                             int max_steps, float thresh_div, float thresh_stable,
                             int test_time, float *div, int *steps, float *drone,
                             float *actions, float *start_states, float *cost,
                             float *workspace, apg_stream_t stream) {
  constexpr int kH = 10;
  if (int e = check_mpc(model, weights, opt, B)) return e;
  if (!plant) {
    set_error("plant is NULL");
    return APG_ERR_ARG;
  }
  if (H != kH) {
    set_error("H must be %d (got %d)", kH, H);
    return APG_ERR_ARG;
  }
  if (plant_learnt && (!plant_learnt->linear_at || !plant_learnt->w1 || !plant_learnt->b1 ||
                       !plant_learnt->w2 || !plant_learnt->b2)) {
    set_error("learnt simulator: weight pointer is NULL");
    return APG_ERR_ARG;
  }
  if (L <= kH || max_steps < 1) {
    set_error("closed loop needs L > %d reference rows and max_steps >= 1", kH);
    return APG_ERR_ARG;
  }
  if (B == 0) return APG_OK;
  if (!traj || !div || !steps || (plant_learnt && !workspace)) {
    set_error("NULL buffer");
    return APG_ERR_ARG;
  }
  MpcLoopArgs A;
  A.traj = traj, A.div = div, A.steps = steps, A.drone = drone, A.actions = actions;
  A.start = start_states, A.cost = cost, A.learnt = plant_learnt ? workspace : nullptr;
  A.cp = make_const(*plant, dt), A.cm = make_const(*model, dt);
  A.w = *weights, A.o = *opt;
  A.B = B, A.L = L, A.T = max_steps < L + 1 ? max_steps : L + 1, A.test_time = test_time;
  A.thresh_div = thresh_div, A.thresh_stable = thresh_stable;
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
