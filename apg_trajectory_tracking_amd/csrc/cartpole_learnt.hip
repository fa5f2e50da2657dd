// cartpole_learnt.hip - LearntCartpoleDynamics on the GPU: the step with its
// reverse (every parameter's batch-summed cotangent) and the fused controller
// phase through it.
//
// Restated from (paths relative to the reference repo):
//   neural_control/dynamics/cartpole_dynamics.py:122-140 (the class; the
//     physics :53-119 on the module's live parameters)
//   neural_control/dynamics/learnt_dynamics.py:58-98 (the 5 -> 64 -> 4 relu
//     residual on [state, action], no output bias)
//   scripts/train_base.py:160-186 (train_dynamics_model: what the reverse
//     feeds), scripts/train_cartpole.py:103-150 (the controller branch)
// Per-lane arithmetic: cartpole_learnt_math.h.  The parameters are read from
// the module's own device tensors (ApgCartpoleLearnt): no host read-back, no
// synchronisation, graph-capturable, always the optimizer's latest values.
// The residual's 640 weights are staged once per workgroup into LDS as unit
// rows [W1[m][0..4], b1[m], W2[0..3][m]] - every lane reads the same row at
// the same time (broadcast).
//
// The parameter reverse sums over the batch in two stages and without float
// atomics, so the same inputs give the same bits: each wave writes one row of
// 646 partials (the six physical ones by a shuffle tree; the 640 weight ones by
// its 64 lanes, lane m owning hidden unit m and looping over the wave's 64
// samples, which it reads from LDS), then one small kernel adds the rows in
// wave order.
#include <stddef.h>

#include "apg_device.h"
#include "cartpole_learnt_math.h"
#include "cartpole_learnt_stage.h"
#include "cartpole_rollout_math.h"

namespace apg {
namespace {

inline int grid_for(int B, int block) { return (B + block - 1) / block; }

constexpr int kStepBlock = 256;
constexpr int kStepWaves = kStepBlock / kWave;

// (stage_residual, load_params: cartpole_learnt_stage.h)

__global__ __launch_bounds__(kStepBlock) void cart_learnt_step_fwd_kernel(
    const float *__restrict__ state, const float *__restrict__ action, ApgCartpoleLearnt m,
    float dt, int B, float *__restrict__ next) {
  __shared__ float rows[kCartResFloats];
  const bool res = m.w1 != nullptr;
  if (res) stage_residual(rows, m);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const CartConst c = make_learnt_const(load_params(m), dt);
  float s[4];
  load_state<APG_LAYOUT_AOS, 4>(state, B, b, s);
  cart_learnt_step(s, action[b], c, res ? rows : nullptr);
  store_state<APG_LAYOUT_AOS, 4>(next, B, b, s);
}

__global__ __launch_bounds__(kStepBlock) void cart_learnt_step_bwd_kernel(
    const float *__restrict__ state, const float *__restrict__ action, ApgCartpoleLearnt m,
    float dt, int B, const float *__restrict__ grad_next, float *__restrict__ grad_state,
    float *__restrict__ grad_action, float *__restrict__ wave_partials) {
  __shared__ float rows[kCartResFloats];
  __shared__ float smp[kStepWaves][9][kWave];   // per wave: z (5), lam (4) per sample
  const bool res = m.w1 != nullptr;
  if (res) stage_residual(rows, m);
  const int lane = threadIdx.x & (kWave - 1), wl = threadIdx.x >> 6;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t wave = (size_t)(blockIdx.x * kStepWaves + wl);
  const CartLearntParams p = load_params(m);
  const CartConst c = make_learnt_const(p, dt);
  float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float z[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, lam0[4] = {0.f, 0.f, 0.f, 0.f};
  if (b < B) {
    float s[4], lam[4];
    load_state<APG_LAYOUT_AOS, 4>(state, B, b, s);
    load_state<APG_LAYOUT_AOS, 4>(grad_next, B, b, lam);
    const float a = action[b];
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = s[i], lam0[i] = lam[i];
    z[4] = a;
    float tmp[4] = {s[0], s[1], s[2], s[3]};
    const CartAux x = cart_step(tmp, a, c);
    cart_param_adjoint(lam, a, s[1], s[3], x, p, dt, g);
    const float ga = cart_learnt_step_adjoint(lam, s, a, x, c, res ? rows : nullptr);
    if (grad_state) store_state<APG_LAYOUT_AOS, 4>(grad_state, B, b, lam);
    if (grad_action) grad_action[b] = ga;
  }
  float *row = wave_partials + wave * kCartLearntGrads;
#pragma unroll
  for (int i = 0; i < kCartPhysGrads; ++i) {
    const float v = wave_sum(g[i]);
    if (lane == 0) row[i] = v;
  }
  if (!res) {
    for (int i = kCartPhysGrads + lane; i < kCartLearntGrads; i += kWave) row[i] = 0.f;
    return;
  }
  // the wave's samples into LDS, then lane m = hidden unit m over all 64
  // (a dead lane holds zeros: it adds nothing)
#pragma unroll
  for (int j = 0; j < 5; ++j) smp[wl][j][lane] = z[j];
#pragma unroll
  for (int o = 0; o < 4; ++o) smp[wl][5 + o][lane] = lam0[o];
  __syncthreads();
  float w[kCartResRow], gw[kCartResRow];
#pragma unroll
  for (int j = 0; j < kCartResRow; ++j) w[j] = rows[lane * kCartResRow + j], gw[j] = 0.f;
#pragma unroll 4
  for (int n = 0; n < kWave; ++n) {
    const float zn[5] = {smp[wl][0][n], smp[wl][1][n], smp[wl][2][n], smp[wl][3][n],
                         smp[wl][4][n]};
    const float ln[4] = {smp[wl][5][n], smp[wl][6][n], smp[wl][7][n], smp[wl][8][n]};
    cart_residual_unit_grads(w, zn, ln, gw);
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) row[kCartGW1 + lane * 5 + j] = gw[j];
  row[kCartGB1 + lane] = gw[5];
#pragma unroll
  for (int o = 0; o < 4; ++o) row[kCartGW2 + o * kCartResHidden + lane] = gw[6 + o];
}

// grad_params[i] = sum over the wave rows, in wave order
__global__ __launch_bounds__(256) void cart_learnt_reduce_kernel(
    const float *__restrict__ wave_partials, int waves, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kCartLearntGrads) return;
  float acc = 0.f;
  for (int w = 0; w < waves; ++w) acc += wave_partials[(size_t)w * kCartLearntGrads + i];
  out[i] = acc;
}

struct CartLearntRolloutArgs {
  const float *state0, *actions;
  float *loss_partials, *grad_actions, *grad_state0, *states_out;
  ApgCartpoleLearnt m;
  float dt;
  int B, H;
};

// cart_rollout_kernel (cartpole.hip) through the learnt step: the residual rows
// in LDS, then the pre-step states [k][4][lane]; the reverse recomputes each
// step's aux and hidden layer from the stashed state.
template <int LAYOUT>
__global__ __launch_bounds__(APG_ROLLOUT_BLOCK) void cart_learnt_rollout_kernel(
    CartLearntRolloutArgs A) {
  extern __shared__ float lds[];
  float *rows = lds, *stash = lds + kCartResFloats;
  stage_residual(rows, A.m);
  const int lane = threadIdx.x;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = b < A.B;
  const int bb = live ? b : A.B - 1;
  const CartConst c = make_learnt_const(load_params(A.m), A.dt);
  const int H = A.H;
  auto action = [&](int k) {
    float a[1];
    load_seq<LAYOUT, 1>(A.actions, A.B, H, 1, bb, k, 0, a);
    return a[0];
  };
  auto ST = [&](int k, int i) -> float & {
    return stash[(k * 4 + i) * APG_ROLLOUT_BLOCK + lane];
  };
  float s0[4], s[4], lam[4];
  load_state<LAYOUT, 4>(A.state0, A.B, bb, s0);
  const float loss = cart_rollout_forward(
      H, s0, s, action, ST, [&](float (&x)[4], float a) { cart_learnt_step(x, a, c, rows); },
      [&](int k, const float (&x)[4]) {
        if (A.states_out && live) store_seq<LAYOUT, 4>(A.states_out, A.B, H, 4, b, k, 0, x);
      });
  write_wave_partial(A.loss_partials, live ? loss : 0.f, (A.B + kWave - 1) / kWave);
  cart_rollout_reverse(
      H, s0, s, lam, action, ST,
      [&](float (&l)[4], const float (&pre)[4], float a) {
        return cart_learnt_step_adjoint(l, pre, a, cart_step_aux(pre, a, c), c, rows);
      },
      [&](int k, float g) {
        const float ga[1] = {g};
        if (live) store_seq<LAYOUT, 1>(A.grad_actions, A.B, H, 1, b, k, 0, ga);
      });
  if (A.grad_state0 && live) store_state<LAYOUT, 4>(A.grad_state0, A.B, b, lam);
}

int check_model(const ApgCartpoleLearnt *m, bool need_residual) {
  const char *e = cart_learnt_check(m, need_residual);
  if (e) set_error("%s", e);
  return e ? APG_ERR_ARG : APG_OK;
}

int check_step(const float *state, const float *action, const ApgCartpoleLearnt *m, int B) {
  if (B < 0) { set_error("B must be >= 0 (got %d)", B); return APG_ERR_ARG; }
  if (int e = check_model(m, false)) return e;
  if (B > 0 && (!state || !action)) { set_error("NULL input pointer"); return APG_ERR_ARG; }
  return APG_OK;
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_cartpole_learnt_param_count(void) { return kCartLearntGrads; }

int apg_cartpole_learnt_workspace_floats(int B) {
  return B <= 0 ? 0 : grid_for(B, kStepBlock) * kStepWaves * kCartLearntGrads;
}

int apg_cartpole_learnt_step_fwd(const float *state, const float *action, float dt,
                                 const ApgCartpoleLearnt *model, int B, float *next_state,
                                 apg_stream_t stream) {
  if (int e = check_step(state, action, model, B)) return e;
  if (B == 0) return APG_OK;
  if (!next_state) { set_error("next_state is NULL"); return APG_ERR_ARG; }
  hipLaunchKernelGGL(cart_learnt_step_fwd_kernel, dim3(grid_for(B, kStepBlock)),
                     dim3(kStepBlock), 0, (hipStream_t)stream, state, action, *model, dt, B,
                     next_state);
  return check_launch("cartpole_learnt_step_fwd");
}

int apg_cartpole_learnt_step_bwd(const float *state, const float *action, float dt,
                                 const ApgCartpoleLearnt *model, int B,
                                 const float *grad_next, float *grad_state,
                                 float *grad_action, float *grad_params, float *workspace,
                                 apg_stream_t stream) {
  if (int e = check_step(state, action, model, B)) return e;
  if (!grad_params) { set_error("grad_params is NULL"); return APG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {
    if (hipMemsetAsync(grad_params, 0, kCartLearntGrads * sizeof(float), st) != hipSuccess) {
      set_error("hipMemsetAsync failed");
      return APG_ERR_HIP;
    }
    return APG_OK;
  }
  if (!grad_next || !workspace) {
    set_error("grad_next / workspace is NULL");
    return APG_ERR_ARG;
  }
  const int blocks = grid_for(B, kStepBlock);
  hipLaunchKernelGGL(cart_learnt_step_bwd_kernel, dim3(blocks), dim3(kStepBlock), 0, st,
                     state, action, *model, dt, B, grad_next, grad_state, grad_action,
                     workspace);
  hipLaunchKernelGGL(cart_learnt_reduce_kernel, dim3(grid_for(kCartLearntGrads, 256)),
                     dim3(256), 0, st, workspace, blocks * kStepWaves, grad_params);
  return check_launch("cartpole_learnt_step_bwd");
}

int apg_cartpole_learnt_rollout_fwd_bwd(const float *state0, const float *actions, float dt,
                                        const ApgCartpoleLearnt *model, int B, int H,
                                        int layout, float *loss_partials, float *loss,
                                        float *grad_actions, float *grad_state0,
                                        float *states_out, apg_stream_t stream) {
  if (B < 0) { set_error("B must be >= 0 (got %d)", B); return APG_ERR_ARG; }
  if (layout != APG_LAYOUT_SOA && layout != APG_LAYOUT_AOS) {
    set_error("unknown layout %d", layout);
    return APG_ERR_ARG;
  }
  if (int e = check_model(model, true)) return e;
  if (B > 0 && (!state0 || !actions)) { set_error("NULL input pointer"); return APG_ERR_ARG; }
  if (H < 1 || H > APG_MAX_HORIZON) {
    set_error("H must be in [1, %d] (got %d)", APG_MAX_HORIZON, H);
    return APG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {
    if (loss && hipMemsetAsync(loss, 0, sizeof(float), st) != hipSuccess)
      return check_launch("memset(loss)");
    return APG_OK;
  }
  if (!loss_partials || !grad_actions) {
    set_error("loss_partials / grad_actions must not be NULL");
    return APG_ERR_ARG;
  }
  CartLearntRolloutArgs A;
  A.state0 = state0, A.actions = actions;
  A.loss_partials = loss_partials, A.grad_actions = grad_actions;
  A.grad_state0 = grad_state0, A.states_out = states_out;
  A.m = *model, A.dt = dt;
  A.B = B, A.H = H;
  const size_t lds =
      ((size_t)kCartResFloats + (size_t)H * 4 * APG_ROLLOUT_BLOCK) * sizeof(float);
  const dim3 grid(grid_for(B, APG_ROLLOUT_BLOCK)), block(APG_ROLLOUT_BLOCK);
  if (layout == APG_LAYOUT_SOA)
    hipLaunchKernelGGL(cart_learnt_rollout_kernel<APG_LAYOUT_SOA>, grid, block, lds, st, A);
  else
    hipLaunchKernelGGL(cart_learnt_rollout_kernel<APG_LAYOUT_AOS>, grid, block, lds, st, A);
  if (int e = check_launch("cartpole_learnt_rollout_fwd_bwd")) return e;
  if (loss)
    return launch_reduce_partials(loss_partials, apg_loss_partials_count(B), loss, st);
  return APG_OK;
}

}  // extern "C"
