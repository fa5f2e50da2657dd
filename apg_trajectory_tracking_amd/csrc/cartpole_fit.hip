// cartpole_fit.hip - the simulator-fit phase of the learnt cart-pole as one
// fused, capturable step: TrainBase.train_dynamics_model (scripts/train_base.py:
// 160-186) with LearntCartpoleDynamics (neural_control/dynamics/
// cartpole_dynamics.py:122-140, learnt_dynamics.py:58-98) as train dynamics, up
// to (not including) the optimizer step.
//   pred = simulate_cartpole(s, a) + W2 relu(W1 [s; a] + b1)
//   loss = sum (pred - target)^2
// and the batch-summed cotangent of all 646 parameters in one flat buffer in
// the order apg_cartpole_learnt_step_bwd publishes.  The six physical
// parameters and the residual are read from the module's own device tensors
// when the launches run, as the kernels of cartpole_learnt.hip do.
//
// Two launches behind one entry point, after quad_fit.hip (no pack launch: the
// 640 residual floats are staged into LDS as unit rows by every workgroup): the
// fit kernel (forward, target, loss, lam = 2 (pred - target), every parameter's
// cotangent summed over the WORKGROUP) and a reduction over the workgroups'
// rows (fit_rows_sum of residual_fit.h).  No float atomics: a wave sums its 64
// samples (the physical six by a shuffle tree; the weights' by lane m = hidden
// unit m looping over the wave's samples in LDS, as cart_learnt_step_bwd_kernel
// does), the four waves of a workgroup are added in wave order in LDS, the rows
// by a fixed tree: the same inputs give the same bits.  No MFMA: per sample the
// products are 5 and 4 wide, and at the batch sizes the fit runs at the step is
// launch latency, not arithmetic.
#include <stddef.h>

#include "apg_device.h"
#include "cartpole_fit_math.h"
#include "residual_fit.h"

namespace apg {
namespace {

inline int grid_for(int B, int block) { return (B + block - 1) / block; }

static_assert(kCartGW1 == APG_CARTPOLE_LEARNT_G_W1 && kCartGB1 == APG_CARTPOLE_LEARNT_G_B1 &&
                  kCartGW2 == APG_CARTPOLE_LEARNT_G_W2 &&
                  kCartLearntGrads == APG_CARTPOLE_LEARNT_GRADS,
              "apg.h publishes these offsets");
constexpr int kFitBlock = 256, kFitWaves = kFitBlock / kWave;
constexpr int kFitSample = 9;                    // z (5), lam (4) per sample
// a wave's LDS: its samples [9][64] first, its 10 weight planes [10][64] after
constexpr int kFitWaveLds = kCartResRow * kWave;
static_assert(kFitSample <= kCartResRow, "the weight planes re-use the sample planes");
static_assert(kCartResHidden == kWave, "lane m owns hidden unit m");

struct CartFitArgs {
  const float *state, *action, *target;   // target NULL: the analytic step on `eval`
  float *loss_partials, *rows;
  ApgCartpoleLearnt m;
  CartConst eval;
  float dt;
  int B;
};

template <bool EVAL>
__global__ __launch_bounds__(kFitBlock) void cartpole_fit_kernel(CartFitArgs A) {
  __shared__ float unit[kCartResFloats];
  __shared__ float smp[kFitWaves][kFitWaveLds];
  __shared__ float head[kFitWaves][kCartPhysGrads];
  for (int t = threadIdx.x; t < kCartResFloats; t += kFitBlock)
    unit[t] = cart_residual_packed(t, A.m.w1, A.m.b1, A.m.w2);
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), wl = threadIdx.x >> 6;
  const int b = blockIdx.x * kFitBlock + threadIdx.x;
  const bool live = b < A.B;
  const int bb = live ? b : A.B - 1;
  const CartLearntParams p{*A.m.max_force_mag, *A.m.masspole,   *A.m.length,
                           *A.m.friction,      *A.m.total_mass, *A.m.polemass_length};
  const CartConst c = make_learnt_const(p, A.dt);
  float s[4], tgt[4], lam[4], g[kCartPhysGrads] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  load_state<APG_LAYOUT_AOS, 4>(A.state, A.B, bb, s);
  const float a = A.action[bb];
  if constexpr (EVAL) {
#pragma unroll
    for (int i = 0; i < 4; ++i) tgt[i] = s[i];
    cart_step(tgt, a, A.eval);
  } else {
    load_state<APG_LAYOUT_AOS, 4>(A.target, A.B, bb, tgt);
  }
  float loss = cart_fit_sample(s, a, tgt, p, c, A.dt, unit, lam, g);
  // a dead lane adds nothing: zero loss, zero seed, zero cotangents
  if (!live) {
    loss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) lam[i] = 0.f;
#pragma unroll
    for (int i = 0; i < kCartPhysGrads; ++i) g[i] = 0.f;
  }
  write_wave_partial(A.loss_partials, loss, (A.B + kWave - 1) / kWave);
#pragma unroll
  for (int i = 0; i < kCartPhysGrads; ++i) {
    const float v = wave_sum(g[i]);
    if (lane == 0) head[wl][i] = v;
  }
  // the wave's samples into its LDS planes, then lane m = hidden unit m over
  // all 64 (each wave reads and writes its own planes only)
  float *mine = smp[wl];
#pragma unroll
  for (int j = 0; j < 4; ++j) mine[j * kWave + lane] = s[j];
  mine[4 * kWave + lane] = a;
#pragma unroll
  for (int o = 0; o < 4; ++o) mine[(5 + o) * kWave + lane] = lam[o];
  __syncthreads();
  float w[kCartResRow], gw[kCartResRow];
#pragma unroll
  for (int j = 0; j < kCartResRow; ++j) w[j] = unit[lane * kCartResRow + j], gw[j] = 0.f;
#pragma unroll 4
  for (int n = 0; n < kWave; ++n) {
    float zn[5], ln[4];
#pragma unroll
    for (int j = 0; j < 5; ++j) zn[j] = mine[j * kWave + n];
#pragma unroll
    for (int o = 0; o < 4; ++o) ln[o] = mine[(5 + o) * kWave + n];
    cart_residual_unit_grads(w, zn, ln, gw);
  }
  __syncthreads();   // (uniform trip count above: every wave is done reading)
#pragma unroll
  for (int j = 0; j < kCartResRow; ++j) mine[j * kWave + lane] = gw[j];
  __syncthreads();
  // the four waves in wave order -> one row per workgroup
  float *row = A.rows + (size_t)blockIdx.x * kCartFitRow;
  for (int col = threadIdx.x; col < kCartFitRow; col += kFitBlock) {
    float acc = 0.f;
    if (col < kCartFitHead) {
      if (col < kCartPhysGrads) {
        acc = head[0][col];
#pragma unroll
        for (int v = 1; v < kFitWaves; ++v) acc += head[v][col];
      }
    } else {
      acc = smp[0][col - kCartFitHead];
#pragma unroll
      for (int v = 1; v < kFitWaves; ++v) acc += smp[v][col - kCartFitHead];
    }
    row[col] = acc;
  }
}

// grad[dest(c)] = sum over the workgroups' rows of column c, fit_rows_sum of
// residual_fit.h
constexpr int kFitCols = 32, kFitSplit = 8;
__global__ __launch_bounds__(kFitCols * kFitSplit) void cartpole_fit_reduce_kernel(
    const float *__restrict__ rows, int nrows, float *__restrict__ grad) {
  __shared__ float part[kFitSplit][kFitCols];
  const int col = threadIdx.x % kFitCols, r = threadIdx.x / kFitCols;
  const int c = blockIdx.x * kFitCols + col;          // kCartFitRow = 21 x 32
  const float v = fit_rows_sum<kCartFitRow>(rows, nrows, c, col, r, part);
  if (r == 0) {
    const int dest = cart_fit_dest(c);
    if (dest >= 0) grad[dest] = v;
  }
}
static_assert(kCartFitRow % kFitCols == 0 && kFitSplit == 8,
              "whole workgroups of columns; fit_rows_sum adds eight sums");

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_cartpole_learnt_fit_workspace_floats(int B) {
  return B <= 0 ? 0 : grid_for(B, kFitBlock) * kCartFitRow;
}

int apg_cartpole_learnt_fit_fwd_bwd(const float *state, const float *action, float dt,
                                    const ApgCartpoleLearnt *model, const float *target,
                                    const ApgCartpoleParams *eval_params, int B,
                                    float *loss_partials, float *loss, float *grad,
                                    float *workspace, apg_stream_t stream) {
  if (B < 0) { set_error("B must be >= 0 (got %d)", B); return APG_ERR_ARG; }
  if (const char *e = cart_learnt_check(model, true)) {
    set_error("%s", e);
    return APG_ERR_ARG;
  }
  if ((target != nullptr) == (eval_params != nullptr)) {
    set_error("exactly one of target / eval_params must be given");
    return APG_ERR_ARG;
  }
  if (!grad) { set_error("grad is NULL"); return APG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {
    if (hipMemsetAsync(grad, 0, kCartLearntGrads * sizeof(float), st) != hipSuccess ||
        (loss && hipMemsetAsync(loss, 0, sizeof(float), st) != hipSuccess))
      return check_launch("memset(grad, loss)");
    return APG_OK;
  }
  if (!state || !action || !loss_partials || !workspace) {
    set_error("state / action / loss_partials / workspace must not be NULL");
    return APG_ERR_ARG;
  }
  CartFitArgs A;
  A.state = state, A.action = action, A.target = target;
  A.loss_partials = loss_partials, A.rows = workspace;
  A.m = *model, A.dt = dt, A.B = B;
  const int blocks = grid_for(B, kFitBlock);
  if (eval_params) {
    A.eval = make_const(*eval_params, dt);
    hipLaunchKernelGGL(cartpole_fit_kernel<true>, dim3(blocks), dim3(kFitBlock), 0, st, A);
  } else {
    A.eval = CartConst{};
    hipLaunchKernelGGL(cartpole_fit_kernel<false>, dim3(blocks), dim3(kFitBlock), 0, st, A);
  }
  if (int e = check_launch("cartpole_learnt_fit_fwd_bwd")) return e;
  if (loss)
    if (int e = launch_reduce_partials(loss_partials, apg_loss_partials_count(B), loss, st))
      return e;
  hipLaunchKernelGGL(cartpole_fit_reduce_kernel, dim3(kCartFitRow / kFitCols),
                     dim3(kFitCols * kFitSplit), 0, st, workspace, blocks, grad);
  return check_launch("cartpole_learnt_fit_reduce");
}

}  // extern "C"
