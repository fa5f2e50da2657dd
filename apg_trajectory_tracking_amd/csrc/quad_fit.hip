// quad_fit.hip - the simulator-fit phase of the learnt quadrotor as one fused,
// capturable step: TrainBase.train_dynamics_model (scripts/train_base.py:
// 160-186) with LearntDynamics (neural_control/dynamics/quad_dynamics_trained.py:
// 10-69) as train dynamics, up to (not including) the optimizer step.
//   a'   = linear_at a
//   pred = quad_step(s, a'; params) + W2 relu(W1 [s; a'] + b1) + b2
//   loss = sum (pred - target)^2 + l2_lambda (|W2| + |b2| + |W1| + |b1|)
// and the batch-summed cotangent of all 1 891 parameters in one flat buffer in
// the order of LearntDynamics.parameters().  The physical constants are those of
// construction time (the reference's torch.diag copies, :48-50) and arrive as
// kernel arguments; kinv and inertia get the closed forms the module documents,
// evaluated at those values, and the mass exactly 0.
//
// Three launches behind one entry point, after wing_learnt.hip's fit: pack (the
// residual's unit rows, linear_at and the four weight norms from the live
// tensors), the fit kernel (forward, target, loss, the step's adjoint, every
// parameter's cotangent summed over the WORKGROUP) and a reduction over the
// workgroups' rows that also adds the regulariser (residual_fit.h).  No float
// atomics: a wave sums its 64 samples (the head - linear_at, kinv, sum lam_w',
// db2 - by a shuffle tree; the weights' by lane m = hidden unit m looping over
// the wave's samples in LDS), the four waves of a workgroup are added in wave
// order in LDS, the rows by a fixed tree: the same inputs give the same bits.
// No MFMA: per sample the products are 16 and 12 wide (W1 x, W2^T lam, and two
// outer products gated per sample and unit by the relu mask), and at the batch
// sizes the fit runs at the step is launch latency, not arithmetic.
#include <stddef.h>

#include "apg_device.h"
#include "quad_fit_math.h"

namespace apg {
namespace {

inline int grid_for(int B, int block) { return (B + block - 1) / block; }

static_assert(kQuadFitGLin == APG_QUAD_FIT_G_LINEAR_AT && kQuadFitGMass == APG_QUAD_FIT_G_MASS &&
                  kQuadFitGInertia == APG_QUAD_FIT_G_INERTIA &&
                  kQuadFitGKinv == APG_QUAD_FIT_G_KINV && kQuadFitGW1 == APG_QUAD_FIT_G_W1 &&
                  kQuadFitGB1 == APG_QUAD_FIT_G_B1 && kQuadFitGW2 == APG_QUAD_FIT_G_W2 &&
                  kQuadFitGB2 == APG_QUAD_FIT_G_B2 && kQuadFitGrads == APG_QUAD_FIT_GRADS,
              "apg.h publishes these offsets");
constexpr int kFitBlock = 256, kFitWaves = kFitBlock / kWave;
constexpr int kFitSample = 28;                    // x (16), lam (12) per sample
// a wave's LDS: its samples [28][64] first, its 29 weight planes [29][64] after
constexpr int kFitWaveLds = kResFitUnit * kWave;
static_assert(kFitSample <= kResFitUnit, "the weight planes re-use the sample planes");
// workspace: [pack | norms (4), padded to 16 | rows]
constexpr int kFitNorms = kQuadPackFloats, kFitRows = kFitNorms + 16;

// the packed model of quad_fit_math.h plus |W2|, |b2|, |W1|, |b1|
__global__ __launch_bounds__(256) void quad_learnt_fit_pack_kernel(ApgLearntResidual m,
                                                                   float *__restrict__ ws) {
  __shared__ float part[4][256];
  for (int t = threadIdx.x; t < kQuadPackFloats; t += blockDim.x) ws[t] = quad_fit_packed(t, m);
  residual_norms(m.w1, m.b1, m.w2, m.b2, part, ws + kFitNorms);
}

struct QuadFitArgs {
  const float *state, *action, *target;   // target NULL: the analytic step on `eval`
  const float *ws;                        // the pack
  float *loss_partials, *rows;
  QuadConst c, eval;
  int B;
};

template <bool EVAL>
__global__ __launch_bounds__(kFitBlock) void quad_learnt_fit_kernel(QuadFitArgs A) {
  __shared__ float smp[kFitWaves][kFitWaveLds];
  __shared__ float head[kFitWaves][kQuadFitHead];
  typedef __attribute__((address_space(4))) const float *cfloat_ptr;
  cfloat_ptr pack = (cfloat_ptr)A.ws;
  const int lane = threadIdx.x & (kWave - 1), wl = threadIdx.x >> 6;
  const int b = blockIdx.x * kFitBlock + threadIdx.x;
  const bool live = b < A.B;
  const int bb = live ? b : A.B - 1;
  float s[12], a[4], tgt[12], lam[12], x[16], hd[kQuadFitHUsed];
  load_state<APG_LAYOUT_AOS, 12>(A.state, A.B, bb, s);
  load_state<APG_LAYOUT_AOS, 4>(A.action, A.B, bb, a);
  const Trig t = make_trig(&s[3]);
  if constexpr (EVAL) {
#pragma unroll
    for (int i = 0; i < 12; ++i) tgt[i] = s[i];
    quad_step(tgt, a, A.eval, t);        // the eval dynamics takes the RAW action
  } else {
    load_state<APG_LAYOUT_AOS, 12>(A.target, A.B, bb, tgt);
  }
  float loss = quad_learnt_fit_sample(s, a, tgt, A.c, t, pack, lam, x, hd);
  // a dead lane adds nothing: zero seed, zero cotangents
  if (!live) {
    loss = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) lam[i] = 0.f;
#pragma unroll
    for (int i = 0; i < kQuadFitHUsed; ++i) hd[i] = 0.f;
  }
  write_wave_partial(A.loss_partials, loss, (A.B + kWave - 1) / kWave);
#pragma unroll
  for (int i = 0; i < kQuadFitHUsed; ++i) {
    const float v = wave_sum(hd[i]);
    if (lane == 0) head[wl][i] = v;
  }
  if (lane < kQuadFitHead - kQuadFitHUsed) head[wl][kQuadFitHUsed + lane] = 0.f;
  // the wave's samples into its LDS planes, then lane m = hidden unit m over
  // all 64 (each wave reads and writes its own planes only)
  float *mine = smp[wl];
#pragma unroll
  for (int j = 0; j < 16; ++j) mine[j * kWave + lane] = x[j];
#pragma unroll
  for (int o = 0; o < 12; ++o) mine[(16 + o) * kWave + lane] = lam[o];
  __syncthreads();
  float w[kQuadResRow], gw[kResFitUnit];
#pragma unroll
  for (int j = 0; j < kQuadResRow; ++j) w[j] = A.ws[lane * kQuadResRow + j];
#pragma unroll
  for (int j = 0; j < kResFitUnit; ++j) gw[j] = 0.f;
#pragma unroll 2
  for (int n = 0; n < kWave; ++n) {
    float xn[16], ln[12];
#pragma unroll
    for (int j = 0; j < 16; ++j) xn[j] = mine[j * kWave + n];
#pragma unroll
    for (int o = 0; o < 12; ++o) ln[o] = mine[(16 + o) * kWave + n];
    residual_unit_grads<kQuadResW2, kQuadResB1>(w, xn, ln, gw);
  }
  __syncthreads();   // (uniform trip count above: every wave is done reading)
#pragma unroll
  for (int j = 0; j < kResFitUnit; ++j) mine[j * kWave + lane] = gw[j];
  __syncthreads();
  // the four waves in wave order -> one row per workgroup
  float *row = A.rows + (size_t)blockIdx.x * kQuadFitRow;
  for (int c = threadIdx.x; c < kQuadFitRow; c += kFitBlock) {
    float acc;
    if (c < kQuadFitHead) {
      acc = head[0][c];
#pragma unroll
      for (int v = 1; v < kFitWaves; ++v) acc += head[v][c];
    } else {
      acc = smp[0][c - kQuadFitHead];
#pragma unroll
      for (int v = 1; v < kFitWaves; ++v) acc += smp[v][c - kQuadFitHead];
    }
    row[c] = acc;
  }
}

// grad[dest(c)] = sum over the workgroups' rows of element c (+ the
// regulariser's gradient), fit_rows_sum of residual_fit.h; the inertia elements
// are scaled into dL/dJ, the mass slot is written as 0.  Thread 0 of workgroup
// 0 adds the penalty to the loss, which the loss reduction in front of this
// launch has written.
constexpr int kFitCols = 32, kFitSplit = 8;
__global__ __launch_bounds__(kFitCols * kFitSplit) void quad_learnt_fit_reduce_kernel(
    const float *__restrict__ ws, int nrows, ApgLearntResidual m, QuadFitInertia q,
    float l2_lambda, float *__restrict__ grad, float *__restrict__ loss) {
  __shared__ float part[kFitSplit][kFitCols];
  const int col = threadIdx.x % kFitCols, r = threadIdx.x / kFitCols;
  const int c = blockIdx.x * kFitCols + col;          // kQuadFitRow = 60 x 32
  const float v = fit_rows_sum<kQuadFitRow>(ws + kFitRows, nrows, c, col, r, part);
  if (r == 0) {
    const int dest = quad_fit_dest(c);
    if (dest >= 0) {
      float reg = 0.f;
      if (l2_lambda > 0.f)
        reg = residual_l2_grad<kQuadFitGW1, kQuadFitGB1, kQuadFitGW2, kQuadFitGB2>(
            dest, l2_lambda, m.w1, m.b1, m.w2, m.b2, ws + kFitNorms);
      grad[dest] = quad_fit_value(c, v, q) + reg;
    }
  }
  if (l2_lambda > 0.f && loss && blockIdx.x == 0 && threadIdx.x == 0) {
    const float *n = ws + kFitNorms;
    loss[0] += l2_lambda * (((n[0] + n[1]) + n[2]) + n[3]);
  }
}
static_assert(kQuadFitRow % kFitCols == 0 && kFitSplit == 8,
              "whole workgroups of columns; fit_rows_sum adds eight sums");

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_quad_learnt_fit_grad_count(void) { return kQuadFitGrads; }

int apg_quad_learnt_fit_workspace_floats(int B) {
  return B <= 0 ? 0 : kFitRows + grid_for(B, kFitBlock) * kQuadFitRow;
}

int apg_quad_learnt_fit_fwd_bwd(const float *state, const float *action, float dt,
                                const ApgQuadParams *params, const ApgLearntResidual *model,
                                const float *target, const ApgQuadParams *eval_params,
                                float l2_lambda, int B, float *loss_partials, float *loss,
                                float *grad, float *workspace, apg_stream_t stream) {
  if (B < 0) { set_error("B must be >= 0 (got %d)", B); return APG_ERR_ARG; }
  if (!params) { set_error("params is NULL"); return APG_ERR_ARG; }
  if (!model || !model->linear_at || !model->w1 || !model->b1 || !model->w2 || !model->b2) {
    set_error("model or one of its pointers is NULL");
    return APG_ERR_ARG;
  }
  if ((target != nullptr) == (eval_params != nullptr)) {
    set_error("exactly one of target / eval_params must be given");
    return APG_ERR_ARG;
  }
  if (!(l2_lambda >= 0.f)) { set_error("l2_lambda must be >= 0"); return APG_ERR_ARG; }
  if (!grad) { set_error("grad is NULL"); return APG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {
    if (hipMemsetAsync(grad, 0, kQuadFitGrads * sizeof(float), st) != hipSuccess ||
        (loss && hipMemsetAsync(loss, 0, sizeof(float), st) != hipSuccess))
      return check_launch("memset(grad, loss)");
    return APG_OK;
  }
  if (!state || !action || !loss_partials || !workspace) {
    set_error("state / action / loss_partials / workspace must not be NULL");
    return APG_ERR_ARG;
  }
  hipLaunchKernelGGL(quad_learnt_fit_pack_kernel, dim3(1), dim3(256), 0, st, *model, workspace);
  QuadFitArgs A;
  A.state = state, A.action = action, A.target = target;
  A.ws = workspace, A.loss_partials = loss_partials, A.rows = workspace + kFitRows;
  A.c = make_const(*params, dt);
  A.B = B;
  const int blocks = grid_for(B, kFitBlock);
  if (eval_params) {
    A.eval = make_const(*eval_params, dt);
    hipLaunchKernelGGL(quad_learnt_fit_kernel<true>, dim3(blocks), dim3(kFitBlock), 0, st, A);
  } else {
    A.eval = QuadConst{};
    hipLaunchKernelGGL(quad_learnt_fit_kernel<false>, dim3(blocks), dim3(kFitBlock), 0, st, A);
  }
  if (int e = check_launch("quad_learnt_fit_fwd_bwd")) return e;
  if (loss)
    if (int e = launch_reduce_partials(loss_partials, apg_loss_partials_count(B), loss, st))
      return e;
  hipLaunchKernelGGL(quad_learnt_fit_reduce_kernel, dim3(kQuadFitRow / kFitCols),
                     dim3(kFitCols * kFitSplit), 0, st, workspace, blocks, *model,
                     make_fit_inertia(*params, dt), l2_lambda, grad, loss);
  return check_launch("quad_learnt_fit_reduce");
}

}  // extern "C"
