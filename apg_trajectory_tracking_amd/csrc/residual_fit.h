// residual_fit.h - the simulator-fit step (TrainBase.train_dynamics_model up to
// the optimizer) of the three learnt simulators, stated once: the fixed wing
// (wing_learnt.hip: apg_wing_learnt_fit_fwd_bwd), the quadrotor (quad_fit.hip:
// apg_quad_learnt_fit_fwd_bwd) and the cart-pole (cartpole_fit.hip:
// apg_cartpole_learnt_fit_fwd_bwd).  All three are a physics step plus a
// IN -> 64 -> OUT relu residual, fitted to a target by the summed squared error.
//
// Behind one entry point (fit_run): a pack launch where the system has one, the
// fit kernel (fit_body: forward, target, loss, lam = 2 (pred - target), every
// parameter's cotangent summed over the WORKGROUP into one partial row), the
// loss reduction, and a reduction over the workgroups' rows (fit_reduce) that
// scatters into the flat gradient and adds the regulariser where the system has
// one.  No float atomics: a wave sums its 64 samples (the row's head by a
// shuffle tree; the weights' cotangents by lane m = hidden unit m looping over
// the wave's samples in LDS), the four waves of a workgroup are added in wave
// order in LDS, the rows by a fixed tree: the same inputs give the same bits.
// No MFMA: per sample the products are at most 16 and 12 wide and gated per
// sample and unit by the relu mask, and at the batch sizes the fit runs at the
// step is launch latency, not arithmetic.
//
// What differs per system is a traits type T next to its per-sample arithmetic
// (WingFit in wing_learnt_math.h, QuadFit in quad_fit_math.h, CartFit in
// cartpole_fit_math.h), read by the kernels and by the host twins
// (cpu_twins.hip: fit_host):
//   S, A, IN, OUT        widths: state, action, the residual's input and output
//   RES_ROW, RW2, RB1    a unit's packed row W1[m][0..IN) at 0, W2[0..OUT)[m]
//                        at RW2, b1[m] at RB1
//   UNIT, UW2, UB1       its IN + OUT + 1 cotangents: dW1 at 0, dW2 at UW2, db1
//                        at UB1 - plane j of a partial row
//   HEAD, USED, ROW      a partial row: [USED head sums, zeros to HEAD | UNIT
//                        planes of 64]
//   GRADS, dest(c), value(c, v, scale)   the flat gradient: where element c of
//                        a row lands (-1: padding) and what is written there
//   REG, G_W1 .. G_B2    whether the four-norm regulariser exists, and where
//                        the residual's tensors start in the flat gradient
//   NORMS_AT, ROWS_AT    the workspace: [pack | norms, padded to 16 | rows]
//   Eval, Scale          the analytic target step's constants; value()'s
//   sample(m, s, a, tgt, eval, lam, z, hd)   one sample on the model m (device:
//                        T::model(A); host: the twin's): tgt from the analytic
//                        step where `eval` is given, the loss (returned), lam,
//                        the residual's input z and the head's USED entries
// and, for the device alone: Args (state, action, target, loss_partials, rows,
// eval, B and the system's own), model(A) (the cart-pole stages its unit rows
// into LDS there), unit_row(A, m, lane, w) (how a lane fetches its unit's row)
// and UNROLL (of the loop over a wave's samples).
#pragma once
#include "apg_device.h"

namespace apg {
namespace {

constexpr int kResHidden = 64;
constexpr int kResFitUnit = 29;   // a 16 -> 64 -> 12 unit's cotangents

// gw += one hidden unit's IN + OUT + 1 cotangents for one sample (z, lam).
// w = the unit's packed row: W1[m][0..IN) at 0, W2[0..OUT)[m] at W2, b1[m] at
// B1; gw: dW1[m][j] at j, dW2[o][m] at GW2 + o, db1[m] at GB1 (relu'(0) = 0, as
// torch's threshold backward).  The wing and the quadrotor keep dW1, dW2, db1
// whatever the row's order; the cart-pole keeps the row's own order.
template <int IN, int OUT, int W2, int B1, int GW2, int GB1>
__host__ __device__ __forceinline__ void residual_unit_grads(const float *w,
                                                             const float (&z)[IN],
                                                             const float (&lam)[OUT],
                                                             float (&gw)[IN + OUT + 1]) {
  float h = w[B1];
#pragma unroll
  for (int j = 0; j < IN; ++j) h = fmaf(w[j], z[j], h);
  float dh = 0.f;
#pragma unroll
  for (int o = 0; o < OUT; ++o) dh = fmaf(w[W2 + o], lam[o], dh);
  dh = h > 0.f ? dh : 0.f;
  h = fmaxf(h, 0.f);
#pragma unroll
  for (int j = 0; j < IN; ++j) gw[j] = fmaf(dh, z[j], gw[j]);
#pragma unroll
  for (int o = 0; o < OUT; ++o) gw[GW2 + o] = fmaf(lam[o], h, gw[GW2 + o]);
  gw[GB1] += dh;
}

// the four tensors of a 16 -> 64 -> 12 residual, for the regulariser
struct ResidualTensors {
  const float *w1, *b1, *w2, *b2;
};

// the regulariser's gradient l2_lambda t / |t| (0 where |t| = 0, as torch's
// norm backward) for element `dest` of a flat gradient whose residual tensors
// start at GW1 < GB1 < GW2 < GB2; norms = |W2|, |b2|, |W1|, |b1| (the order of
// _residual_weight_norm)
template <int GW1, int GB1, int GW2, int GB2>
__host__ __device__ __forceinline__ float residual_l2_grad(int dest, float l2_lambda,
                                                           const ResidualTensors &t,
                                                           const float *norms) {
  if (dest < GW1) return 0.f;
  float v, n;
  if (dest < GB1) v = t.w1[dest - GW1], n = norms[2];
  else if (dest < GW2) v = t.b1[dest - GB1], n = norms[3];
  else if (dest < GB2) v = t.w2[dest - GW2], n = norms[0];
  else v = t.b2[dest - GB2], n = norms[1];
  return n > 0.f ? l2_lambda * (v / n) : 0.f;
}

// a system without a regulariser, or whose summed row elements are written as
// they are
struct FitNoScale {};

// grad[dest(c)] for the summed element c of a partial row, the regulariser's
// gradient included; the kernels' reduction and the twins share it
template <class T>
__host__ __device__ __forceinline__ void fit_scatter(int c, float v,
                                                     const typename T::Scale &scale,
                                                     const ResidualTensors &t, const float *norms,
                                                     float l2_lambda, float *grad) {
  const int dest = T::dest(c);
  if (dest < 0) return;
  float g = T::value(c, v, scale);
  if constexpr (T::REG)
    g += l2_lambda > 0.f
             ? residual_l2_grad<T::G_W1, T::G_B1, T::G_W2, T::G_B2>(dest, l2_lambda, t, norms)
             : 0.f;
  grad[dest] = g;
}

// the penalty l2_lambda (|W2| + |b2| + |W1| + |b1|)
__host__ __device__ __forceinline__ float fit_penalty(float l2_lambda, const float *n) {
  return l2_lambda * (((n[0] + n[1]) + n[2]) + n[3]);
}

#if defined(__HIPCC__)
// |W2|, |b2|, |W1|, |b1| (2-norms) by one workgroup of 256: per-thread strided
// sums, then a fixed tree; thread q < 4 writes norms[q]
__device__ __forceinline__ void residual_norms(const float *w1, const float *b1,
                                               const float *w2, const float *b2,
                                               float (&part)[4][256], float *norms) {
  const float *tens[4] = {w2, b2, w1, b1};
  const int count[4] = {12 * kResHidden, 12, kResHidden * 16, kResHidden};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float acc = 0.f;
    for (int t = threadIdx.x; t < count[q]; t += 256) acc = fmaf(tens[q][t], tens[q][t], acc);
    part[q][threadIdx.x] = acc;
  }
  for (int half = 128; half >= 1; half >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < half)
#pragma unroll
      for (int q = 0; q < 4; ++q) part[q][threadIdx.x] += part[q][threadIdx.x + half];
  }
  if (threadIdx.x < 4) norms[threadIdx.x] = sqrtf(part[threadIdx.x][0]);
}

// Element c of the sum over `nrows` partial rows of ROW floats, by the 8
// threads (r = 0..7) that share column `col` of a workgroup: thread r adds rows
// r, r + 8, ... in order, then a fixed tree over the 8 sums.  The value is
// returned to thread r == 0 (the others get 0).
template <int ROW, int COLS>
__device__ __forceinline__ float fit_rows_sum(const float *__restrict__ rows, int nrows, int c,
                                              int col, int r, float (&part)[8][COLS]) {
  float acc = 0.f;
#pragma unroll 4
  for (int i = r; i < nrows; i += 8) acc += rows[(size_t)i * ROW + c];
  part[r][col] = acc;
  __syncthreads();
  if (r != 0) return 0.f;
  return ((part[0][col] + part[1][col]) + (part[2][col] + part[3][col])) +
         ((part[4][col] + part[5][col]) + (part[6][col] + part[7][col]));
}

constexpr int kFitBlock = 256, kFitWaves = kFitBlock / kWave;   // the fit kernel
constexpr int kFitCols = 32, kFitSplit = 8;                     // the reduction
static_assert(kResHidden == kWave, "lane m owns hidden unit m");
static_assert(kFitSplit == 8, "fit_rows_sum adds eight sums");

inline int fit_blocks(int B) { return (B + kFitBlock - 1) / kFitBlock; }

template <class T>
int fit_workspace_floats(int B) {
  return B <= 0 ? 0 : T::ROWS_AT + fit_blocks(B) * T::ROW;
}

// The fit kernel's body: one lane = one sample, one partial row per workgroup.
// (The LDS is named here, not handed in: its address is then a constant to the
// compiler.)
template <class T, bool EVAL>
__device__ __forceinline__ void fit_body(const typename T::Args &A) {
  static_assert(T::UNIT == T::IN + T::OUT + 1 && T::USED <= T::HEAD &&
                    T::HEAD - T::USED <= kWave && T::ROW == T::HEAD + T::UNIT * kResHidden &&
                    T::ROW % kFitCols == 0,
                "row layout; the reduction takes whole workgroups of columns");
  // a wave's LDS: its samples [IN + OUT][64] first, its UNIT weight planes
  // [UNIT][64] after (the weight planes re-use the sample planes)
  __shared__ float smp[kFitWaves][T::UNIT * kWave];
  __shared__ float head[kFitWaves][T::HEAD];
  const auto m = T::model(A);
  const int lane = threadIdx.x & (kWave - 1), wl = threadIdx.x >> 6;
  const int b = blockIdx.x * kFitBlock + threadIdx.x;
  const bool live = b < A.B;
  const int bb = live ? b : A.B - 1;
  float s[T::S], a[T::A], tgt[T::S], lam[T::OUT], z[T::IN], hd[T::USED];
  load_state<APG_LAYOUT_AOS, T::S>(A.state, A.B, bb, s);
  load_state<APG_LAYOUT_AOS, T::A>(A.action, A.B, bb, a);
  if constexpr (!EVAL) load_state<APG_LAYOUT_AOS, T::S>(A.target, A.B, bb, tgt);
  float loss = T::sample(m, s, a, tgt, EVAL ? &A.eval : nullptr, lam, z, hd);
  // a dead lane adds nothing: zero loss, zero seed, zero cotangents
  if (!live) {
    loss = 0.f;
#pragma unroll
    for (int i = 0; i < T::OUT; ++i) lam[i] = 0.f;
#pragma unroll
    for (int i = 0; i < T::USED; ++i) hd[i] = 0.f;
  }
  write_wave_partial(A.loss_partials, loss, (A.B + kWave - 1) / kWave);
#pragma unroll
  for (int i = 0; i < T::USED; ++i) {
    const float v = wave_sum(hd[i]);
    if (lane == 0) head[wl][i] = v;
  }
  if (lane < T::HEAD - T::USED) head[wl][T::USED + lane] = 0.f;
  // the wave's samples into its LDS planes, then lane m = hidden unit m over
  // all 64 (each wave reads and writes its own planes only)
  float *mine = smp[wl];
#pragma unroll
  for (int j = 0; j < T::IN; ++j) mine[j * kWave + lane] = z[j];
#pragma unroll
  for (int o = 0; o < T::OUT; ++o) mine[(T::IN + o) * kWave + lane] = lam[o];
  __syncthreads();
  float w[T::RES_ROW], gw[T::UNIT];
  T::unit_row(A, m, lane, w);
#pragma unroll
  for (int j = 0; j < T::UNIT; ++j) gw[j] = 0.f;
#pragma unroll T::UNROLL
  for (int n = 0; n < kWave; ++n) {
    float zn[T::IN], ln[T::OUT];
#pragma unroll
    for (int j = 0; j < T::IN; ++j) zn[j] = mine[j * kWave + n];
#pragma unroll
    for (int o = 0; o < T::OUT; ++o) ln[o] = mine[(T::IN + o) * kWave + n];
    residual_unit_grads<T::IN, T::OUT, T::RW2, T::RB1, T::UW2, T::UB1>(w, zn, ln, gw);
  }
  __syncthreads();   // (uniform trip count above: every wave is done reading)
#pragma unroll
  for (int j = 0; j < T::UNIT; ++j) mine[j * kWave + lane] = gw[j];
  __syncthreads();
  // the four waves in wave order -> one row per workgroup
  float *row = A.rows + (size_t)blockIdx.x * T::ROW;
  for (int c = threadIdx.x; c < T::ROW; c += kFitBlock) {
    float acc;
    if (c < T::HEAD) {
      acc = head[0][c];
#pragma unroll
      for (int v = 1; v < kFitWaves; ++v) acc += head[v][c];
    } else {
      acc = smp[0][c - T::HEAD];
#pragma unroll
      for (int v = 1; v < kFitWaves; ++v) acc += smp[v][c - T::HEAD];
    }
    row[c] = acc;
  }
}

// The reduction's body, T::ROW / kFitCols workgroups of kFitCols x kFitSplit:
// grad[dest(c)] = value(sum over the workgroups' rows of element c) (+ the
// regulariser's gradient), fit_rows_sum then fit_scatter.  Thread 0 of
// workgroup 0 adds the penalty to the loss, which the loss reduction in front
// of this launch has written.
template <class T>
__device__ __forceinline__ void fit_reduce(const float *__restrict__ rows, int nrows,
                                           const typename T::Scale &scale,
                                           const ResidualTensors &t, const float *norms,
                                           float l2_lambda, float *__restrict__ grad,
                                           float *__restrict__ loss) {
  __shared__ float part[kFitSplit][kFitCols];
  const int col = threadIdx.x % kFitCols, r = threadIdx.x / kFitCols;
  const int c = blockIdx.x * kFitCols + col;
  const float v = fit_rows_sum<T::ROW>(rows, nrows, c, col, r, part);
  if (r == 0) fit_scatter<T>(c, v, scale, t, norms, l2_lambda, grad);
  if constexpr (T::REG)
    if (l2_lambda > 0.f && loss && blockIdx.x == 0 && threadIdx.x == 0)
      loss[0] += fit_penalty(l2_lambda, norms);
}

// What an entry point was called with.  model_error: the outcome of its own
// model and pointer checks (NULL: fine), reported where they stood.
struct FitCall {
  const float *state, *action, *target;
  bool eval;                      // eval_params given
  float l2_lambda;
  int B;
  float *loss_partials, *loss, *grad, *workspace;
  hipStream_t st;
  const char *model_error;
};

// The host side of an entry point: the common checks, the empty batch, then the
// launches - prepare(A) (the system's own fields of A, its pack launch), the
// fit kernel, the loss reduction, reduce(blocks) (the system's reduce launch).
// fit_name / reduce_name: what a failed launch is reported as.
template <class T, class Prepare, class Reduce>
int fit_run(const FitCall &c, const char *fit_name, const char *reduce_name,
            void (*eval_kernel)(typename T::Args), void (*target_kernel)(typename T::Args),
            Prepare &&prepare, Reduce &&reduce) {
  if (c.B < 0) { set_error("B must be >= 0 (got %d)", c.B); return APG_ERR_ARG; }
  if (c.model_error) { set_error("%s", c.model_error); return APG_ERR_ARG; }
  if ((c.target != nullptr) == c.eval) {
    set_error("exactly one of target / eval_params must be given");
    return APG_ERR_ARG;
  }
  if (!(c.l2_lambda >= 0.f)) { set_error("l2_lambda must be >= 0"); return APG_ERR_ARG; }
  if (!c.grad) { set_error("grad is NULL"); return APG_ERR_ARG; }
  if (c.B == 0) {
    if (hipMemsetAsync(c.grad, 0, T::GRADS * sizeof(float), c.st) != hipSuccess ||
        (c.loss && hipMemsetAsync(c.loss, 0, sizeof(float), c.st) != hipSuccess))
      return check_launch("memset(grad, loss)");
    return APG_OK;
  }
  if (!c.state || !c.action || !c.loss_partials || !c.workspace) {
    set_error("state / action / loss_partials / workspace must not be NULL");
    return APG_ERR_ARG;
  }
  typename T::Args A;
  A.state = c.state, A.action = c.action, A.target = c.target;
  A.loss_partials = c.loss_partials, A.rows = c.workspace + T::ROWS_AT;
  A.B = c.B;
  prepare(A);
  const int blocks = fit_blocks(c.B);
  hipLaunchKernelGGL(c.eval ? eval_kernel : target_kernel, dim3(blocks), dim3(kFitBlock), 0,
                     c.st, A);
  if (int e = check_launch(fit_name)) return e;
  if (c.loss)
    if (int e = launch_reduce_partials(c.loss_partials, apg_loss_partials_count(c.B), c.loss,
                                       c.st))
      return e;
  reduce(blocks);
  return check_launch(reduce_name);
}
#endif

}  // namespace
}  // namespace apg
