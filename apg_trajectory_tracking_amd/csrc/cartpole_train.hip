// cartpole_train.hip - the controller step of the cart-pole as one fused,
// capturable step: the controller branch of TrainCartpole.run_epoch
// (scripts/train_cartpole.py:127-155) with simple_model.Net(4, H)
// (neural_control/models/simple_model.py:9-28) as policy - policy forward,
// make_reference + H steps + cartpole_loss_mpc (cartpole_rollout_math.h), the
// reverse sweep, the cotangent chain back through the five tanh layers, every
// parameter's gradient summed over the batch and, optionally, momentum SGD.
//
// Plain fp32, no MFMA ("cart-pole controller step"): the step is
// launch latency at the batch sizes it runs at, and fp32 FMAs in one fixed
// order are what the host twin can restate exactly.  A workgroup of 256 takes
// CHUNKS of 64 samples (chunk = blockIdx.x, += gridDim.x).  The activations of
// a chunk sit in LDS as [unit][sample] rows of 65 floats (the pad makes the
// row-wise reads of the weight gradient conflict-free, cdna_hip_programming.md
// §2).  Forward and transposed products: lane = sample, wave = a quarter of the
// layer's units, the weights wave-uniform loads of the live parameters.  The
// rollout: wave 0, lane = sample, its stash behind the activations.  Cotangents
// overwrite the activations they belong to.  Weight gradients: lane = unit,
// each thread owns up to 16 inputs of its unit and adds the chunk's samples in
// sample order into registers that live across the chunks.
// One row per workgroup (the flat gradient's own layout), then a fixed tree
// over the rows (cart_train_reduce_kernel), which also sums the loss partials
// and applies the update; with one workgroup (B <= 64) the first kernel does
// all of that itself and the second launch is not made.  No float atomics.
// The same body serves the step through LearntCartpoleDynamics
// (cartpole_learnt_policy_kernel): only the rollout's two step functions differ.
#include <stddef.h>

#include "apg_device.h"
#include "cartpole_learnt_stage.h"
#include "cartpole_math.h"
#include "cartpole_train_math.h"

namespace apg {
namespace {

static_assert(kCptGW0 == APG_CARTPOLE_POLICY_G_W0 && kCptGB0 == APG_CARTPOLE_POLICY_G_B0 &&
                  kCptGW1 == APG_CARTPOLE_POLICY_G_W1 && kCptGB1 == APG_CARTPOLE_POLICY_G_B1 &&
                  kCptGW2 == APG_CARTPOLE_POLICY_G_W2 && kCptGB2 == APG_CARTPOLE_POLICY_G_B2 &&
                  kCptGW3 == APG_CARTPOLE_POLICY_G_W3 && kCptGB3 == APG_CARTPOLE_POLICY_G_B3 &&
                  kCptGWout == APG_CARTPOLE_POLICY_G_WOUT,
              "apg.h publishes these offsets");

constexpr int kTrBlock = 256, kTrWaves = kTrBlock / kWave;
constexpr int kTrChunk = kWave;         // samples per chunk: one loss partial
constexpr int kTrLd = kTrChunk + 1;     // an activation row
constexpr int kTrMaxGrid = 256;         // workgroups = rows of the second stage
// activation rows of a chunk: x, h0 .. h3, then H rows of actions
constexpr int rX = 0, rH0 = rX + kCptIn, rH1 = rH0 + kCptH0, rH2 = rH1 + kCptH1;
constexpr int rH3 = rH2 + kCptH2, rOut = rH3 + kCptH3;
static_assert(rOut == 196, "LDS map");

inline int train_chunks(int B) { return (B + kTrChunk - 1) / kTrChunk; }
inline int train_grid(int B) {
  const int n = train_chunks(B);
  return n < kTrMaxGrid ? n : kTrMaxGrid;
}
__host__ __device__ inline size_t train_lds_floats(int H) {
  return (size_t)(rOut + H) * kTrLd + (size_t)H * 4 * kTrChunk;
}

struct CartTrainOut {
  ApgCartpolePolicyGrads grads, param, mom;
  double lr, momentum;
  float *loss;
  int H, update;
};

struct CartTrainArgs {
  const float *in_state, *state0;
  ApgCartpolePolicy p;
  float *loss_partials, *actions_out, *rows;
  CartTrainOut out;
  CartConst c;
  int B, H;
};

__device__ __forceinline__ float *cpt_tensor(const ApgCartpolePolicyGrads &g, int q) {
  float *p = g.w0;
  p = q == 1 ? g.b0 : p;
  p = q == 2 ? g.w1 : p;
  p = q == 3 ? g.b1 : p;
  p = q == 4 ? g.w2 : p;
  p = q == 5 ? g.b2 : p;
  p = q == 6 ? g.w3 : p;
  p = q == 7 ? g.b3 : p;
  p = q == 8 ? g.w_out : p;
  p = q == 9 ? g.b_out : p;
  return p;
}

// the last stage of element c of the flat gradient, by the thread that holds
// its final sum v: the gradient into its tensor and, with an update, momentum
// SGD on the parameter and its buffer
__device__ __forceinline__ void train_finish(const CartTrainOut &O, int c, float v) {
  int q, off;
  cpt_locate(c, O.H, q, off);
  cpt_tensor(O.grads, q)[off] = v;
  if (O.update) {
    float *pp = cpt_tensor(O.param, q) + off, *pm = cpt_tensor(O.mom, q) + off;
    float p = *pp, buf = *pm;
    cpt_sgd(v, O.lr, O.momentum, p, buf);
    *pm = buf;
    *pp = p;
  }
}

// y[u][lane] = tanh(b[u] + sum_j W[u][j] x[j][lane]) for the wave's N / 4 units
template <int N, int K>
__device__ __forceinline__ void layer_fwd(const float *__restrict__ W,
                                          const float *__restrict__ b, const float *x,
                                          float *y, int wave, int lane) {
  constexpr int U = N / kTrWaves;
  const int u0 = wave * U;
  float z[U];
#pragma unroll
  for (int u = 0; u < U; ++u) z[u] = b[u0 + u];
  cpt_dense<U>(
      z, K, [&](int u, int j) { return W[(u0 + u) * K + j]; },
      [&](int j) { return x[j * kTrLd + lane]; });
#pragma unroll
  for (int u = 0; u < U; ++u) y[(u0 + u) * kTrLd + lane] = tanhf(z[u]);
}

// acc[jj] = sum over m < N of W[m][j0 + jj] dz[m][lane] for the wave's K / 4
// inputs (the cotangent of the layer's input, before its tanh)
template <int K>
__device__ __forceinline__ void layer_dx(float (&acc)[K / kTrWaves], int N,
                                         const float *__restrict__ W, const float *dz,
                                         int wave, int lane) {
  constexpr int J = K / kTrWaves;
  const int j0 = wave * J;
#pragma unroll
  for (int jj = 0; jj < J; ++jj) acc[jj] = 0.f;
  cpt_dense<J>(
      acc, N, [&](int jj, int m) { return W[m * K + j0 + jj]; },
      [&](int m) { return dz[m * kTrLd + lane]; });
}

// dz_prev = acc (1 - y^2) over the activations y it belongs to
template <int J>
__device__ __forceinline__ void layer_dz_store(const float (&acc)[J], float *y, int wave,
                                               int lane) {
#pragma unroll
  for (int jj = 0; jj < J; ++jj) {
    float *at = y + (wave * J + jj) * kTrLd + lane;
    *at = cpt_dtanh(acc[jj], *at);
  }
}

// the chunk's samples, in sample order, into the cotangents of unit m's
// weights on inputs j0 .. j0 + KP - 1 (and its bias)
template <int KP>
__device__ __forceinline__ void layer_wgrad(float (&gw)[KP], float &gb, const float *dz_m,
                                            const float *x_j0) {
#pragma unroll 4
  for (int s = 0; s < kTrChunk; ++s)
    cpt_wgrad<KP>(gw, gb, dz_m[s], [&](int jj) { return x_j0[jj * kTrLd + s]; });
}

// The step, whatever simulates: `step(x, a)` advances a state in place,
// `adjoint(lam, pre, a)` turns dL/dnext into dL/dstate over lam and returns
// dL/daction (the two step functions of cart_rollout_forward / _reverse).
// (The workgroup's LDS is named here, not handed in as a pointer: its address
// is then a constant to the compiler - handed in, the analytic kernel took 255
// VGPRs instead of 251 and the learnt one 256 + 2 AGPRs, one wave per SIMD.)
template <class Step, class Adjoint>
__device__ __forceinline__ void policy_step_body(const CartTrainArgs &A, Step &&step,
                                                 Adjoint &&adjoint) {
  extern __shared__ float lds[];
  const int H = A.H, B = A.B;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float *stash = lds + (rOut + H) * kTrLd;
  const ApgCartpolePolicy &P = A.p;
  // who owns what of the weight gradients: 32-unit layers (fc0, fc3) m32 / g32
  // (8 groups), 64-unit layers (fc1, fc2, the head padded to 64) m64 / g64 (4)
  const int m32 = tid & 31, g32 = tid >> 5, m64 = lane, g64 = wave;
  float gw0[1] = {0.f}, gw1[8], gw2[16], gw3[8], gwo[8];
  float gb0 = 0.f, gb1 = 0.f, gb2 = 0.f, gb3 = 0.f, gbo = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) gw1[j] = gw3[j] = gwo[j] = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) gw2[j] = 0.f;

  const int nchunks = (B + kTrChunk - 1) / kTrChunk;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int b = chunk * kTrChunk + lane;
    const bool live = b < B;
    // a dead lane computes on zeros and adds nothing: zero loss, zero seed.
    // Component `wave` of the input; column 0 is read as 0 (Net.forward)
    lds[(rX + wave) * kTrLd + lane] =
        (live && wave > 0) ? A.in_state[(size_t)b * kCptIn + wave] : 0.f;
    __syncthreads();
    layer_fwd<kCptH0, kCptIn>(P.w0, P.b0, lds + rX * kTrLd, lds + rH0 * kTrLd, wave, lane);
    __syncthreads();
    layer_fwd<kCptH1, kCptH0>(P.w1, P.b1, lds + rH0 * kTrLd, lds + rH1 * kTrLd, wave, lane);
    __syncthreads();
    layer_fwd<kCptH2, kCptH1>(P.w2, P.b2, lds + rH1 * kTrLd, lds + rH2 * kTrLd, wave, lane);
    __syncthreads();
    layer_fwd<kCptH3, kCptH2>(P.w3, P.b3, lds + rH2 * kTrLd, lds + rH3 * kTrLd, wave, lane);
    __syncthreads();
    // the head: H units, dealt to the waves one at a time
    for (int u = wave; u < H; u += kTrWaves) {
      float z[1] = {P.b_out[u]};
      cpt_dense<1>(
          z, kCptH3, [&](int, int j) { return P.w_out[u * kCptH3 + j]; },
          [&](int j) { return lds[(rH3 + j) * kTrLd + lane]; });
      lds[(rOut + u) * kTrLd + lane] = tanhf(z[0]);
    }
    __syncthreads();
    if (A.actions_out) {
      // [B][H]: the chunk's stretch is contiguous
      const int rows_live = B - chunk * kTrChunk < kTrChunk ? B - chunk * kTrChunk : kTrChunk;
      float *dst = A.actions_out + (size_t)chunk * kTrChunk * H;
      for (int e = tid; e < rows_live * H; e += kTrBlock) {
        const int s = e / H, k = e - s * H;
        dst[e] = lds[(rOut + k) * kTrLd + s];
      }
      __syncthreads();
    }
    if (wave == 0) {
      // the rollout of cartpole.hip's kernel, lane = sample; the cotangent of
      // the head's pre-activation replaces the action it belongs to
      auto action = [&](int k) { return lds[(rOut + k) * kTrLd + lane]; };
      auto ST = [&](int k, int i) -> float & { return stash[(k * 4 + i) * kTrChunk + lane]; };
      float s0[4], s[4], lam[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) s0[i] = live ? A.state0[(size_t)b * 4 + i] : 0.f;
      const float loss = cart_rollout_forward(
          H, s0, s, action, ST, step, [](int, const float (&)[4]) {});
      const float sum = wave_sum(live ? loss : 0.f);
      if (lane == 0) {
        A.loss_partials[chunk] = sum;
        if (gridDim.x == 1 && A.out.loss) A.out.loss[0] = sum;
      }
      cart_rollout_reverse(
          H, s0, s, lam, action, ST, adjoint,
          [&](int k, float g) {
            float *at = lds + (rOut + k) * kTrLd + lane;
            *at = live ? cpt_dtanh(g, *at) : 0.f;
          });
    }
    __syncthreads();
    // the head, reverse: cotangent of h3 into registers, the head's weight
    // gradient (reads h3), then the cotangent over h3
    {
      float acc[kCptH3 / kTrWaves];
      layer_dx<kCptH3>(acc, H, P.w_out, lds + rOut * kTrLd, wave, lane);
      if (m64 < H)
        layer_wgrad<8>(gwo, gbo, lds + (rOut + m64) * kTrLd, lds + (rH3 + g64 * 8) * kTrLd);
      __syncthreads();
      layer_dz_store(acc, lds + rH3 * kTrLd, wave, lane);
      __syncthreads();
    }
    {   // fc3: 64 -> 32
      float acc[kCptH2 / kTrWaves];
      layer_dx<kCptH2>(acc, kCptH3, P.w3, lds + rH3 * kTrLd, wave, lane);
      layer_wgrad<8>(gw3, gb3, lds + (rH3 + m32) * kTrLd, lds + (rH2 + g32 * 8) * kTrLd);
      __syncthreads();
      layer_dz_store(acc, lds + rH2 * kTrLd, wave, lane);
      __syncthreads();
    }
    {   // fc2: 64 -> 64
      float acc[kCptH1 / kTrWaves];
      layer_dx<kCptH1>(acc, kCptH2, P.w2, lds + rH2 * kTrLd, wave, lane);
      layer_wgrad<16>(gw2, gb2, lds + (rH2 + m64) * kTrLd, lds + (rH1 + g64 * 16) * kTrLd);
      __syncthreads();
      layer_dz_store(acc, lds + rH1 * kTrLd, wave, lane);
      __syncthreads();
    }
    {   // fc1: 32 -> 64
      float acc[kCptH0 / kTrWaves];
      layer_dx<kCptH0>(acc, kCptH1, P.w1, lds + rH1 * kTrLd, wave, lane);
      layer_wgrad<8>(gw1, gb1, lds + (rH1 + m64) * kTrLd, lds + (rH0 + g64 * 8) * kTrLd);
      __syncthreads();
      layer_dz_store(acc, lds + rH0 * kTrLd, wave, lane);
      __syncthreads();
    }
    // fc0: 4 -> 32, one input per thread (groups 0..3); no input cotangent
    if (g32 < kCptIn) layer_wgrad<1>(gw0, gb0, lds + (rH0 + m32) * kTrLd, lds + (rX + g32) * kTrLd);
    __syncthreads();   // the next chunk's input overwrites x
  }

  // the workgroup's sums: straight to the last stage when it is the only one,
  // else into its row (the flat gradient's layout)
  const bool single = gridDim.x == 1;
  float *row = A.rows + (size_t)blockIdx.x * cpt_grads(H);
  auto put = [&](int dest, float v) {
    if (single) train_finish(A.out, dest, v);
    else row[dest] = v;
  };
  if (g32 < kCptIn) put(kCptGW0 + m32 * kCptIn + g32, gw0[0]);
  if (g32 == 0) put(kCptGB0 + m32, gb0), put(kCptGB3 + m32, gb3);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    put(kCptGW1 + m64 * kCptH0 + g64 * 8 + j, gw1[j]);
    put(kCptGW3 + m32 * kCptH2 + g32 * 8 + j, gw3[j]);
    if (m64 < H) put(kCptGWout + m64 * kCptH3 + g64 * 8 + j, gwo[j]);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) put(kCptGW2 + m64 * kCptH1 + g64 * 16 + j, gw2[j]);
  if (g64 == 0) {
    put(kCptGB1 + m64, gb1), put(kCptGB2 + m64, gb2);
    if (m64 < H) put(kCptGWout + kCptH3 * H + m64, gbo);
  }
}

__global__ __launch_bounds__(kTrBlock) void cart_train_kernel(CartTrainArgs A) {
  const CartConst c = A.c;
  policy_step_body(
      A, [&](float (&x)[4], float a) { cart_step(x, a, c); },
      [&](float (&l)[4], const float (&pre)[4], float a) {
        return cart_step_adjoint(l, pre[1], pre[3], cart_step_aux(pre, a, c), c);
      });
}

// The same step through LearntCartpoleDynamics (apg_cartpole_learnt_mlp_train_
// step): the simulator is frozen in the controller phase, so only the two step
// functions differ - cart_learnt_step / cart_learnt_step_adjoint of
// cartpole_learnt_math.h, as cart_learnt_rollout_kernel (cartpole_learnt.hip)
// calls them, all 64 residual units in ascending order on wave 0.  The step
// constants are built here from the module's six live device parameters, the
// residual's packed unit rows sit in LDS behind the rollout's stash.
struct CartLearntTrainArgs {
  CartTrainArgs t;        // (t.c is not read)
  ApgCartpoleLearnt m;
  float dt;
};

__global__ __launch_bounds__(kTrBlock) void cartpole_learnt_policy_kernel(
    CartLearntTrainArgs A) {
  extern __shared__ float lds[];
  float *rows = lds + train_lds_floats(A.t.H);
  stage_residual(rows, A.m);
  const CartConst c = make_learnt_const(load_params(A.m), A.dt);
  policy_step_body(
      A.t, [&](float (&x)[4], float a) { cart_learnt_step(x, a, c, rows); },
      [&](float (&l)[4], const float (&pre)[4], float a) {
        return cart_learnt_step_adjoint(l, pre, a, cart_step_aux(pre, a, c), c, rows);
      });
}

// Element c of the flat gradient = the sum over the workgroups' rows: the 8
// threads of a column add rows r, r + 8, ... in order, then a fixed tree (the
// scheme of fit_rows_sum, residual_fit.h, with a row length known at run time);
// thread r == 0 finishes the element.  The last workgroup sums the loss
// partials instead, as reduce_partials_kernel (common.hip) does.
constexpr int kTrCols = 32, kTrSplit = 8;
static_assert(kTrCols * kTrSplit == kTrBlock, "one workgroup of columns");
struct CartTrainReduceArgs {
  const float *rows, *loss_partials;
  CartTrainOut out;
  int nrows, npartials;
};
__global__ __launch_bounds__(kTrBlock) void cart_train_reduce_kernel(CartTrainReduceArgs A) {
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ double sm[kTrWaves];
    if (!A.out.loss) return;
    double acc = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < A.npartials; i += kTrBlock) acc += (double)A.loss_partials[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) A.out.loss[0] = (float)((sm[0] + sm[1]) + (sm[2] + sm[3]));
    return;
  }
  __shared__ float part[kTrSplit][kTrCols];
  const int row_len = cpt_grads(A.out.H);
  const int col = threadIdx.x % kTrCols, r = threadIdx.x / kTrCols;
  const int cc = blockIdx.x * kTrCols + col;
  float acc = 0.f;
  if (cc < row_len) {
#pragma unroll 4
    for (int i = r; i < A.nrows; i += kTrSplit) acc += A.rows[(size_t)i * row_len + cc];
  }
  part[r][col] = acc;
  __syncthreads();
  if (r != 0 || cc >= row_len) return;
  const float v = ((part[0][col] + part[1][col]) + (part[2][col] + part[3][col])) +
                  ((part[4][col] + part[5][col]) + (part[6][col] + part[7][col]));
  train_finish(A.out, cc, v);
}

bool all_set(const ApgCartpolePolicyGrads &g) {
  return g.w0 && g.b0 && g.w1 && g.b1 && g.w2 && g.b2 && g.w3 && g.b3 && g.w_out && g.b_out;
}

// Everything the two entry points check and build alike: the arguments but for
// the simulator (argument errors before any HIP call), the kernels' arguments
// and the launches.
int check_step_args(const float *in_state, const float *state0, const void *sim,
                    const ApgCartpolePolicy *policy, int B, int H, const float *loss_partials,
                    const ApgCartpolePolicyGrads *grads, const float *workspace,
                    const ApgCartpoleSgdUpdate *update) {
  if (B < 1) { set_error("B must be >= 1 (got %d)", B); return APG_ERR_ARG; }
  if (H < 1 || H > APG_MAX_HORIZON) {
    set_error("H must be in [1, %d] (got %d)", APG_MAX_HORIZON, H);
    return APG_ERR_ARG;
  }
  if (!sim || !policy || !grads) {
    set_error("params / policy / grads is NULL");
    return APG_ERR_ARG;
  }
  if (!policy->w0 || !policy->b0 || !policy->w1 || !policy->b1 || !policy->w2 ||
      !policy->b2 || !policy->w3 || !policy->b3 || !policy->w_out || !policy->b_out) {
    set_error("policy weight pointer is NULL");
    return APG_ERR_ARG;
  }
  if (!all_set(*grads)) { set_error("grads: pointer is NULL"); return APG_ERR_ARG; }
  if (update && (!all_set(update->param) || !all_set(update->momentum_buf))) {
    set_error("update: parameter / momentum pointer is NULL");
    return APG_ERR_ARG;
  }
  if (update && !(update->lr == update->lr && update->momentum == update->momentum)) {
    set_error("update: lr / momentum is NaN");
    return APG_ERR_ARG;
  }
  if (!in_state || !state0 || !loss_partials || !workspace) {
    set_error("in_state / state0 / loss_partials / workspace must not be NULL");
    return APG_ERR_ARG;
  }
  return APG_OK;
}

CartTrainArgs step_args(const float *in_state, const float *state0,
                        const ApgCartpolePolicy *policy, int B, int H, float *loss_partials,
                        float *loss, const ApgCartpolePolicyGrads *grads, float *actions_out,
                        float *workspace, const ApgCartpoleSgdUpdate *update) {
  CartTrainArgs A;
  A.in_state = in_state, A.state0 = state0, A.p = *policy;
  A.loss_partials = loss_partials, A.actions_out = actions_out, A.rows = workspace;
  A.out.grads = *grads;
  A.out.param = update ? update->param : *grads;
  A.out.mom = update ? update->momentum_buf : *grads;
  A.out.lr = update ? update->lr : 0.0, A.out.momentum = update ? update->momentum : 0.0;
  A.out.loss = loss, A.out.H = H, A.out.update = update != nullptr;
  A.c = CartConst{};
  A.B = B, A.H = H;
  return A;
}

// `kernel(args)` on min(ceil(B / 64), 256) workgroups with `lds` bytes, then -
// more than one workgroup - the second stage over their rows
template <class Args>
int launch_step(void (*kernel)(Args), const Args &args, const CartTrainArgs &A, size_t lds,
                hipStream_t st, const char *what) {
  const int grid = train_grid(A.B);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return check_launch("hipFuncSetAttribute(cartpole train step)");
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kTrBlock), lds, st, args);
  if (int e = check_launch(what)) return e;
  if (grid == 1) return APG_OK;
  CartTrainReduceArgs R;
  R.rows = A.rows, R.loss_partials = A.loss_partials, R.out = A.out;
  R.nrows = grid, R.npartials = train_chunks(A.B);
  const int columns = (cpt_grads(A.H) + kTrCols - 1) / kTrCols;
  hipLaunchKernelGGL(cart_train_reduce_kernel, dim3(columns + 1), dim3(kTrBlock), 0, st, R);
  return check_launch("cartpole_mlp_train_reduce");
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_cartpole_mlp_train_step_workspace_floats(int B, int H) {
  if (B <= 0 || H < 1 || H > APG_MAX_HORIZON) return 0;
  return train_grid(B) * cpt_grads(H);
}

int apg_cartpole_mlp_train_step(const float *in_state, const float *state0, float dt,
                                const ApgCartpoleParams *params,
                                const ApgCartpolePolicy *policy, int B, int H,
                                float *loss_partials, float *loss,
                                const ApgCartpolePolicyGrads *grads, float *actions_out,
                                float *workspace, const ApgCartpoleSgdUpdate *update,
                                apg_stream_t stream) {
  if (int e = check_step_args(in_state, state0, params, policy, B, H, loss_partials, grads,
                              workspace, update))
    return e;
  CartTrainArgs A = step_args(in_state, state0, policy, B, H, loss_partials, loss, grads,
                              actions_out, workspace, update);
  A.c = make_const(*params, dt);
  return launch_step(cart_train_kernel, A, A, train_lds_floats(H) * sizeof(float),
                     (hipStream_t)stream, "cartpole_mlp_train_step");
}

int apg_cartpole_learnt_mlp_train_step(const float *in_state, const float *state0, float dt,
                                       const ApgCartpoleLearnt *model,
                                       const ApgCartpolePolicy *policy, int B, int H,
                                       float *loss_partials, float *loss,
                                       const ApgCartpolePolicyGrads *grads,
                                       float *actions_out, float *workspace,
                                       const ApgCartpoleSgdUpdate *update,
                                       apg_stream_t stream) {
  if (int e = check_step_args(in_state, state0, model, policy, B, H, loss_partials, grads,
                              workspace, update))
    return e;
  if (const char *e = cart_learnt_check(model, /*need_residual=*/true)) {
    set_error("%s", e);
    return APG_ERR_ARG;
  }
  CartLearntTrainArgs A;
  A.t = step_args(in_state, state0, policy, B, H, loss_partials, loss, grads, actions_out,
                  workspace, update);
  A.m = *model, A.dt = dt;
  return launch_step(cartpole_learnt_policy_kernel, A, A.t,
                     (train_lds_floats(H) + kCartResFloats) * sizeof(float),
                     (hipStream_t)stream, "cartpole_learnt_mlp_train_step");
}

}  // extern "C"
