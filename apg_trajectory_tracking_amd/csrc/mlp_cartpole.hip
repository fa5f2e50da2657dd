// mlp_cartpole.hip - closed-loop evaluation of the cart-pole controller: B
// episodes of up to max_steps steps in ONE launch, the policy inside the kernel.
//
// Restated from (paths relative to the reference repo):
//   scripts/evaluate_cartpole.py:79-318   Evaluator.evaluate_in_environment /
//                                          evaluate_swingup (APPLY_UNTIL = 1)
//   neural_control/controllers/network_wrapper.py:101-149  CartpoleWrapper
//                                          (raw state, no normalisation)
//   neural_control/models/simple_model.py:9-28  Net: 4 -> 32 -> 64 -> 64 -> 32
//                                          -> H, tanh after every layer;
//                                          forward() zeroes input column 0
//   neural_control/environments/cartpole_env.py:57-82  CartPoleEnv._step /
//                                          is_upright (the theta wrap)
// The step is cart_step (cartpole_math.h), unchanged.
//
// Two quirks of the reference loop are restated:
//  * the policy zeroes column 0 of its input IN PLACE, and from the second
//    step on that input shares memory with the environment's float32 state
//    (torch.from_numpy + .float() of a float32 array is no copy): the cart
//    position entering steps 1, 2, ... is 0.  The first step starts from the
//    float64 reset state, which is copied, so x0 is stepped as drawn.  The
//    dynamics never read x, so only the recorded x column shows it.
//  * the wrap `if theta > pi: theta -= 2 pi; if theta <= -pi: theta += 2 pi`
//    compares and adds a numpy float32 scalar with Python floats, i.e. in fp32
//    under NumPy >= 2 (the goldens' NumPy): atan2f's -fp32(pi) becomes
//    +fp32(pi), +fp32(pi) stays.
//
// Layout as the other in-kernel policies (policy_mfma.h / policy_mfma16.h):
// one wave = 32 episodes, layers chained through the accumulator registers on
// the 16-bit matrix pipe with fp16-split operands, the weights packed into
// LDS tables by a pack launch.  Only row 0 of fc_out is evaluated
// (action_seq[:, 0] is the action applied).
//
// cart_closed_loop_kernel<true> flies the LEARNT environment of the adapt flow
// (LearntCartpoleDynamics, cartpole_learnt_math.h) with the same policy.
#include <type_traits>

#include "apg_device.h"
#include "cart_flight_rule.h"
#include "cartpole_learnt_math.h"
#include "cartpole_math.h"
#include "policy_mfma.h"
#include "policy_mfma16.h"

namespace apg {
namespace {

constexpr int kNI = 4;                     // network inputs
constexpr int kMaxWaves = 4;               // waves per workgroup (128 episodes)

// Tables: bias tables [rb][16][2] (fc0 1 row block, fc1 2, fc2 2, fc3 1, head
// 1), then 19 A-operand blocks of 2 KB: fc0 (one k-block: inputs 8 hi + j of
// the 4), fc1 [rb of 2][kb of 2], fc2 [rb of 2][kb of 4], fc3 [kb of 4], head
// [kb of 2] (row 0 only).
constexpr int hT0 = 0, hT1 = 32, hT2 = 96, hT3 = 160, hTo = 192, hTend = 224;  // floats
constexpr int hA = 1024;                                                      // bytes
constexpr int n0 = 0, n1 = 1, n2 = 5, n3 = 13, nO = 17, nBlocks16 = 19;
constexpr int kCartLds = (hA + nBlocks16 * kBlock16) / 4;  // 9 984 floats = 39 936 B
static_assert(hTend <= hA / 4, "LDS map");
static_assert(kCartLds * 4 < 61440, "LdsView16: one base covers the tables");

__device__ __forceinline__ float cart16_weight(const ApgCartpolePolicy &p, int n, int row,
                                               int j, int hi) {
  if (n < n1) {
    const int k = 8 * hi + j;
    return k < kNI ? p.w0[row * kNI + k] : 0.f;
  }
  if (n < n2) {
    const int m = n - n1, rb = m / 2, kb = m % 2;
    return p.w1[(rb * 32 + row) * 32 + kin(kb, j, hi)];
  }
  if (n < n3) {
    const int m = n - n2, rb = m / 4, kb = m % 4;
    return p.w2[(rb * 32 + row) * 64 + kin(kb, j, hi)];
  }
  if (n < nO) return p.w3[row * 64 + kin(n - n3, j, hi)];
  return row == 0 ? p.w_out[kin(n - nO, j, hi)] : 0.f;
}

__global__ __launch_bounds__(256) void cart_pack16_kernel(ApgCartpolePolicy p, float *dst) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, T = gridDim.x * blockDim.x;
  unsigned *du = reinterpret_cast<unsigned *>(dst);
  for (int idx = tid; idx < nBlocks16 * 64 * 4; idx += T) {
    const int q = idx & 3, l = (idx >> 2) & 63, n = idx >> 8;
    unsigned h, lo;
    split_pair(cart16_weight(p, n, l & 31, 2 * q, l >> 5),
               cart16_weight(p, n, l & 31, 2 * q + 1, l >> 5), h, lo);
    du[(hA + n * kBlock16) / 4 + l * 4 + q] = h;
    du[(hA + n * kBlock16 + 1024) / 4 + l * 4 + q] = lo;
  }
  for (int idx = tid; idx < hA / 4; idx += T) {
    const int base = idx < hT1 ? hT0 : idx < hT2 ? hT1 : idx < hT3 ? hT2 : idx < hTo ? hT3 : hTo;
    const int e = idx - base, hi = e & 1, i = (e >> 1) & 15, rb = e >> 5;
    const int row = rb * 32 + rrow(i) + 4 * hi;   // (table of entry idx: base)
    float v = 0.f;
    if (idx < hT1) v = p.b0[row];
    else if (idx < hT2) v = p.b1[row];
    else if (idx < hT3) v = p.b2[row];
    else if (idx < hTo) v = p.b3[row];
    else if (idx < hTend) v = row == 0 ? p.b_out[0] : 0.f;
    dst[idx] = v;                                  // (the pad after hTend: zeros)
  }
}

struct CartLoopArgs {
  const float *state0;     // [4][B]
  int *steps;              // [B] steps taken
  int *upright;            // [B] see apg.h
  double *vel_sum;         // [B] sum of the recorded |x_dot|
  double *vel_sq;          // [B] sum of their squares
  float *states;           // [T][4][B] or NULL: state after each step
  float *actions;          // [T][B] or NULL: action applied at each step
  const float *tables;
  CartConst c;
  float thresh_div;
  int B, T, mode, burn_in;
};

// the policy's first action for the state s (input column 0 zeroed)
__device__ __forceinline__ float cart_policy(const float (&s)[4], int hi, const LdsView &L,
                                             const LdsView16 &L16) {
  // fc0: 4 -> 32, one k-block (the upper half-wave's slots are zero)
  f32x16 x;
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = L.T(hT0 + i * 2);
  {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (hi || j >= kNI || j == 0) ? 0.f : s[j < kNI ? j : 0];
    x = mma3(L16.A(hA, n0), split8(v), x);
  }
  // fc1: 32 -> 64
  f32x16 a[2], u[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) a[rb][i] = L.T(hT1 + (rb * 16 + i) * 2);
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tanh_fast(x[8 * kb + j]);
    const Op16 xv = split8(v);
    a[0] = mma3(L16.A(hA, n1 + kb), xv, a[0]);
    a[1] = mma3(L16.A(hA, n1 + 2 + kb), xv, a[1]);
  }
  // fc2: 64 -> 64
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) u[rb][i] = L.T(hT2 + (rb * 16 + i) * 2);
  dense64_16(u, a, L16, hA, n2, [](int, int, float v) { return tanh_fast(v); });
  // fc3: 64 -> 32
  f32x16 y;
#pragma unroll
  for (int i = 0; i < 16; ++i) y[i] = L.T(hT3 + i * 2);
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tanh_fast(u[kb >> 1][8 * (kb & 1) + j]);
    y = mma3(L16.A(hA, n3 + kb), split8(v), y);
  }
  // head row 0: register 0 of the lower half-wave
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = L.T(hTo + i * 2);
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tanh_fast(y[8 * kb + j]);
    z = mma3(L16.A(hA, nO + kb), split8(v), z);
  }
  const float oth = other_half(z[0]);
  return tanhf(hi ? oth : z[0]);
}

// The learnt environment (apg_cartpole_learnt_mlp_closed_loop): the module's
// tensors; its residual's unit rows (cartpole_learnt_math.h) sit in LDS behind
// the policy tables, its six physical parameters are read at kernel start.
struct CartLearntLoopArgs : CartLoopArgs {
  ApgCartpoleLearnt m;
};

template <bool LEARNT>
__global__ __launch_bounds__(kMaxWaves * 64) void cart_closed_loop_kernel(
    std::conditional_t<LEARNT, CartLearntLoopArgs, CartLoopArgs> A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  fill_lds(lds, A.tables, kCartLds);
  CartConst cc = A.c;
  if constexpr (LEARNT) {
    float *rows = lds + kCartLds;
    for (int t = threadIdx.x; t < kCartResFloats; t += blockDim.x)
      rows[t] = cart_residual_packed(t, A.m.w1, A.m.b1, A.m.w2);
    cc = make_learnt_const(CartLearntParams{*A.m.max_force_mag, *A.m.masspole, *A.m.length,
                                            *A.m.friction, *A.m.total_mass,
                                            *A.m.polemass_length},
                           A.c.dt);
    __syncthreads();
  }
  const CartConst &c = cc;
  const int lane = threadIdx.x & 63, hi = lane >> 5;
  const LdsView L(lds, lane);
  const LdsView16 L16(lds, lane);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = (blockIdx.x * (blockDim.x >> 6) + wave) * 32 + (lane & 31);
  const int B = A.B, T = A.T;
  const bool live = b < B;
  const unsigned pN = (unsigned)B * 4u;
  // a NULL tensor becomes an empty buffer: stores are dropped
  const Planes Ps0(A.state0, 4, pN);
  const Planes Pst(A.states, A.states ? T * 4 : 0, pN);
  const Planes Pac(A.actions, A.actions ? T : 0, pN);
  const unsigned vb = live ? (unsigned)b * 4u : kDead;
  const bool swingup = A.mode == APG_CARTPOLE_SWINGUP;
  const float pi = 3.14159265358979323846f, two_pi = 2.f * pi;

  float s[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = Ps0.ld(vb, i * pN);
  double vs = 0.0, vq = 0.0;
  int steps = 0;
  bool alive = live, upright = true;

#pragma unroll 1
  for (int k = 0; k < T; ++k) {
    const unsigned pB = opaque(pN);
    const unsigned vrec = (alive && hi == 0) ? vb : kDead;
    const float act = cart_policy(s, hi, L, L16);
    if (k > 0) s[0] = 0.f;          // the in-place zeroing of the policy input
    if constexpr (LEARNT) {
      // the residual on the pre-step state: each half-wave takes 32 of the 64
      // hidden units, the two halves exchange their 4 sums (same order on both:
      // both end with the same state)
      const float z[5] = {s[0], s[1], s[2], s[3], act};
      cart_step(s, act, c);
      float add[4] = {0.f, 0.f, 0.f, 0.f};
      int u0 = 32 * hi;
      asm volatile("" : "+v"(u0));
      cart_residual_add(add, z, lds + kCartLds, u0, u0 + 32);
#pragma unroll
      for (int o = 0; o < 4; ++o) s[o] += add[o] + other_half(add[o]);
    } else {
      cart_step(s, act, c);
    }
    // CartPoleEnv._step: the comparisons with the ORIGINAL theta, in fp32
    const float th = s[2];
    if (th > pi) s[2] = th - two_pi;
    if (th <= -pi) s[2] = two_pi + th;
#pragma unroll
    for (int i = 0; i < 4; ++i) Pst.st(vrec, (k * 4 + i) * pB, s[i]);
    Pac.st(vrec, k * pB, act);
    // the statistics take |x_dot| (swing-up: the mean of np.absolute of the
    // recorded values)
    const double v = (double)fabsf(s[1]);
    bool done = false;
    if (swingup) {
      if (k > A.burn_in) {
        vs += v, vq += v * v;
        if (s[2] > 1.f) upright = false;
      }
    } else if (alive) {   // (an episode that stopped keeps stepping with its wave)
      vs += v, vq += v * v;
      if (!(-A.thresh_div < s[2] && s[2] < A.thresh_div)) {
        done = true;
        upright = false;
      }
    }
    if (alive) steps = k + 1;
    alive = alive && !done;
    if (!__any(alive)) break;
  }
  if (live && hi == 0) {
    A.steps[b] = steps;
    A.upright[b] = upright ? 1 : 0;
    A.vel_sum[b] = vs;
    A.vel_sq[b] = vq;
  }
}

// argument checks and the two launches of both entry points; `learnt` NULL:
// the analytic environment on `params`
int closed_loop(const ApgCartpoleFlight *flight, float dt, const ApgCartpoleParams *params,
                const ApgCartpoleLearnt *learnt, const ApgCartpolePolicy *policy, int B,
                float *workspace, apg_stream_t stream) {
  if (!(params || learnt) || !policy) {
    set_error("%s / policy is NULL", learnt ? "model" : "params");
    return APG_ERR_ARG;
  }
  if (learnt && cart_learnt_check(learnt, true)) {
    set_error("learnt model pointer is NULL");
    return APG_ERR_ARG;
  }
  if (!policy->w0 || !policy->b0 || !policy->w1 || !policy->b1 || !policy->w2 ||
      !policy->b2 || !policy->w3 || !policy->b3 || !policy->w_out || !policy->b_out) {
    set_error("policy weight pointer is NULL");
    return APG_ERR_ARG;
  }
  CartFlightRule rule;
  if (const char *e = cart_flight_check(flight, B, &rule)) {
    set_error("%s", e);
    return APG_ERR_ARG;
  }
  // this loop's own rules: plane offsets are 32-bit, the tables need a workspace
  if ((long long)B * 4 * 4 * (long long)rule.T >= (1ll << 32) - 64) {
    set_error("B x max_steps too large for 32-bit plane offsets; split the batch");
    return APG_ERR_ARG;
  }
  if (!workspace) {
    set_error("NULL buffer");
    return APG_ERR_ARG;
  }
  CartLearntLoopArgs A = {};
  A.state0 = flight->state0, A.steps = flight->steps, A.upright = flight->upright;
  A.vel_sum = flight->vel_sum, A.vel_sq = flight->vel_sq;
  A.states = flight->states, A.actions = flight->actions;
  A.tables = workspace;
  if (learnt) {
    A.c.dt = dt;          // (the rest is built in the kernel from the tensors)
    A.m = *learnt;
  } else {
    A.c = make_const(*params, dt);
  }
  A.thresh_div = rule.thresh_div;
  A.B = B, A.T = rule.T, A.mode = rule.mode, A.burn_in = rule.burn_in;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cart_pack16_kernel, dim3((nBlocks16 * 256 + 255) / 256), dim3(256), 0,
                     st, *policy, workspace);
  // a small batch gets a small workgroup: the trainer's 10 episodes are one wave
  const int waves = (B + 31) / 32 < kMaxWaves ? (B + 31) / 32 : kMaxWaves;
  const int per_block = waves * 32;
  const dim3 grid((B + per_block - 1) / per_block), block(waves * 64);
  if (learnt)
    hipLaunchKernelGGL(cart_closed_loop_kernel<true>, grid, block,
                       (kCartLds + kCartResFloats) * sizeof(float), st, A);
  else
    hipLaunchKernelGGL(cart_closed_loop_kernel<false>, grid, block, kCartLds * sizeof(float),
                       st, static_cast<const CartLoopArgs &>(A));
  return check_launch(learnt ? "cartpole_learnt_mlp_closed_loop" : "cartpole_mlp_closed_loop");
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_cartpole_policy_workspace_floats(void) { return kCartLds; }

int apg_cartpole_mlp_closed_loop(const ApgCartpoleFlight *flight, float dt,
                                 const ApgCartpoleParams *params,
                                 const ApgCartpolePolicy *policy, int B,
                                 float *workspace, apg_stream_t stream) {
  return closed_loop(flight, dt, params, nullptr, policy, B, workspace, stream);
}

int apg_cartpole_learnt_mlp_closed_loop(const ApgCartpoleFlight *flight, float dt,
                                        const ApgCartpoleLearnt *model,
                                        const ApgCartpolePolicy *policy, int B,
                                        float *workspace, apg_stream_t stream) {
  if (!model) {
    set_error("model / policy is NULL");
    return APG_ERR_ARG;
  }
  return closed_loop(flight, dt, nullptr, model, policy, B, workspace, stream);
}

}  // extern "C"
