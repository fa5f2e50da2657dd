// mlp_wing.hip - the fixed-wing controller on the matrix cores (BASELINE config
// 4's full training step: fixed-wing concurrent, H = 20).
//
// Replaces the policy part of the concurrent step of the fixed-wing trainer:
//   TrainBase.run_epoch, concurrent branch   scripts/train_base.py:198-204
//     actions = sigmoid(net(in_state, in_ref_state)) reshaped [B, H, 4]
//   hutter_model.Net(9, 1, 3, 80, conv=False) neural_control/models/hutter_model.py:6-49
//     s1 = tanh(W_s in_state + b_s) (9 -> 64), r1 = tanh(W_r in_ref + b_r) (3 -> 64),
//     h1 = tanh(W_1 [s1, r1] + b_1) (128 -> 64), h2, h3 (64 -> 64), out (64 -> 80)
// and its backward.  The dynamics / loss / adjoint stay in wing.hip
// (apg_wing_rollout_fwd_bwd): the forward kernel writes the actions as
// [H][4][B] planes - exactly what that kernel reads - and the reverse kernel
// starts from its dL/dactions planes.  Same layout as policy_mfma.h: one wave =
// 32 trajectories, layers chain through the accumulator registers; the two
// input branches are ONE block-diagonal 12 -> 128 layer.  Since round 3 the
// layers are v_mfma_f32_32x32x16_f16 products of fp16-split operands
// (policy_mfma16.h: fp32 accuracy, cotangents scaled per trajectory).  Weight
// gradients: cotangent planes x activation planes by apg_planes_gemm_grouped.
// The same step through the learnt simulator (apg_wing_learnt_mlp_train_step):
// wing_learnt_policy_fwd_kernel runs policy, rollout, loss and adjoint in one
// kernel, in front of the unchanged reverse kernel.
#include "apg_device.h"
#include "policy_mfma.h"
#include "policy_mfma16.h"
#include "wing_math.h"
#include "learnt_residual.h"
#include "wing_flight_rule.h"
#include "wing_learnt_math.h"
#include "wing_rollout_math.h"

namespace apg {
namespace {

constexpr int kNS = 9, kNR = 3, kNI = kNS + kNR;  // network inputs (12)
constexpr int kW = 64, kW0 = 2 * kW;              // layer widths (64; first 128)
constexpr int kNA = 80;                           // head width = H x 4 actions
constexpr int kThreads = 512;
constexpr int kTrajPerBlock = kThreads / 2;

// ------------------------------------------------------------------ forward
struct PackArgs {
  ApgWingPolicy pol;
  float *dst;
  int head_rows;  // rows of fc_out behind pol.w_out / b_out that may be read
};

// Tables (fp16 split operands, policy_mfma16.h).  Forward: the bias tables
// [rb][16][2] (first layer 4 row blocks, then fc1, fc2, fc3, head 3 row
// blocks), then 48 A-operand blocks of 2 KB: first layer [rb of 4] (one
// k-block: inputs 8 hi + j of the 12), fc1 [rb][kb of 8], fc2 / fc3 [rb][kb],
// head [rb of 3][kb].
constexpr int hT0 = 0, hT1 = 128, hT2 = 192, hT3 = 256, hTo = 320;   // floats
constexpr int hA = 2048;                                            // bytes
constexpr int n0 = 0, n1 = 4, n2 = 20, n3 = 28, nO = 36, nBlocks16 = 48;
constexpr int kFwd16Lds = (hA + nBlocks16 * kBlock16) / 4;   // 25 088 floats = 100 352 B
static_assert(hTo + 96 <= hA / 4, "LDS map");

// input index of slot j of k-block kb for a layer fed by FOUR row blocks
// (fc1: 128 inputs) or two (64): registers 8 (kb & 1) .. + 7 of block kb >> 1
__device__ __forceinline__ float wing_fwd16_weight(const ApgWingPolicy &p, int n, int row,
                                                   int j, int hi, int head_rows) {
  if (n < n1) {                        // [states_in 0; 0 ref_in], inputs 8 hi + j
    const int m = n * 32 + row, k = 8 * hi + j;
    if (m < kW && k < kNS) return p.w_s[m * kNS + k];
    if (m >= kW && k >= kNS && k < kNI) return p.w_r[(m - kW) * kNR + (k - kNS)];
    return 0.f;
  }
  if (n < n2) {
    const int m = n - n1, rb = m / 8, kb = m % 8;
    return p.w_1[(rb * 32 + row) * kW0 + kin(kb, j, hi)];
  }
  if (n < nO) {
    const int m = (n - n2) % 8, rb = m / 4, k = kin(m % 4, j, hi);
    return n < n3 ? p.w_2[(rb * 32 + row) * kW + k] : p.w_3[(rb * 32 + row) * kW + k];
  }
  const int m = n - nO, rb = m / 4, out = rb * 32 + row;
  return out < head_rows ? p.w_out[out * kW + kin(m % 4, j, hi)] : 0.f;
}

__global__ __launch_bounds__(256) void wing_pack_fwd16_kernel(PackArgs A) {
  const ApgWingPolicy &p = A.pol;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, T = gridDim.x * blockDim.x;
  unsigned *dst = reinterpret_cast<unsigned *>(A.dst);
  for (int idx = tid; idx < nBlocks16 * 64 * 4; idx += T) {
    const int q = idx & 3, l = (idx >> 2) & 63, n = idx >> 8;
    unsigned h, lo;
    split_pair(wing_fwd16_weight(p, n, l & 31, 2 * q, l >> 5, A.head_rows),
               wing_fwd16_weight(p, n, l & 31, 2 * q + 1, l >> 5, A.head_rows), h, lo);
    dst[(hA + n * kBlock16) / 4 + l * 4 + q] = h;
    dst[(hA + n * kBlock16 + 1024) / 4 + l * 4 + q] = lo;
  }
  for (int idx = tid; idx < 128; idx += T) {
    const int hi = idx & 1, i = (idx >> 1) & 15, rb = idx >> 5;
    const int row = rb * 32 + rrow(i) + 4 * hi;
    A.dst[hT0 + idx] = row < kW ? p.b_s[row] : p.b_r[row - kW];
    if (rb < 2) {
      A.dst[hT1 + idx] = p.b_1[row];
      A.dst[hT2 + idx] = p.b_2[row];
      A.dst[hT3 + idx] = p.b_3[row];
    }
    if (rb < 3) A.dst[hTo + idx] = row < A.head_rows ? p.b_out[row] : 0.f;
  }
}

struct Args {
  const float *feat, *ref_in;   // [9][B], [3][B]
  float *actions;               // [80][B] = [H][4][B]
  const float *grad_actions;    // [80][B] (reverse)
  float *x1, *h;                // [128][B], [192][B]
  float *d_zout, *d_pre;        // [80][B], [320][B]: fc1, fc2, fc3 (64 each), first layer (128)
  const float *tables;
  int B, NA;   // NA = 4 H head rows in use (40 or 80)
};

// this lane's place in the launch, as the policy part leaves it to what follows
// it in the same kernel: half-wave, plane offsets
struct WingLane {
  int hi;
  bool live;
  unsigned pN, vb, vr;
};

// The policy part of a forward kernel, tables already in LDS: the network once
// per trajectory on the matrix pipe, x1 / h to the planes the reverse kernel
// reads, the head's pre-activations z in accumulator layout (HB row blocks of
// 32: 3 for the 80 rows of H = 20, 2 where at most 64 are in use).  Shared by
// wing_policy_fwd_kernel and wing_learnt_policy_fwd_kernel.
template <int HB>
__device__ __forceinline__ void wing_policy_forward(const Args &A, const float *lds,
                                                    WingLane &Z, f32x16 (&z)[HB]) {
  const int lane = threadIdx.x & 63, hi = lane >> 5;
  const LdsView L(lds, lane);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = (blockIdx.x * (kThreads / 64) + wave) * 32 + (lane & 31);
  const int B = A.B;
  const bool live = b < B;
  const unsigned pN = (unsigned)B * 4u;
  const Planes Pfe(A.feat, kNS, pN), Prf(A.ref_in, kNR, pN);
  const Planes Px1(A.x1, kW0, pN), Ph(A.h, 3 * kW, pN);
  const unsigned vb = live ? (unsigned)b * 4u : kDead;
  const unsigned vr = live ? vb + (hi ? 4u * pN : 0u) : kDead;  // + row 4 hi

  float in[kNI];
#pragma unroll
  for (int j = 0; j < kNS; ++j) in[j] = Pfe.ld(vb, j * pN);
#pragma unroll
  for (int j = 0; j < kNR; ++j) in[kNS + j] = Prf.ld(vb, j * pN);

  // the layers on the 16-bit matrix pipe (policy_mfma16.h): every operand as
  // two fp16 terms, three products per k-block
  const LdsView16 L16(lds, lane);
  // first layer: [states_in 0; 0 ref_in], 12 -> 128: one k-block
  f32x16 x[4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) x[rb][i] = L.T(hT0 + (rb * 16 + i) * 2);
  {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = hi ? (8 + j < kNI ? in[8 + j < kNI ? 8 + j : 0] : 0.f) : in[j];
    const Op16 xi = split8(v);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) x[rb] = mma3(L16.A(hA, n0 + rb), xi, x[rb]);
  }
  // fc1 (tanh of the first layer applied, and stored, where it is consumed)
  f32x16 u[2], a[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) a[rb][i] = L.T(hT1 + (rb * 16 + i) * 2);
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = 8 * (kb & 1) + j;
      v[j] = tanh_fast(x[kb >> 1][i]);
      Px1.st(vr, ((kb >> 1) * 32 + rrow(i)) * pN, v[j]);
    }
    const Op16 xv = split8(v);
    a[0] = mma3(L16.A(hA, n1 + kb), xv, a[0]);
    a[1] = mma3(L16.A(hA, n1 + 8 + kb), xv, a[1]);
  }
  // fc2, fc3
#pragma unroll
  for (int layer = 0; layer < 2; ++layer) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) u[rb][i] = L.T((layer ? hT3 : hT2) + (rb * 16 + i) * 2);
    dense64_16(u, a, L16, hA, layer ? n3 : n2, [&](int rb, int i, float v) {
      const float tv = tanh_fast(v);
      Ph.st(vr, (layer * kW + rb * 32 + rrow(i)) * pN, tv);
      return tv;
    });
    a[0] = u[0], a[1] = u[1];
  }
  // head: 80 outputs in three row blocks
#pragma unroll
  for (int rb = 0; rb < HB; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) z[rb][i] = L.T(hTo + (rb * 16 + i) * 2);
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = 8 * (kb & 1) + j;
      v[j] = tanh_fast(a[kb >> 1][i]);
      Ph.st(vr, (2 * kW + (kb >> 1) * 32 + rrow(i)) * pN, v[j]);
    }
    const Op16 xv = split8(v);
#pragma unroll
    for (int rb = 0; rb < HB; ++rb) z[rb] = mma3(L16.A(hA, nO + rb * 4 + kb), xv, z[rb]);
  }
  Z.hi = hi, Z.live = live, Z.pN = pN, Z.vb = vb, Z.vr = vr;
}

__global__ __launch_bounds__(kThreads) void wing_policy_fwd_kernel(Args A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  fill_lds(lds, A.tables, kFwd16Lds);
  WingLane Z;
  f32x16 z[3];
  wing_policy_forward<3>(A, lds, Z, z);
  const unsigned pN = Z.pN, vr = Z.vr;
  const Planes Pac(A.actions, A.NA, pN);
  // actions = sigmoid(z): accumulator rows ARE the action planes
#pragma unroll
  for (int rb = 0; rb < 3; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (rb * 32 + rrow(i) + 4 < kNA)  // rows r(i), r(i) + 4 both < 80; rows >= NA
        Pac.st(vr, (rb * 32 + rrow(i)) * pN, sigmoidf_(z[rb][i]));  // are out of range
}

// ------------------------------------------------------ closed-loop evaluation
// Beyond SURVEY.md §8 (VERDICT r2 "what's missing" #5): FixedWingEvaluator.
// fly_to_point (scripts/evaluate_fixed_wing.py:45-131) for a batch of target
// lists in ONE launch.  Per step: WingDataset.prepare_data
// (neural_control/dataset.py:322-350: ((state - mean) / std)[3:] and the last
// point of the linear reference relative to the aircraft),
// FixedWingNetWrapper.predict_actions (network_wrapper.py:81-98: sigmoid, first
// action of the plan), SimpleWingEnv.step (wing_env.py:44-57: dynamics +
// |roll|, |pitch| < thresh_stable), project_to_line (q_funcs.py:6-18), the
// target switch and either the break (test_time) or the reset onto the line.
// As in the reference, after a reset the POLICY still sees the last simulated
// state (the local `state` of fly_to_point is not refreshed, :124) while the
// environment continues from the reset state.
struct WingLoopArgs {
  const float *targets;  // [n_targets][3][B]
  const float *state0;   // [12][B] or NULL: SimpleWingEnv.zero_reset (:26-28)
  float *div_linear;     // [T][B] distance to the current line after each step
  float *div_pass;       // [T][B] miss distance when a target is passed, else -1
  float *div_fail;       // [T][B] entry appended on divergence, else -1
  int *steps;            // [B] iterations executed = len(drone_traj)
  float *drone;          // [T][16][B] or NULL: state after the step + action
  float *seen;           // [T][15][B] or NULL: state the policy saw + its target
  const float *tables;
  WingGeneralConst k;         // (the full inertia matrix: LearntFixedWingDynamics only)
  float mean[kNS], std[kNS];  // entries 3..11 of the data set's mean / std
  float vec_len, horizon;     // 12 * dt of the data set, its horizon
  float thresh_div, thresh_stable, des_speed;
  int B, T, n_targets, test_time;
};

// a + ab (ab . (p - a)) / |ab|^2, and a itself for a degenerate line
__device__ __forceinline__ void project_to_line(const float (&a)[3], const float (&b)[3],
                                                const float (&p)[3], float (&out)[3]) {
  const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float n2 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2];
  const float d =
      ab[0] * (p[0] - a[0]) + ab[1] * (p[1] - a[1]) + ab[2] * (p[2] - a[2]);
  const float f = n2 > 0.f ? d / n2 : 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = a[j] + ab[j] * f;
}

__device__ __forceinline__ float dist3(const float (&a)[3], const float (&b)[3]) {
  const float x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
  return sqrtf(x * x + y * y + z * z);
}

// LEARNT: the environment steps through LearntFixedWingDynamics.forward
// (neural_control/dynamics/fixed_wing_dynamics.py:270-326): simulate_fixed_wing on
// its CURRENT parameters - the 3 x 3 inertia in full - plus the residual network
// on [state, action] (learnt_residual.h, weights behind the policy tables); what
// SimpleWingEnv(train_dynamics) is after train_dynamics() (scripts/
// train_fixed_wing.py:42-43).  A second instantiation: the analytic loop keeps
// its registers.
template <bool LEARNT>
__global__ __launch_bounds__(kThreads) void wing_closed_loop_kernel(WingLoopArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  fill_lds(lds, A.tables, kFwd16Lds + (LEARNT ? kLearntFloats : 0));
  const LdsView16 L16(lds, threadIdx.x & 63);
  const int lane = threadIdx.x & 63, hi = lane >> 5;
  const LdsView L(lds, lane);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = (blockIdx.x * (kThreads / 64) + wave) * 32 + (lane & 31);
  const int B = A.B, T = A.T;
  const bool live = b < B;
  const unsigned pN = (unsigned)B * 4u;
  // a NULL tensor becomes an empty buffer: loads give 0, stores are dropped
  const Planes Ptg(A.targets, A.n_targets * 3, pN), Ps0(A.state0, A.state0 ? 12 : 0, pN);
  const Planes Pdl(A.div_linear, T, pN), Pdp(A.div_pass, T, pN), Pdf(A.div_fail, T, pN);
  const Planes Pdr(A.drone, A.drone ? T * 16 : 0, pN);
  const Planes Pse(A.seen, A.seen ? T * 15 : 0, pN);
  const unsigned vb = live ? (unsigned)b * 4u : kDead;

  float s[12], obs[12], line[3], prev[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = Ps0.ld(vb, i * pN);
  if (!A.state0) s[3] = kWingDesSpeed;
#pragma unroll
  for (int i = 0; i < 12; ++i) obs[i] = s[i];
#pragma unroll
  for (int j = 0; j < 3; ++j) line[j] = prev[j] = s[j];
  int ti = 0, steps = 0;
  bool alive = live;

#pragma unroll 1
  for (int k = 0; k < T; ++k) {
    const unsigned pB = opaque(pN);
    const unsigned vrec = (alive && hi == 0) ? vb : kDead;
    const unsigned vt = live ? vb + (unsigned)(ti * 3) * pB : kDead;
    float tg[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) tg[j] = Ptg.ld(vt, j * pB);
#pragma unroll
    for (int i = 0; i < 12; ++i) Pse.st(vrec, (k * 15 + i) * pB, obs[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) Pse.st(vrec, (k * 15 + 12 + j) * pB, tg[j]);

    // WingDataset.prepare_data
    float in[kNI];
#pragma unroll
    for (int j = 0; j < kNS; ++j) in[j] = (obs[3 + j] - A.mean[j]) / A.std[j];
    {
      const float rel[3] = {tg[0] - obs[0], tg[1] - obs[1], tg[2] - obs[2]};
      const float nrm = sqrtf(rel[0] * rel[0] + rel[1] * rel[1] + rel[2] * rel[2]);
#pragma unroll
      for (int j = 0; j < 3; ++j)  // last point of _compute_target_pos, then - position
        in[kNS + j] = (obs[j] + (rel[j] / nrm) * A.vec_len * A.horizon) - obs[j];
    }

    // the policy (as wing_policy_fwd_kernel: fp16-split operands on the 16-bit
    // matrix pipe; nothing saved, first head block only)
    f32x16 x[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) x[rb][i] = L.T(hT0 + (rb * 16 + i) * 2);
    {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = hi ? (8 + j < kNI ? in[8 + j < kNI ? 8 + j : 0] : 0.f) : in[j];
      const Op16 xi = split8(v);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) x[rb] = mma3(L16.A(hA, n0 + rb), xi, x[rb]);
    }
    f32x16 u[2], a[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) a[rb][i] = L.T(hT1 + (rb * 16 + i) * 2);
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = tanh_fast(x[kb >> 1][8 * (kb & 1) + j]);
      const Op16 xv = split8(v);
      a[0] = mma3(L16.A(hA, n1 + kb), xv, a[0]);
      a[1] = mma3(L16.A(hA, n1 + 8 + kb), xv, a[1]);
    }
    const auto th = [](int, int, float v) { return tanh_fast(v); };
#pragma unroll
    for (int layer = 0; layer < 2; ++layer) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          u[rb][i] = L.T((layer ? hT3 : hT2) + (rb * 16 + i) * 2);
      dense64_16(u, a, L16, hA, layer ? n3 : n2, th);
      a[0] = u[0], a[1] = u[1];
    }
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = L.T(hTo + i * 2);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = tanh_fast(a[kb >> 1][8 * (kb & 1) + j]);
      z = mma3(L16.A(hA, nO + kb), split8(v), z);
    }
    // head rows 0..3 (the first action of the plan) sit in registers 0..3 of
    // the lower half-wave
    float act[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float oth = other_half(z[j]);
      act[j] = sigmoidf_(hi ? oth : z[j]);
    }

    // SimpleWingEnv.step (sin / cos of the attitude in software: relative accuracy
    // at small angles, wing_math.h sincos_att)
    if (LEARNT) {
      float x[16];
#pragma unroll
      for (int i = 0; i < 12; ++i) x[i] = s[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[12 + j] = act[j];
      wing_step<true>(s, act, A.k);
      learnt_residual_add(s, x, lds + kFwd16Lds, hi);
    } else {
      wing_step<true>(s, act, static_cast<const WingConst &>(A.k));
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) obs[i] = s[i];
    const bool stable =
        fabsf(s[6]) < A.thresh_stable && fabsf(s[7]) < A.thresh_stable;
    const float pos[3] = {s[0], s[1], s[2]};
    float on_line[3];
    project_to_line(line, tg, pos, on_line);
    const float div = dist3(on_line, pos);
    Pdl.st(vrec, k * pB, div);
#pragma unroll
    for (int i = 0; i < 12; ++i) Pdr.st(vrec, (k * 16 + i) * pB, s[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) Pdr.st(vrec, (k * 16 + 12 + j) * pB, act[j]);

    bool done = false;
    float d_pass = -1.f, d_fail = -1.f;
    if (pos[0] > tg[0]) {  // passed the target: miss distance on the last segment
      float on_seg[3];
      project_to_line(prev, pos, tg, on_seg);
      d_pass = dist3(on_seg, tg);
      if (ti < A.n_targets - 1) {
        ++ti;
#pragma unroll
        for (int j = 0; j < 3; ++j) line[j] = pos[j];
      } else {
        done = true;
      }
    }
    if (!done && (!stable || div > A.thresh_div)) {
      d_fail = A.thresh_div;
      if (A.test_time) {
        d_fail = dist3(pos, tg);
        done = true;
      } else {  // continue on the line, flying towards the (old) target
        const float v[3] = {tg[0] - on_line[0], tg[1] - on_line[1], tg[2] - on_line[2]};
        const float vn = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          s[j] = on_line[j];
          s[3 + j] = v[j] / vn * A.des_speed;
          s[6 + j] = 0.f;
          s[9 + j] = 0.f;
        }
      }
    }
    Pdp.st(vrec, k * pB, d_pass);
    Pdf.st(vrec, k * pB, d_fail);
#pragma unroll
    for (int j = 0; j < 3; ++j) prev[j] = pos[j];
    if (alive) steps = k + 1;
    alive = alive && !done;
    if (!__any(alive)) break;
  }
  if (live && hi == 0) A.steps[b] = steps;
}

// ------------------------------------------------------------------ reverse
// k index of head k-pair c (accumulator layout of the 80 outputs: row blocks
// 0 and 1 registers 0..15, row block 2 registers 0..7)
__host__ __device__ constexpr int khead(int c, int hi) {
  return (c >> 4) * 32 + rrow(c & 15) + 4 * hi;
}

// Reverse tables (fp16 split operands): 42 transposed blocks: head^T
// [rb][kb of 5] (this lane's 40 dL/dz rows), fc3^T, fc2^T [rb][kb], fc1^T
// [rb of 4][kb].
constexpr int mOT = 0, m3T = 10, m2T = 18, m1T = 26, mBlocks16 = 42;
constexpr int kBwd16Lds = mBlocks16 * kBlock16 / 4;   // 21 504 floats = 86 016 B

__device__ __forceinline__ float wing_bwd16_weight(const ApgWingPolicy &p, int n, int row,
                                                   int j, int hi, int head_rows) {
  if (n < m3T) {
    const int rb = n / 5, c = (n % 5) * 8 + j;       // dz register c: head row khead(c, hi)
    return khead(c, hi) < head_rows ? p.w_out[khead(c, hi) * kW + rb * 32 + row] : 0.f;
  }
  if (n < m1T) {
    const int m = (n - m3T) % 8, rb = m / 4, k = kin(m % 4, j, hi);
    return n < m2T ? p.w_3[k * kW + rb * 32 + row] : p.w_2[k * kW + rb * 32 + row];
  }
  const int m = n - m1T, rb = m / 4;
  return p.w_1[kin(m % 4, j, hi) * kW0 + rb * 32 + row];
}

__global__ __launch_bounds__(256) void wing_pack_bwd16_kernel(PackArgs A) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, T = gridDim.x * blockDim.x;
  unsigned *dst = reinterpret_cast<unsigned *>(A.dst);
  for (int idx = tid; idx < mBlocks16 * 64 * 4; idx += T) {
    const int q = idx & 3, l = (idx >> 2) & 63, n = idx >> 8;
    unsigned h, lo;
    split_pair(wing_bwd16_weight(A.pol, n, l & 31, 2 * q, l >> 5, A.head_rows),
               wing_bwd16_weight(A.pol, n, l & 31, 2 * q + 1, l >> 5, A.head_rows), h, lo);
    dst[(n * kBlock16) / 4 + l * 4 + q] = h;
    dst[(n * kBlock16 + 1024) / 4 + l * 4 + q] = lo;
  }
}

__global__ __launch_bounds__(kThreads) void wing_policy_bwd_kernel(Args A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  fill_lds(lds, A.tables, kBwd16Lds);
  const int lane = threadIdx.x & 63, hi = lane >> 5;
  const LdsView L(lds, lane);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = (blockIdx.x * (kThreads / 64) + wave) * 32 + (lane & 31);
  const int B = A.B;
  const bool live = b < B;
  const unsigned pN = (unsigned)B * 4u;
  const Planes Pac(A.actions, A.NA, pN), Pga(A.grad_actions, A.NA, pN);
  const Planes Px1(A.x1, kW0, pN), Ph(A.h, 3 * kW, pN);
  const Planes Pdz(A.d_zout, A.NA, pN), Pdp(A.d_pre, 3 * kW + kW0, pN);
  const unsigned vb = live ? (unsigned)b * 4u : kDead;
  const unsigned vr = live ? vb + (hi ? 4u * pN : 0u) : kDead;

  // dL/dz = dL/da * a (1 - a), 40 k-pairs in accumulator layout (rows beyond
  // NA are outside the buffers: they load 0 and their stores are dropped)
  float dz[40];
#pragma unroll
  for (int c = 0; c < 40; ++c) {
    const float a = Pac.ld(vr, khead(c, 0) * pN), g = Pga.ld(vr, khead(c, 0) * pN);
    dz[c] = g * a * (1.f - a);
    Pdz.st(vr, khead(c, 0) * pN, dz[c]);
  }
  float hv[2][16];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) hv[rb][i] = Ph.ld(vr, (2 * kW + rb * 32 + rrow(i)) * pN);
  __builtin_amdgcn_sched_barrier(0);
  // the reverse layers on the 16-bit matrix pipe: cotangents scaled per
  // trajectory, two fp16 terms, three products per k-block
  const LdsView16 L16(lds, lane);
  f32x16 d[2], e[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) d[rb][i] = 0.f;
  int ex;
  {  // dL/dh3 = W_out^T dL/dz: this lane's 40 rows = 5 k-blocks
    float amax = 0.f;
#pragma unroll
    for (int c = 0; c < 40; ++c) amax = fmaxf(amax, fabsf(dz[c]));
    ex = scale_exponent(amax);
#pragma unroll
    for (int kb = 0; kb < 5; ++kb) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = __builtin_amdgcn_ldexpf(dz[kb * 8 + j], -ex);
      const Op16 xv = split8(v);
      d[0] = mma3(L16.A(0, mOT + kb), xv, d[0]);
      d[1] = mma3(L16.A(0, mOT + 5 + kb), xv, d[1]);
    }
  }
  Op16 xs[4];
  // fc3, fc2: v = 2^ex v (1 - act^2), store, multiply by the transposed weights
#pragma unroll
  for (int layer = 2; layer >= 1; --layer) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        d[rb][i] = __builtin_amdgcn_ldexpf(d[rb][i], ex) * (1.f - hv[rb][i] * hv[rb][i]);
        Pdp.st(vr, (layer * kW + rb * 32 + rrow(i)) * pN, d[rb][i]);  // d_pre fc3 / fc2
      }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        hv[rb][i] = Ph.ld(vr, ((layer - 1) * kW + rb * 32 + rrow(i)) * pN);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) e[rb][i] = 0.f;
    ex = scaled_split64(d, xs);
    dense64T_16(e, xs, L16, 0, layer == 2 ? m3T : m2T);
    d[0] = e[0], d[1] = e[1];
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      d[rb][i] = __builtin_amdgcn_ldexpf(d[rb][i], ex) * (1.f - hv[rb][i] * hv[rb][i]);
      Pdp.st(vr, (rb * 32 + rrow(i)) * pN, d[rb][i]);  // d_pre fc1
    }
  // first layer: 128 outputs, then tanh' from the saved x1
  float xv[4][16];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) xv[rb][i] = Px1.ld(vr, (rb * 32 + rrow(i)) * pN);
  __builtin_amdgcn_sched_barrier(0);
  ex = scaled_split64(d, xs);
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    f32x16 y;
#pragma unroll
    for (int i = 0; i < 16; ++i) y[i] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) y = mma3(L16.A(0, m1T + rb * 4 + kb), xs[kb], y);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      Pdp.st(vr, (3 * kW + rb * 32 + rrow(i)) * pN,
             __builtin_amdgcn_ldexpf(y[i], ex) * (1.f - xv[rb][i] * xv[rb][i]));  // d_pre first layer
  }
}

// ------------------------ the controller step through the learnt simulator --
// The controller phase of the adapt flow (TrainFixedWing.train_controller_model,
// scripts/train_fixed_wing.py:90-116, behind the concurrent policy of
// scripts/train_base.py:198-209, with LearntFixedWingDynamics,
// neural_control/dynamics/fixed_wing_dynamics.py:270-326, as train dynamics) in
// ONE forward kernel: the policy (wing_policy_forward), H = 10 steps of
//   s' = simulate_fixed_wing(s, a; live theta, full I) + W2 relu(W1 [s; a] + b1) + b2,
// fixed_wing_mpc_loss and the reverse sweep down to dL/dactions, which leaves as
// the planes wing_policy_bwd_kernel starts from.  Geometry of
// wing_policy_fwd_kernel; both half-waves of a trajectory run the rollout
// (wing_rollout_math.h), each with 32 of the residual's 64 hidden units
// (learnt_residual.h).  The simulator is frozen: nothing is produced for it.
//   LDS     [0, 100 352) the policy tables, dead once every wave has its head;
//           [0, 122 880) over them the ten pre-step states [k][12][256];
//           [122 880, 130 560) the packed residual, from the start.
//   actions the head's accumulators, sigmoid applied, stay in 20 registers per
//           lane: rows 4 k .. 4 k + 3 of step k = 2 q + h are registers 4 q ..
//           4 q + 3 of half-wave h; the other half takes them by other_half.
//           The step loops stay rolled (k is a scalar: the pick is a chain of
//           selects), so one step's registers serve all ten.
//   table   the step's constants (wing_learnt_table, built on the device by the
//           pack launch) are read where they are used through the constant
//           address space, as wing_learnt_rollout_kernel reads them.
constexpr int kLpH = 10, kLpNA = 4 * kLpH;
constexpr int kLpPre = kLpH * 12 * kTrajPerBlock;   // 30 720 floats
constexpr int kLpLds = kLpPre + kLearntFloats;      // 32 640 floats = 130 560 B
static_assert(kFwd16Lds <= kLpPre, "the pre-states lie over the dead policy tables");
static_assert(kLpPre % 4 == 0 && kLpLds * 4 <= 160 * 1024, "LDS");

struct WingLearntPolicyArgs {
  Args P;                      // feat, ref_in, actions, x1, h, tables, B, NA = 40
  const float *state0, *ref;   // [12][B], [H][3][B]
  float *grad_actions;         // [40][B]
  float *states;               // [H][12][B] or NULL
  float *loss_partials;        // one per wave = 32 trajectories
  const float *sim;            // the step table (WingGeneralConst)
  const float *learnt;         // the packed residual (learnt_pack_kernel)
  ApgWingLossWeights w;
  int H;
};

__global__ __launch_bounds__(kThreads) void wing_learnt_policy_fwd_kernel(
    WingLearntPolicyArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  fill_lds_issue(lds + kLpPre, A.learnt, kLearntFloats);
  fill_lds(lds, A.P.tables, kFwd16Lds);   // (waits for both)
  WingLane Z;
  f32x16 z[2];
  wing_policy_forward<2>(A.P, lds, Z, z);
  const int hi = Z.hi;
  const unsigned pN = Z.pN, vb = Z.vb, vr = Z.vr;
  const unsigned vb_lo = Z.live && hi == 0 ? vb : kDead;
  const Planes Pac(A.P.actions, kLpNA, pN), Pga(A.grad_actions, kLpNA, pN);
  const Planes Ps0(A.state0, 12, pN), Prf(A.ref, kLpH * 3, pN);
  const Planes Pst(A.states, A.states ? kLpH * 12 : 0, pN);
  // own[4 q + j]: action j of step 2 q + hi (head row 8 q + 4 hi + j)
  float own[20];
#pragma unroll
  for (int cc = 0; cc < 20; ++cc) {
    own[cc] = sigmoidf_(cc < 16 ? z[0][cc] : z[1][cc - 16]);
    Pac.st(vr, khead(cc, 0) * pN, own[cc]);
  }
  float s[12], lam[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = Ps0.ld(vb, i * pN);
  __syncthreads();   // every wave is done with the policy tables
  const int tl = (threadIdx.x >> 6) * 32 + (threadIdx.x & 31);
  float *pre_at = lds + tl;     // + (k * 12 + i) * 256: this trajectory's pre-states
  const float *lr = lds + kLpPre;
  WingGeneralConstK *kp = (WingGeneralConstK *)A.sim;
  // (stops the compiler from hoisting the table's scalar loads out of the step
  // loops, where they would not fit the SGPR file)
#define APG_LAUNDER(p) asm volatile("" : "+s"(p))
  const int H = A.H;
  auto action = [&](int k, float (&a)[4]) {
    const int q = k >> 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = own[16 + j];
#pragma unroll
      for (int c = 3; c >= 0; --c) {
        // (opaque: left to itself the compiler folds the chain into ONE load at a
        // computed index, which puts `own` into scratch)
        float cand = own[4 * c + j];
        asm volatile("" : "+v"(cand));
        v = q == c ? cand : v;
      }
      const float oth = other_half(v);
      a[j] = (k & 1) == hi ? v : oth;
    }
  };
  auto ref = [&](int k, float (&rp)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) rp[i] = Prf.ld(vb, (unsigned)(k * 3 + i) * pN);
  };
  auto ST = [&](int k, int i) -> float & { return pre_at[(k * 12 + i) * kTrajPerBlock]; };
  const float loss = wing_rollout_forward(
      H, s, A.w.pos, A.w.action, action, ref, ST,
      [&](float (&x)[12], const float (&a)[4]) {
        APG_LAUNDER(kp);
        float xin[16];
#pragma unroll
        for (int i = 0; i < 12; ++i) xin[i] = x[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) xin[12 + j] = a[j];
        wing_step(x, a, *kp);
        learnt_residual_add(x, xin, lr, hi);
      },
      [&](int k, const float (&x)[12]) {
#pragma unroll
        for (int i = 0; i < 12; ++i) Pst.st(vb_lo, (unsigned)(k * 12 + i) * pN, x[i]);
      });
  wing_rollout_reverse(
      H, s, lam, A.w.pos, A.w.action, action, ref, ST,
      [&](float (&l)[12], float (&ga)[4], const float (&pre)[12], const float (&a)[4]) {
        APG_LAUNDER(kp);
        float xin[16], gx[16], sd[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) xin[i] = pre[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) xin[12 + j] = a[j];
        learnt_residual_adjoint(gx, l, xin, lr, hi);   // (before l is overwritten)
        WingAux x;
        wing_rates(pre, a, *kp, x, sd);
        NoWingParamGrads none;
        wing_step_adjoint(l, ga, pre, x, sd, *kp, none);
#pragma unroll
        for (int i = 0; i < 12; ++i) l[i] += gx[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) ga[j] += gx[12 + j];
      },
      [&](int k, const float (&ga)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Pga.st(vb_lo, (unsigned)(k * 4 + j) * pN, ga[j]);
      });
#undef APG_LAUNDER
  write_wave_partial(A.loss_partials, vb_lo != kDead ? loss : 0.f, (A.P.B + 31) / 32);
}

// the flat gradient of the step (include/apg.h, APG_WING_POLICY_G_*): the twelve
// tensors in ApgWingPolicy order for H = 10
__host__ __device__ constexpr int pol_size(int t) {
  return t == 0 ? kW * kNS : t == 2 ? kW * kNR : t == 4 ? kW * kW0
         : (t == 6 || t == 8) ? kW * kW : t == 10 ? kLpNA * kW : t == 11 ? kLpNA : kW;
}
__host__ __device__ constexpr int pol_at(int t) {
  int at = 0;
  for (int i = 0; i < t; ++i) at += pol_size(i);
  return at;
}
static_assert(pol_at(0) == APG_WING_POLICY_G_W_S && pol_at(1) == APG_WING_POLICY_G_B_S &&
                  pol_at(2) == APG_WING_POLICY_G_W_R && pol_at(3) == APG_WING_POLICY_G_B_R &&
                  pol_at(4) == APG_WING_POLICY_G_W_1 && pol_at(5) == APG_WING_POLICY_G_B_1 &&
                  pol_at(6) == APG_WING_POLICY_G_W_2 && pol_at(7) == APG_WING_POLICY_G_B_2 &&
                  pol_at(8) == APG_WING_POLICY_G_W_3 && pol_at(9) == APG_WING_POLICY_G_B_3 &&
                  pol_at(10) == APG_WING_POLICY_G_W_OUT &&
                  pol_at(11) == APG_WING_POLICY_G_B_OUT && pol_at(12) == APG_WING_POLICY_GRADS,
              "apg.h publishes these offsets");

// The step's workspace: [forward tables | packed residual | step table |
// reverse tables | column descriptors of the weight products | products' scratch]
constexpr int wsFwd = 0, wsLr = wsFwd + kFwd16Lds, wsSim = wsLr + kLearntFloats,
              wsBwd = wsSim + kWingLearntTableFloats, wsDesc = wsBwd + kBwd16Lds,
              kDescInts = 256, wsGemm = wsDesc + kDescInts;
constexpr int dJ64 = 0, dJ9 = 192, dJ3 = 219;   // [3][J] each: plane, two strides (0)
constexpr int kLpGroupWgs = 256;
static_assert(wsLr % 4 == 0 && wsBwd % 4 == 0, "16-byte rows for the DMA");

// the step table from the module's live tensors (wing_learnt_rollout_pack_kernel's)
// and the descriptors: column j of a product is plane j behind its first one
__global__ __launch_bounds__(256) void wing_learnt_policy_pack_kernel(ApgWingLearnt m, float dt,
                                                                      float *__restrict__ sim,
                                                                      int *__restrict__ desc) {
  const int t = threadIdx.x;
  if (t == 0) {
    *reinterpret_cast<WingGeneralConst *>(sim) = wing_learnt_table(m.theta, m.inertia, dt);
    for (int i = (int)(sizeof(WingGeneralConst) / sizeof(float)); i < kWingLearntTableFloats; ++i)
      sim[i] = 0.f;
  }
  if (t < dJ9) desc[t] = t < 64 ? t : 0;
  else if (t < dJ3) desc[t] = t - dJ9 < 9 ? t - dJ9 : 0;
  else if (t < kDescInts) desc[t] = t - dJ3 < 3 ? t - dJ3 : 0;
}

// torch.optim.SGD on the twelve tensors: buf = momentum buf + grad, p -= lr buf,
// in double, rounded once each (as the quadrotor's second stage, mlp_common.h)
struct WingSgdArgs {
  const float *g[12];
  float *p[12], *m[12];
  double lr, momentum;
};

__global__ __launch_bounds__(256) void wing_policy_sgd_kernel(WingSgdArgs A) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= pol_at(12)) return;
  const float *g = nullptr;
  float *p = nullptr, *m = nullptr;
#pragma unroll
  for (int t = 0; t < 12; ++t)
    if (idx >= pol_at(t) && idx < pol_at(t + 1)) {
      g = A.g[t] + (idx - pol_at(t));
      p = A.p[t] + (idx - pol_at(t));
      m = A.m[t] + (idx - pol_at(t));
    }
  const float buf = (float)(A.momentum * (double)*m + (double)*g);
  *m = buf;
  *p = (float)((double)*p - A.lr * (double)buf);
}

inline void pointers_of(const ApgWingPolicyGrads &g, float *(&out)[12]) {
  float *v[12] = {g.w_s, g.b_s, g.w_r, g.b_r, g.w_1, g.b_1,
                  g.w_2, g.b_2, g.w_3, g.b_3, g.w_out, g.b_out};
  for (int t = 0; t < 12; ++t) out[t] = v[t];
}

inline bool all_set(const ApgWingPolicyGrads &g) {
  float *v[12];
  pointers_of(g, v);
  for (int t = 0; t < 12; ++t)
    if (!v[t]) return false;
  return true;
}

// the seven weight-gradient products of the step (H = 10: the head is one):
// cotangent planes x activation planes, as functional.wing_concurrent_policy_grads
// states them.  acts: feat 0..8 | ref 9..11 | x1 12..139 | h1 140.. | h2 204.. |
// h3 268..; cot: d_zout 0..39 | d_pre fc1, fc2, fc3 (64 each), first layer (128)
constexpr int kLpProducts = 7;
void wing_lp_products(const float *acts, const float *cot, float *const (&g)[12],
                      const int *desc, long long B, ApgGemmProblem (&q)[kLpProducts]) {
  // (acts / cot NULL: the shapes only, for the workspace size)
  const auto set = [&](int p, int cot_plane, int M, int plane, int J, const int *d,
                       float *C, int ldc, float *bias, bool ones) {
    q[p].A = cot ? cot + cot_plane * B : nullptr;
    q[p].B = acts ? acts + plane * B : nullptr;
    q[p].bdesc = d, q[p].C = C, q[p].bias_out = bias;
    q[p].N = B, q[p].M = M, q[p].S = 1, q[p].J = J, q[p].sdiv = 1;
    q[p].with_ones = ones, q[p].b_planes = J, q[p].ldc = ldc;
  };
  const int dp = kLpNA;   // d_pre's first plane
  set(0, 0, kLpNA, 268, kW, desc + dJ64, g[10], kW, g[11], true);
  set(1, dp + 128, kW, 204, kW, desc + dJ64, g[8], kW, g[9], true);
  set(2, dp + 64, kW, 140, kW, desc + dJ64, g[6], kW, g[7], true);
  set(3, dp, kW, 12, kW, desc + dJ64, g[4], kW0, nullptr, false);
  set(4, dp, kW, 76, kW, desc + dJ64, g[4] ? g[4] + kW : nullptr, kW0, g[5], true);
  set(5, dp + 192, kW, 0, kNS, desc + dJ9, g[0], kNS, g[1], true);
  set(6, dp + 256, kW, kNS, kNR, desc + dJ3, g[2], kNR, g[3], true);
}

// functional._run_products' rule: few columns - all products in one launch pair
inline bool lp_grouped(long long B) { return kLpProducts * B <= 8 * 8192 && B <= 131072; }

int check_wing_horizon(int H) {
  if (H != 10 && H != 20) {
    set_error("the fused fixed-wing policy is built for horizon 10 or 20 (got %d)", H);
    return APG_ERR_ARG;
  }
  return APG_OK;
}

int check_wing_policy(const ApgWingPolicy *pol, int B) {
  if (!pol) { set_error("policy is NULL"); return APG_ERR_ARG; }
  if (B < 0) { set_error("B must be >= 0 (got %d)", B); return APG_ERR_ARG; }
  if ((long long)B * 4 * 320 >= (1ll << 32) - 64) {
    set_error("B too large for 32-bit plane offsets; split the batch");
    return APG_ERR_ARG;
  }
  if (!pol->w_s || !pol->b_s || !pol->w_r || !pol->b_r || !pol->w_1 || !pol->b_1 ||
      !pol->w_2 || !pol->b_2 || !pol->w_3 || !pol->b_3 || !pol->w_out || !pol->b_out) {
    set_error("policy weight pointer is NULL");
    return APG_ERR_ARG;
  }
  return APG_OK;
}

template <typename K>
int raise_lds(K kernel, int floats) {
  if (hipFuncSetAttribute((const void *)kernel,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(floats * sizeof(float))) != hipSuccess)
    return check_launch("hipFuncSetAttribute(wing_policy)");
  return APG_OK;
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_wing_policy_workspace_floats(void) {
  // (+ the packed residual network of a learnt environment's closed loop)
  return (kFwd16Lds > kBwd16Lds ? kFwd16Lds : kBwd16Lds) + kLearntFloats;
}

int apg_wing_policy_fwd(const float *feat, const float *ref_in,
                        const ApgWingPolicy *policy, int B, int H, float *actions,
                        float *x1, float *h, float *workspace,
                        apg_stream_t stream) {
  if (int e = check_wing_policy(policy, B)) return e;
  if (int e = check_wing_horizon(H)) return e;
  if (B == 0) return APG_OK;
  if (!feat || !ref_in || !actions || !x1 || !h || !workspace) {
    set_error("NULL buffer");
    return APG_ERR_ARG;
  }
  static PerDeviceOnce attr;
  if (!attr.test()) {
    if (int e = raise_lds(wing_policy_fwd_kernel, kFwd16Lds)) return e;
    attr.set();
  }
  Args A = {};
  A.feat = feat, A.ref_in = ref_in, A.actions = actions, A.x1 = x1, A.h = h;
  A.tables = workspace, A.B = B, A.NA = 4 * H;
  PackArgs P;
  P.pol = *policy, P.dst = workspace, P.head_rows = 4 * H;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wing_pack_fwd16_kernel, dim3((kFwd16Lds + 255) / 256), dim3(256), 0,
                     st, P);
  hipLaunchKernelGGL(wing_policy_fwd_kernel,
                     dim3((B + kTrajPerBlock - 1) / kTrajPerBlock), dim3(kThreads),
                     kFwd16Lds * sizeof(float), st, A);
  return check_launch("wing_policy_fwd");
}

int apg_wing_policy_bwd(const float *actions, const float *grad_actions,
                        const float *x1, const float *h,
                        const ApgWingPolicy *policy, int B, int H, float *d_zout,
                        float *d_pre, float *workspace, apg_stream_t stream) {
  if (int e = check_wing_policy(policy, B)) return e;
  if (int e = check_wing_horizon(H)) return e;
  if (B == 0) return APG_OK;
  if (!actions || !grad_actions || !x1 || !h || !d_zout || !d_pre || !workspace) {
    set_error("NULL buffer");
    return APG_ERR_ARG;
  }
  static PerDeviceOnce attr;
  if (!attr.test()) {
    if (int e = raise_lds(wing_policy_bwd_kernel, kBwd16Lds)) return e;
    attr.set();
  }
  Args A = {};
  A.actions = const_cast<float *>(actions), A.grad_actions = grad_actions;
  A.x1 = const_cast<float *>(x1), A.h = const_cast<float *>(h);
  A.d_zout = d_zout, A.d_pre = d_pre, A.tables = workspace, A.B = B, A.NA = 4 * H;
  PackArgs P;
  P.pol = *policy, P.dst = workspace, P.head_rows = 4 * H;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wing_pack_bwd16_kernel, dim3((kBwd16Lds + 255) / 256), dim3(256), 0,
                     st, P);
  hipLaunchKernelGGL(wing_policy_bwd_kernel,
                     dim3((B + kTrajPerBlock - 1) / kTrajPerBlock), dim3(kThreads),
                     kBwd16Lds * sizeof(float), st, A);
  return check_launch("wing_policy_bwd");
}

int apg_wing_mlp_closed_loop(const ApgWingFlight *flight, float dt,
                             const ApgWingParams *params, const float *inertia,
                             const ApgLearntResidual *learnt, const ApgWingPolicy *policy,
                             const float *mean, const float *std, float data_dt,
                             int data_horizon, int B, float *workspace, apg_stream_t stream) {
  if (int e = check_wing_policy(policy, B)) return e;
  if ((inertia != nullptr) != (learnt != nullptr)) {
    set_error("learnt environment: `inertia` and `learnt` come together");
    return APG_ERR_ARG;
  }
  if (learnt && (!learnt->w1 || !learnt->b1 || !learnt->w2 || !learnt->b2)) {
    set_error("learnt simulator: weight pointer is NULL");
    return APG_ERR_ARG;
  }
  if (!params || !mean || !std) {
    set_error("params / mean / std is NULL");
    return APG_ERR_ARG;
  }
  WingFlightRule rule;
  if (const char *e = wing_flight_check(flight, B, &rule)) {
    set_error("%s", e);
    return APG_ERR_ARG;
  }
  // this loop's own rules: no step is a no-op, plane offsets are 32-bit, the
  // tables need a workspace
  const int n_targets = rule.n_targets, max_steps = rule.T;
  if (max_steps < 0 || data_horizon < 1) {
    set_error("max_steps >= 0, data_horizon >= 1 (got %d, %d)", max_steps, data_horizon);
    return APG_ERR_ARG;
  }
  const long long widest = 16ll * max_steps > 3ll * n_targets ? 16ll * max_steps
                                                              : 3ll * n_targets;
  if ((long long)B * 4 * widest >= (1ll << 32) - 64) {
    set_error("B x max_steps too large for 32-bit plane offsets; split the batch");
    return APG_ERR_ARG;
  }
  if (B == 0 || max_steps == 0) return APG_OK;
  if (!workspace) {
    set_error("NULL buffer");
    return APG_ERR_ARG;
  }
  static PerDeviceOnce attr;
  if (!attr.test()) {
    if (int e = raise_lds(wing_closed_loop_kernel<false>, kFwd16Lds)) return e;
    if (int e = raise_lds(wing_closed_loop_kernel<true>, kFwd16Lds + kLearntFloats)) return e;
    attr.set();
  }
  WingLoopArgs A = {};
  A.targets = flight->targets, A.state0 = flight->state0;
  A.div_linear = flight->div_linear, A.div_pass = flight->div_pass;
  A.div_fail = flight->div_fail, A.steps = flight->steps, A.drone = flight->drone;
  A.seen = flight->seen, A.tables = workspace;
  if (learnt) A.k = make_general_const(*params, dt, inertia);
  else static_cast<WingConst &>(A.k) = make_const(*params, dt);
  for (int j = 0; j < kNS; ++j) A.mean[j] = mean[3 + j], A.std[j] = std[3 + j];
  // `ref_vector * vec_len_per_step * (i + 1)`: the Python double 12 * dt enters
  // the float32 tensor product rounded to float32 (dataset.py:312-319)
  A.vec_len = (float)(12.0 * (double)data_dt), A.horizon = (float)data_horizon;
  A.thresh_div = rule.thresh_div, A.thresh_stable = rule.thresh_stable;
  A.des_speed = rule.des_speed;
  A.B = B, A.T = max_steps, A.n_targets = n_targets, A.test_time = flight->test_time;
  PackArgs P;
  P.pol = *policy, P.dst = workspace, P.head_rows = 4;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wing_pack_fwd16_kernel, dim3((kFwd16Lds + 255) / 256), dim3(256), 0,
                     st, P);
  const dim3 grid((B + kTrajPerBlock - 1) / kTrajPerBlock);
  if (learnt) {
    hipLaunchKernelGGL(learnt_pack_kernel, dim3((kLearntFloats + 255) / 256), dim3(256), 0, st,
                       *learnt, workspace + kFwd16Lds);
    hipLaunchKernelGGL(wing_closed_loop_kernel<true>, grid, dim3(kThreads),
                       (kFwd16Lds + kLearntFloats) * sizeof(float), st, A);
  } else {
    hipLaunchKernelGGL(wing_closed_loop_kernel<false>, grid, dim3(kThreads),
                       kFwd16Lds * sizeof(float), st, A);
  }
  return check_launch("wing_mlp_closed_loop");
}

int apg_wing_learnt_mlp_step_workspace_floats(int B) {
  if (B <= 0) return 0;
  long long scratch = (long long)kLpGroupWgs * 64 * 128;
  if (!lp_grouped(B)) {
    float *const none[12] = {};
    ApgGemmProblem q[kLpProducts];
    static const int no_desc[kDescInts] = {};
    wing_lp_products(nullptr, nullptr, none, no_desc, B, q);
    scratch = apg_planes_gemm_multi_workspace_floats(q, kLpProducts);
  }
  return (int)(wsGemm + scratch);
}

int apg_wing_learnt_mlp_train_step(
    const float *feat, const float *ref_in, const float *state0, const float *ref,
    float dt, const ApgWingLearnt *model, const ApgWingLossWeights *weights,
    const ApgWingPolicy *policy, int B, int H,
    float *acts, float *cot, float *loss_partials, float *loss,
    const ApgWingPolicyGrads *grads, float *states, float *workspace,
    const ApgWingSgdUpdate *update, apg_stream_t stream) {
  if (!model || !model->theta || !model->inertia || !model->w1 || !model->b1 || !model->w2 ||
      !model->b2) {
    set_error("model or one of its pointers is NULL");
    return APG_ERR_ARG;
  }
  if (int e = check_wing_policy(policy, B)) return e;
  if (H != kLpH) {
    set_error("the fused learnt-simulator step is built for horizon 10 (got %d)", H);
    return APG_ERR_ARG;
  }
  if ((long long)B * 4 * (332 + 2 * kLpNA) >= (1ll << 32) - 64) {
    set_error("B too large for 32-bit plane offsets; split the batch");
    return APG_ERR_ARG;
  }
  if (!weights) { set_error("weights is NULL"); return APG_ERR_ARG; }
  if (!grads || !all_set(*grads)) {
    set_error("gradient pointer is NULL");
    return APG_ERR_ARG;
  }
  if (update) {
    if (!all_set(update->param) || !all_set(update->momentum_buf)) {
      set_error("update: parameter / momentum pointer is NULL");
      return APG_ERR_ARG;
    }
    // (NaN fails both comparisons)
    if (!(update->lr >= 0.0 && update->lr < HUGE_VAL) ||
        !(update->momentum >= 0.0 && update->momentum < HUGE_VAL)) {
      set_error("update: lr and momentum must be finite and >= 0");
      return APG_ERR_ARG;
    }
    // (an update with zero gradients would still move the parameters by the
    // decaying momentum: not implemented)
    if (B == 0) {
      set_error("update with B = 0 is not supported");
      return APG_ERR_ARG;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  float *g[12];
  pointers_of(*grads, g);
  if (B == 0) {   // no trajectory: zero gradients, zero loss
    for (int t = 0; t < 12; ++t)
      if (hipMemsetAsync(g[t], 0, pol_size(t) * sizeof(float), st) != hipSuccess)
        return check_launch("memset(grads)");
    if (loss && hipMemsetAsync(loss, 0, sizeof(float), st) != hipSuccess)
      return check_launch("memset(loss)");
    return APG_OK;
  }
  if (!feat || !ref_in || !state0 || !ref || !acts || !cot || !loss_partials || !workspace) {
    set_error("NULL buffer");
    return APG_ERR_ARG;
  }
  static PerDeviceOnce attr;
  if (!attr.test()) {
    if (int e = raise_lds(wing_learnt_policy_fwd_kernel, kLpLds)) return e;
    if (int e = raise_lds(wing_policy_bwd_kernel, kBwd16Lds)) return e;
    attr.set();
  }
  const size_t plane = (size_t)B;
  float *x1 = acts + 12 * plane, *h = acts + 140 * plane;
  float *actions = acts + 332 * plane, *grad_actions = actions + kLpNA * plane;
  int *desc = reinterpret_cast<int *>(workspace + wsDesc);
  // 1. the tables, from the tensors as they are when the launches run
  PackArgs P;
  P.pol = *policy, P.head_rows = kLpNA;
  P.dst = workspace + wsFwd;
  hipLaunchKernelGGL(wing_pack_fwd16_kernel, dim3((kFwd16Lds + 255) / 256), dim3(256), 0,
                     st, P);
  const ApgLearntResidual res = {nullptr, model->w1, model->b1, model->w2, model->b2};
  hipLaunchKernelGGL(learnt_pack_kernel, dim3((kLearntFloats + 255) / 256), dim3(256), 0, st,
                     res, workspace + wsLr);
  hipLaunchKernelGGL(wing_learnt_policy_pack_kernel, dim3(1), dim3(256), 0, st, *model, dt,
                     workspace + wsSim, desc);
  P.dst = workspace + wsBwd;
  hipLaunchKernelGGL(wing_pack_bwd16_kernel, dim3((kBwd16Lds + 255) / 256), dim3(256), 0,
                     st, P);
  // 2. policy, rollout, loss, adjoint
  const dim3 grid((B + kTrajPerBlock - 1) / kTrajPerBlock);
  WingLearntPolicyArgs F = {};
  F.P.feat = feat, F.P.ref_in = ref_in, F.P.actions = actions, F.P.x1 = x1, F.P.h = h;
  F.P.tables = workspace + wsFwd, F.P.B = B, F.P.NA = kLpNA;
  F.state0 = state0, F.ref = ref, F.grad_actions = grad_actions, F.states = states;
  F.loss_partials = loss_partials, F.sim = workspace + wsSim, F.learnt = workspace + wsLr;
  F.w = *weights, F.H = H;
  hipLaunchKernelGGL(wing_learnt_policy_fwd_kernel, grid, dim3(kThreads),
                     kLpLds * sizeof(float), st, F);
  // 3. the policy's reverse pass
  Args R = {};
  R.actions = actions, R.grad_actions = grad_actions, R.x1 = x1, R.h = h;
  R.d_zout = cot, R.d_pre = cot + kLpNA * plane, R.tables = workspace + wsBwd;
  R.B = B, R.NA = kLpNA;
  hipLaunchKernelGGL(wing_policy_bwd_kernel, grid, dim3(kThreads), kBwd16Lds * sizeof(float),
                     st, R);
  if (int e = check_launch("wing_learnt_mlp_train_step")) return e;
  // 4. the weight gradients, straight into `grads`
  ApgGemmProblem q[kLpProducts];
  wing_lp_products(acts, cot, g, desc, B, q);
  if (int e = lp_grouped(B)
                  ? apg_planes_gemm_grouped(q, kLpProducts, workspace + wsGemm, kLpGroupWgs, stream)
                  : apg_planes_gemm_multi(q, kLpProducts, workspace + wsGemm, stream))
    return e;
  // 5. the loss
  if (loss)
    if (int e = launch_reduce_partials(loss_partials, (B + 31) / 32, loss, st)) return e;
  // 6. the optimizer
  if (update) {
    WingSgdArgs S;
    float *p[12], *m[12];
    pointers_of(update->param, p);
    pointers_of(update->momentum_buf, m);
    for (int t = 0; t < 12; ++t) S.g[t] = g[t], S.p[t] = p[t], S.m[t] = m[t];
    S.lr = update->lr, S.momentum = update->momentum;
    hipLaunchKernelGGL(wing_policy_sgd_kernel, dim3((pol_at(12) + 255) / 256), dim3(256), 0,
                       st, S);
    return check_launch("wing_policy_sgd");
  }
  return APG_OK;
}


}  // extern "C"
