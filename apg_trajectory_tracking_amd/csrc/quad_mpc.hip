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
// The same solver with the LEARNT simulator as its model
// (apg_quad_learnt_mpc_solve, apg_quad_learnt_mpc_closed_loop;
// quad_learnt_mpc_math.h): the model's packed weights and the pre-step states of
// the forward sweep live in LDS, everything else as above; the residual is a
// 16 -> 64 -> 12 network per trajectory on per-lane inputs - no MFMA either
// (DESIGN.md §7).
#include "learnt_residual.h"
#include "quad_learnt_mpc_math.h"
#include "static_dispatch.h"

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

// one solve of trajectory b on `model` (quad_mpc_math.h: a model of the solver)
template <int H, class Model>
__device__ __forceinline__ void mpc_solve_lane(const MpcSolveArgs &A, int b, const Model &model) {
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
  const float J = mpc_solve<H>(s0, ref, u, model, A.w, A.o, [&](int i, float Ji) {
    if (trace) trace[(size_t)i * B + b] = Ji;
  });
  A.cost_out[b] = J;
#pragma unroll
  for (int k = 0; k < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) A.u[((size_t)k * 4 + j) * B + b] = u[k][j];
}

template <int H>
__global__ __launch_bounds__(kMpcThreads) void quad_mpc_solve_kernel(MpcSolveArgs A) {
  const int b = blockIdx.x * kMpcThreads + threadIdx.x;
  if (b >= A.B) return;
  mpc_solve_lane<H>(A, b, MpcAnalytic{A.c});
}

// The learnt model's kernels keep two things in LDS: the model's packed block
// (learnt_pack.h, 7.7 KB) and, behind it, the lanes' pre-step states of the
// forward sweep, [H][12][64 lanes] (H = 10: 30 KB) - 37.5 KB per one-wave
// workgroup, four workgroups per CU.
template <int H>
constexpr int kLearntMpcLds = kLearntFloats + H * kMpcPreRow * kMpcThreads;
static_assert(4 * kLearntMpcLds<10> * sizeof(float) <= 160 * 1024, "four workgroups per CU");
static_assert(kMpcPreStride == kMpcThreads || kMpcPreStride == 1, "one wave per workgroup");

// lds <- the packed block at `packed`; -> the solver's model for this lane
__device__ __forceinline__ MpcLearnt<const float *> learnt_model_in_lds(float *lds,
                                                                         const float *packed,
                                                                         const QuadConst &c) {
  for (int i = threadIdx.x; i < kLearntFloats; i += kMpcThreads) lds[i] = packed[i];
  __syncthreads();
  return MpcLearnt<const float *>{c, lds, lds + kLearntFloats + threadIdx.x};
}

template <int H>
__global__ __launch_bounds__(kMpcThreads) void quad_learnt_mpc_solve_kernel(
    MpcSolveArgs A, const float *packed) {
  __shared__ float lds[kLearntMpcLds<H>];
  const MpcLearnt<const float *> model = learnt_model_in_lds(lds, packed, A.c);
  const int b = blockIdx.x * kMpcThreads + threadIdx.x;
  if (b >= A.B) return;
  mpc_solve_lane<H>(A, b, model);
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

// mpc_flight (quad_mpc_math.h), one flight per lane.  (The lane body stands in
// both closed-loop kernels: moved into one __forceinline__ function - by
// reference or by value, with the plant step passed in or built inside - hipcc
// schedules all four instantiations differently, the learnt-model ones by 300
// instructions; they are kept as measured.)
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
        if (LEARNT) learnt_quad_step_lane(s, u0, A.cp, t, (const float *)lr);
        else quad_step(s, u0, A.cp, t);
      },
      MpcAnalytic{A.cm}, A.w, A.o, A.rule, log);
}

// The same flight with the solver planning on the learnt model (`packed`: its
// block, into LDS).  The plant's block - another module's, or the same one's -
// stays where learnt_pack_kernel put it: one plant step per control step against
// 210 model steps and 100 adjoints, its weights wave-uniform reads through the
// constant address space (scalar operands), no LDS for them.
template <bool LEARNT>
__global__ __launch_bounds__(kMpcThreads) void quad_learnt_mpc_closed_loop_kernel(
    MpcLoopArgs A, const float *packed) {
  typedef __attribute__((address_space(4))) const float *cfloat_ptr;
  __shared__ float lds[kLearntMpcLds<kFlightH>];
  const MpcLearnt<const float *> model = learnt_model_in_lds(lds, packed, A.cm);
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
        if (LEARNT) learnt_quad_step_lane(s, u0, A.cp, t, (cfloat_ptr)A.learnt);
        else quad_step(s, u0, A.cp, t);
      },
      model, A.w, A.o, A.rule, log);
}

int fail_arg(const char *e) {
  set_error("%s", e);
  return APG_ERR_ARG;
}

int check_mpc(const ApgQuadParams *model, const ApgQuadLossWeights *weights,
              const ApgQuadMpcOptions *opt, int B) {
  if (B < 0) {
    set_error("B must be >= 0 (got %d)", B);
    return APG_ERR_ARG;
  }
  if (!model || !weights) return fail_arg("model / weights is NULL");
  if (const char *e = mpc_check_options(opt)) return fail_arg(e);
  return APG_OK;
}

void pack_learnt(const ApgLearntResidual &m, float *block, hipStream_t st) {
  hipLaunchKernelGGL(learnt_pack_kernel, dim3((kLearntFloats + 255) / 256), dim3(256), 0, st, m,
                     block);
}

// The solve behind both entry points.  learnt: the solver plans through
// `model_learnt`, packed into workspace[0, kLearntFloats); else neither is read.
int mpc_solve_launch(const char *name, bool learnt, const float *state0, const float *ref,
                     int ref_cols, float dt, const ApgQuadParams *model,
                     const ApgLearntResidual *model_learnt, const ApgQuadLossWeights *weights,
                     const ApgQuadMpcOptions *opt, int B, int H, float *u, float *cost_out,
                     float *cost_trace, float *workspace, apg_stream_t stream) {
  if (int e = check_mpc(model, weights, opt, B)) return e;
  if (const char *e = learnt ? learnt_mpc_check_model(model_learnt) : nullptr) return fail_arg(e);
  if (H != 5 && H != 10) {
    set_error("H must be 5 or 10 (got %d)", H);
    return APG_ERR_ARG;
  }
  if (ref_cols != 9 && ref_cols != 6)
    return fail_arg("ref_cols must be 9 ([pos, euler, vel]) or 6 ([pos, vel])");
  if (B == 0) return APG_OK;
  if (!state0 || !ref || !u || !cost_out || (learnt && !workspace))
    return fail_arg("NULL buffer");
  MpcSolveArgs A;
  A.state0 = state0, A.ref = ref, A.u = u, A.cost_out = cost_out, A.cost_trace = cost_trace;
  A.c = make_const(*model, dt);
  A.w = *weights, A.o = *opt;
  A.B = B, A.ref_cols = ref_cols;
  const dim3 grid((B + kMpcThreads - 1) / kMpcThreads), block(kMpcThreads);
  hipStream_t st = (hipStream_t)stream;
  const float *packed = workspace;
  if (learnt) pack_learnt(*model_learnt, workspace, st);
  with_horizon(H, [&](auto h) {
    if (learnt)
      hipLaunchKernelGGL(quad_learnt_mpc_solve_kernel<h()>, grid, block, 0, st, A, packed);
    else
      hipLaunchKernelGGL(quad_mpc_solve_kernel<h()>, grid, block, 0, st, A);
  });
  return check_launch(name);
}

// The closed loop behind both entry points.  learnt: the solver plans through
// `model_learnt`, packed into workspace[0, kLearntFloats), and the plant's block
// (plant_learnt) follows it; else the plant's block is at workspace[0].
int mpc_loop_launch(const char *name, bool learnt, const ApgQuadFlight *flight, float dt,
                    const ApgQuadParams *plant, const ApgLearntResidual *plant_learnt,
                    const ApgQuadParams *model, const ApgLearntResidual *model_learnt,
                    const ApgQuadLossWeights *weights, const ApgQuadMpcOptions *opt, int B,
                    int H, float *cost, float *workspace, apg_stream_t stream) {
  if (int e = check_mpc(model, weights, opt, B)) return e;
  if (!plant) return fail_arg("plant is NULL");
  if (const char *e = learnt ? learnt_mpc_check_model(model_learnt) : nullptr) return fail_arg(e);
  if (H != kFlightH) {
    set_error("H must be %d (got %d)", kFlightH, H);
    return APG_ERR_ARG;
  }
  MpcLoopArgs A;
  if (const char *e = quad_flight_check(flight, plant_learnt, B, &A.rule)) return fail_arg(e);
  if (B == 0) return APG_OK;
  if ((learnt || plant_learnt) && !workspace) return fail_arg("NULL buffer");
  float *plant_block = learnt ? workspace + kLearntFloats : workspace;
  A.traj = flight->traj, A.steps = flight->steps;
  A.log = {flight->div, flight->drone, flight->actions, flight->start_states, cost, 0, 0};
  A.learnt = plant_learnt ? plant_block : nullptr;
  A.cp = make_const(*plant, dt), A.cm = make_const(*model, dt);
  A.w = *weights, A.o = *opt, A.B = B;
  const dim3 grid((B + kMpcThreads - 1) / kMpcThreads), block(kMpcThreads);
  hipStream_t st = (hipStream_t)stream;
  const float *packed = workspace;
  if (learnt) pack_learnt(*model_learnt, workspace, st);
  if (plant_learnt) pack_learnt(*plant_learnt, plant_block, st);
  with_flag(plant_learnt != nullptr, [&](auto pl) {
    if (learnt)
      hipLaunchKernelGGL(quad_learnt_mpc_closed_loop_kernel<pl()>, grid, block, 0, st, A, packed);
    else
      hipLaunchKernelGGL(quad_mpc_closed_loop_kernel<pl()>, grid, block, 0, st, A);
  });
  return check_launch(name);
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_quad_mpc_solve(const float *state0, const float *ref, int ref_cols, float dt,
                       const ApgQuadParams *model, const ApgQuadLossWeights *weights,
                       const ApgQuadMpcOptions *opt, int B, int H, float *u,
                       float *cost_out, float *cost_trace, apg_stream_t stream) {
  return mpc_solve_launch("quad_mpc_solve", false, state0, ref, ref_cols, dt, model, nullptr,
                          weights, opt, B, H, u, cost_out, cost_trace, nullptr, stream);
}

int apg_quad_mpc_workspace_floats(void) { return kLearntFloats; }

int apg_quad_mpc_closed_loop(const ApgQuadFlight *flight, float dt, const ApgQuadParams *plant,
                             const ApgLearntResidual *plant_learnt, const ApgQuadParams *model,
                             const ApgQuadLossWeights *weights, const ApgQuadMpcOptions *opt,
                             int B, int H, float *cost, float *workspace, apg_stream_t stream) {
  return mpc_loop_launch("quad_mpc_closed_loop", false, flight, dt, plant, plant_learnt, model,
                         nullptr, weights, opt, B, H, cost, workspace, stream);
}

// [0, kLearntFloats): the model's block, [kLearntFloats, 2 kLearntFloats): the plant's
int apg_quad_learnt_mpc_workspace_floats(void) { return 2 * kLearntFloats; }

int apg_quad_learnt_mpc_solve(const float *state0, const float *ref, int ref_cols, float dt,
                              const ApgQuadParams *model, const ApgLearntResidual *model_learnt,
                              const ApgQuadLossWeights *weights, const ApgQuadMpcOptions *opt,
                              int B, int H, float *u, float *cost_out, float *cost_trace,
                              float *workspace, apg_stream_t stream) {
  return mpc_solve_launch("quad_learnt_mpc_solve", true, state0, ref, ref_cols, dt, model,
                          model_learnt, weights, opt, B, H, u, cost_out, cost_trace, workspace,
                          stream);
}

int apg_quad_learnt_mpc_closed_loop(const ApgQuadFlight *flight, float dt,
                                    const ApgQuadParams *plant,
                                    const ApgLearntResidual *plant_learnt,
                                    const ApgQuadParams *model,
                                    const ApgLearntResidual *model_learnt,
                                    const ApgQuadLossWeights *weights,
                                    const ApgQuadMpcOptions *opt, int B, int H, float *cost,
                                    float *workspace, apg_stream_t stream) {
  return mpc_loop_launch("quad_learnt_mpc_closed_loop", true, flight, dt, plant, plant_learnt,
                         model, model_learnt, weights, opt, B, H, cost, workspace, stream);
}

}  // extern "C"

