// wing_mpc.hip - batched shooting MPC for the fixed wing (include/apg.h:
// apg_wing_mpc_solve, apg_wing_mpc_closed_loop): the solver of wing_mpc_math.h,
// one trajectory per lane, one wave per workgroup.  Plain per-lane fp32 like
// the rollout kernels of wing.hip - there is no matrix product in it, so no
// MFMA.  Between the iterations of a solve nothing leaves the lane: the
// unknowns (40) and the momentum (40) stay in registers, the pre-step states of
// the forward sweep, which the reverse sweep recomputes its steps from, go to
// LDS as [H][12][64 lanes] (H = 10: 30 KB per workgroup; lane-strided
// addresses, no bank conflicts) - the layout of quad_mpc.hip's kLearntMpcLds.
// kernel_resources.json must show no scratch and no spill for both kernels
// (tests/test_wing_mpc_cpu.py).
#include "wing_mpc_math.h"

namespace apg {
namespace {

constexpr int kWingMpcThreads = 64;
constexpr int kWingMpcH = 10;   // the one horizon (wing_mpc_check)

template <int H>
constexpr int kWingMpcLds = H * 12 * kWingMpcThreads;
static_assert(4 * kWingMpcLds<kWingMpcH> * sizeof(float) <= 160 * 1024,
              "four workgroups per CU");

struct WingMpcSolveArgs {
  const float *state0, *ref;           // [12][B], [H][3][B]
  float *u, *cost_out, *cost_trace;    // [H][4][B], [B], [iters + 1][B] or NULL
  WingConst c;
  ApgWingLossWeights w;
  ApgWingMpcOptions o;
  int B;
};

template <int H>
__global__ __launch_bounds__(kWingMpcThreads) void wing_mpc_solve_kernel(WingMpcSolveArgs A) {
  __shared__ float lds[kWingMpcLds<H>];
  const int lane = threadIdx.x;
  const int b = blockIdx.x * kWingMpcThreads + lane;
  if (b >= A.B) return;
  const size_t B = (size_t)A.B;
  float s0[12], u[H][4];
#pragma unroll
  for (int i = 0; i < 12; ++i) s0[i] = A.state0[i * B + b];
#pragma unroll
  for (int k = 0; k < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) u[k][j] = A.u[((size_t)k * 4 + j) * B + b];
  const float *ref = A.ref + b;
  float *trace = A.cost_trace;
  const float J = wing_mpc_solve<H>(
      s0,
      [&](int k, float (&rp)[3]) {
#pragma unroll
        for (int i = 0; i < 3; ++i) rp[i] = ref[((size_t)k * 3 + i) * B];
      },
      u, A.c, A.w, A.o,
      [&](int k, int i) -> float & { return lds[(k * 12 + i) * kWingMpcThreads + lane]; },
      [&](int i, float Ji) {
        if (trace) trace[(size_t)i * B + b] = Ji;
      });
  A.cost_out[b] = J;
#pragma unroll
  for (int k = 0; k < H; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) A.u[((size_t)k * 4 + j) * B + b] = u[k][j];
}

struct WingMpcLoopArgs {
  const float *targets, *state0;   // [n][3][B], [12][B] or NULL
  int *steps;                      // [B]
  WingMpcFlightLog log;            // B, b: set per lane
  WingConst cp, cm;                // plant, model
  ApgWingLossWeights w;
  ApgWingMpcOptions o;
  WingFlightRule rule;
  int B;
};

// wing_mpc_flight (wing_mpc_math.h), one flight per lane.  A lane past the
// batch, or a flight that has ended, keeps stepping with its wave (no writes);
// the wave leaves when none of its flights is alive.
template <int H>
__global__ __launch_bounds__(kWingMpcThreads) void wing_mpc_closed_loop_kernel(
    WingMpcLoopArgs A) {
  __shared__ float lds[kWingMpcLds<H>];
  const int lane = threadIdx.x;
  const int b = blockIdx.x * kWingMpcThreads + lane;
  const bool live = b < A.B;
  const size_t B = (size_t)A.B;
  const size_t bb = live ? (size_t)b : B - 1;   // (a dead lane reads the last flight's inputs)
  WingMpcFlightLog log = A.log;
  log.B = B, log.b = bb;
  const float *tg = A.targets + bb;
  const int steps = wing_mpc_flight<H>(
      A.state0 != nullptr, [&](int i) { return A.state0[i * B + bb]; },
      [&](int ti, float (&t)[3]) {
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = tg[((size_t)ti * 3 + j) * B];
      },
      [&](float (&s)[12], const float (&a)[4]) { wing_step<true>(s, a, A.cp); }, A.cm, A.w,
      A.o, A.rule, log,
      [&](int k, int i) -> float & { return lds[(k * 12 + i) * kWingMpcThreads + lane]; },
      [](bool alive) { return __any(alive) != 0; }, live);
  if (live) A.steps[b] = steps;
}

int fail_arg(const char *e) {
  set_error("%s", e);
  return APG_ERR_ARG;
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_wing_mpc_solve(const float *state0, const float *ref, float dt,
                       const ApgWingParams *model, const ApgWingLossWeights *weights,
                       const ApgWingMpcOptions *opt, int B, int H, float *u, float *cost_out,
                       float *cost_trace, apg_stream_t stream) {
  if (const char *e = wing_mpc_check(model, weights, opt, B, H)) return fail_arg(e);
  if (B == 0) return APG_OK;
  if (!state0 || !ref || !u || !cost_out) return fail_arg("NULL buffer");
  WingMpcSolveArgs A;
  A.state0 = state0, A.ref = ref, A.u = u, A.cost_out = cost_out, A.cost_trace = cost_trace;
  A.c = make_const(*model, dt);
  A.w = *weights, A.o = *opt, A.B = B;
  const dim3 grid((B + kWingMpcThreads - 1) / kWingMpcThreads), block(kWingMpcThreads);
  hipLaunchKernelGGL(wing_mpc_solve_kernel<kWingMpcH>, grid, block, 0, (hipStream_t)stream, A);
  return check_launch("wing_mpc_solve");
}

int apg_wing_mpc_closed_loop(const ApgWingFlight *flight, float dt,
                             const ApgWingParams *plant, const ApgWingParams *model,
                             const ApgWingLossWeights *weights,
                             const ApgWingMpcOptions *opt, int B, int H,
                             float *cost, apg_stream_t stream) {
  WingMpcLoopArgs A;
  if (const char *e = wing_mpc_check(model, weights, opt, B, H)) return fail_arg(e);
  if (const char *e = wing_mpc_check_flight(plant, flight, B, &A.rule)) return fail_arg(e);
  if (B == 0) return APG_OK;
  A.targets = flight->targets, A.state0 = flight->state0, A.steps = flight->steps;
  A.log = {flight->div_linear, flight->div_pass, flight->div_fail, flight->drone,
           flight->seen, cost, 0, 0};
  A.cp = make_const(*plant, dt), A.cm = make_const(*model, dt);
  A.w = *weights, A.o = *opt, A.B = B;
  const dim3 grid((B + kWingMpcThreads - 1) / kWingMpcThreads), block(kWingMpcThreads);
  hipLaunchKernelGGL(wing_mpc_closed_loop_kernel<kWingMpcH>, grid, block, 0,
                     (hipStream_t)stream, A);
  return check_launch("wing_mpc_closed_loop");
}

}  // extern "C"
