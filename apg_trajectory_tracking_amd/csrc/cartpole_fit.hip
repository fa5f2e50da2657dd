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
// Two launches behind one entry point, the shared fit of residual_fit.h on
// CartFit (cartpole_fit_math.h): no pack launch - the 640 residual floats are
// staged into LDS as unit rows by every workgroup - and no regulariser.
#include <stddef.h>

#include "apg_device.h"
#include "cartpole_fit_math.h"

namespace apg {
namespace {

static_assert(kCartGW1 == APG_CARTPOLE_LEARNT_G_W1 && kCartGB1 == APG_CARTPOLE_LEARNT_G_B1 &&
                  kCartGW2 == APG_CARTPOLE_LEARNT_G_W2 &&
                  kCartLearntGrads == APG_CARTPOLE_LEARNT_GRADS,
              "apg.h publishes these offsets");

template <bool EVAL>
__global__ __launch_bounds__(kFitBlock) void cartpole_fit_kernel(CartFitArgs A) {
  fit_body<CartFit, EVAL>(A);
}

__global__ __launch_bounds__(kFitCols * kFitSplit) void cartpole_fit_reduce_kernel(
    const float *__restrict__ rows, int nrows, float *__restrict__ grad) {
  fit_reduce<CartFit>(rows, nrows, FitNoScale{}, ResidualTensors{}, nullptr, 0.f, grad, nullptr);
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_cartpole_learnt_fit_workspace_floats(int B) { return fit_workspace_floats<CartFit>(B); }

int apg_cartpole_learnt_fit_fwd_bwd(const float *state, const float *action, float dt,
                                    const ApgCartpoleLearnt *model, const float *target,
                                    const ApgCartpoleParams *eval_params, int B,
                                    float *loss_partials, float *loss, float *grad,
                                    float *workspace, apg_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const FitCall call{state, action, target, eval_params != nullptr, 0.f, B, loss_partials,
                     loss, grad, workspace, st, cart_learnt_check(model, true)};
  return fit_run<CartFit>(
      call, "cartpole_learnt_fit_fwd_bwd", "cartpole_learnt_fit_reduce",
      cartpole_fit_kernel<true>, cartpole_fit_kernel<false>,
      [&](CartFitArgs &A) {
        A.m = *model, A.dt = dt;
        A.eval = eval_params ? make_const(*eval_params, dt) : CartConst{};
      },
      [&](int blocks) {
        hipLaunchKernelGGL(cartpole_fit_reduce_kernel, dim3(CartFit::ROW / kFitCols),
                           dim3(kFitCols * kFitSplit), 0, st, workspace, blocks, grad);
      });
}

}  // extern "C"
