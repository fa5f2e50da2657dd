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
// Three launches behind one entry point, the shared fit of residual_fit.h on
// QuadFit (quad_fit_math.h): pack (the residual's unit rows, linear_at and the
// four weight norms from the live tensors), the fit kernel (the row's head:
// linear_at, kinv, sum lam_w', db2) and the reduction, which scales the inertia
// elements into dL/dJ and writes the mass slot as 0.
#include <stddef.h>

#include "apg_device.h"
#include "quad_fit_math.h"

namespace apg {
namespace {

static_assert(kQuadFitGLin == APG_QUAD_FIT_G_LINEAR_AT && kQuadFitGMass == APG_QUAD_FIT_G_MASS &&
                  kQuadFitGInertia == APG_QUAD_FIT_G_INERTIA &&
                  kQuadFitGKinv == APG_QUAD_FIT_G_KINV && kQuadFitGW1 == APG_QUAD_FIT_G_W1 &&
                  kQuadFitGB1 == APG_QUAD_FIT_G_B1 && kQuadFitGW2 == APG_QUAD_FIT_G_W2 &&
                  kQuadFitGB2 == APG_QUAD_FIT_G_B2 && kQuadFitGrads == APG_QUAD_FIT_GRADS,
              "apg.h publishes these offsets");

// the packed model of quad_fit_math.h plus |W2|, |b2|, |W1|, |b1|
__global__ __launch_bounds__(256) void quad_learnt_fit_pack_kernel(ApgLearntResidual m,
                                                                   float *__restrict__ ws) {
  __shared__ float part[4][256];
  for (int t = threadIdx.x; t < kQuadPackFloats; t += blockDim.x) ws[t] = quad_fit_packed(t, m);
  residual_norms(m.w1, m.b1, m.w2, m.b2, part, ws + QuadFit::NORMS_AT);
}

template <bool EVAL>
__global__ __launch_bounds__(kFitBlock) void quad_learnt_fit_kernel(QuadFitArgs A) {
  fit_body<QuadFit, EVAL>(A);
}

__global__ __launch_bounds__(kFitCols * kFitSplit) void quad_learnt_fit_reduce_kernel(
    const float *__restrict__ ws, int nrows, ApgLearntResidual m, QuadFitInertia q,
    float l2_lambda, float *__restrict__ grad, float *__restrict__ loss) {
  fit_reduce<QuadFit>(ws + QuadFit::ROWS_AT, nrows, q, ResidualTensors{m.w1, m.b1, m.w2, m.b2},
                      ws + QuadFit::NORMS_AT, l2_lambda, grad, loss);
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_quad_learnt_fit_grad_count(void) { return kQuadFitGrads; }

int apg_quad_learnt_fit_workspace_floats(int B) { return fit_workspace_floats<QuadFit>(B); }

int apg_quad_learnt_fit_fwd_bwd(const float *state, const float *action, float dt,
                                const ApgQuadParams *params, const ApgLearntResidual *model,
                                const float *target, const ApgQuadParams *eval_params,
                                float l2_lambda, int B, float *loss_partials, float *loss,
                                float *grad, float *workspace, apg_stream_t stream) {
  const char *bad = nullptr;
  if (!params) bad = "params is NULL";
  else if (!model || !model->linear_at || !model->w1 || !model->b1 || !model->w2 || !model->b2)
    bad = "model or one of its pointers is NULL";
  hipStream_t st = (hipStream_t)stream;
  const FitCall call{state, action, target, eval_params != nullptr, l2_lambda, B,
                     loss_partials, loss, grad, workspace, st, bad};
  return fit_run<QuadFit>(
      call, "quad_learnt_fit_fwd_bwd", "quad_learnt_fit_reduce", quad_learnt_fit_kernel<true>,
      quad_learnt_fit_kernel<false>,
      [&](QuadFitArgs &A) {
        hipLaunchKernelGGL(quad_learnt_fit_pack_kernel, dim3(1), dim3(256), 0, st, *model,
                           workspace);
        A.ws = workspace;
        A.c = make_const(*params, dt);
        A.eval = eval_params ? make_const(*eval_params, dt) : QuadConst{};
      },
      [&](int blocks) {
        hipLaunchKernelGGL(quad_learnt_fit_reduce_kernel, dim3(QuadFit::ROW / kFitCols),
                           dim3(kFitCols * kFitSplit), 0, st, workspace, blocks, *model,
                           make_fit_inertia(*params, dt), l2_lambda, grad, loss);
      });
}

}  // extern "C"
