/*
 * apg_cpu_quad_fit.h - host twin of the fused simulator-fit step of the learnt
 * quadrotor (apg_quad_learnt_fit_fwd_bwd of apg.h; TrainBase.
 * train_dynamics_model, scripts/train_base.py:160-186, on LearntDynamics), in
 * libapg_cpu.so next to the twins of apg_cpu.h and under the same rules: HOST
 * pointers (the ApgLearntResidual fields included), synchronous, the per-lane
 * header of the kernel (csrc/quad_fit_math.h) looped over the batch, the
 * signature of apg.h minus the stream.  `workspace` is not used (may be NULL).
 */
#ifndef APG_CPU_QUAD_FIT_H_
#define APG_CPU_QUAD_FIT_H_

#include "apg.h"

#ifdef __cplusplus
extern "C" {
#endif

int apg_quad_learnt_fit_fwd_bwd_cpu(const float *state, const float *action, float dt,
    const ApgQuadParams *params, const ApgLearntResidual *model, const float *target,
    const ApgQuadParams *eval_params, float l2_lambda, int B, float *loss_partials,
    float *loss, float *grad, float *workspace);

#ifdef __cplusplus
}
#endif
#endif /* APG_CPU_QUAD_FIT_H_ */
