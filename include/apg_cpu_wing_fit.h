/*
 * apg_cpu_wing_fit.h - host twin of the fused simulator-fit step of the learnt
 * fixed wing (apg_wing_learnt_fit_fwd_bwd of apg.h; TrainBase.
 * train_dynamics_model, scripts/train_base.py:160-186, on
 * LearntFixedWingDynamics), in libapg_cpu.so next to the twins of apg_cpu.h and
 * under the same rules: HOST pointers (the ApgWingLearnt fields included),
 * synchronous, the per-lane header of the kernel (csrc/wing_learnt_math.h)
 * looped over the batch, the signature of apg.h minus the stream.  `workspace`
 * is not used (may be NULL).
 */
#ifndef APG_CPU_WING_FIT_H_
#define APG_CPU_WING_FIT_H_

#include "apg.h"

#ifdef __cplusplus
extern "C" {
#endif

int apg_wing_learnt_fit_fwd_bwd_cpu(const float *state, const float *action, float dt,
    const ApgWingLearnt *model, const float *target, const ApgWingParams *eval_params,
    float l2_lambda, int B, float *loss_partials, float *loss, float *grad,
    float *workspace);

#ifdef __cplusplus
}
#endif
#endif /* APG_CPU_WING_FIT_H_ */
