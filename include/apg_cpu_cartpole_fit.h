/*
 * apg_cpu_cartpole_fit.h - host twin of the fused simulator-fit step of the
 * learnt cart-pole (apg_cartpole_learnt_fit_fwd_bwd of apg.h; TrainBase.
 * train_dynamics_model, scripts/train_base.py:160-186, on
 * LearntCartpoleDynamics), in libapg_cpu.so next to the twins of apg_cpu.h and
 * under the same rules: HOST pointers (the ApgCartpoleLearnt fields included),
 * synchronous, the per-lane header of the kernel (csrc/cartpole_fit_math.h)
 * looped over the batch and summed in sample order, the signature of apg.h
 * minus the stream.  `workspace` is not used (may be NULL).
 */
#ifndef APG_CPU_CARTPOLE_FIT_H_
#define APG_CPU_CARTPOLE_FIT_H_

#include "apg.h"

#ifdef __cplusplus
extern "C" {
#endif

int apg_cartpole_learnt_fit_fwd_bwd_cpu(const float *state, const float *action, float dt,
    const ApgCartpoleLearnt *model, const float *target,
    const ApgCartpoleParams *eval_params, int B, float *loss_partials,
    float *loss, float *grad, float *workspace);

#ifdef __cplusplus
}
#endif
#endif /* APG_CPU_CARTPOLE_FIT_H_ */
