/*
 * apg_cpu_cartpole_learnt_train.h - host twin of the fused controller step of
 * the cart-pole through LearntCartpoleDynamics
 * (apg_cartpole_learnt_mlp_train_step of apg.h), in libapg_cpu.so next to the
 * twin of apg_cpu_cartpole_train.h and under the same rules: HOST pointers (the
 * fields of ApgCartpoleLearnt, ApgCartpolePolicy, ApgCartpolePolicyGrads and
 * ApgCartpoleSgdUpdate included), synchronous, the per-sample headers of the
 * kernel (csrc/cartpole_train_math.h, csrc/cartpole_learnt_math.h) looped over
 * the batch and summed in sample order, the signature of apg.h minus the
 * stream.  `workspace` is not used (may be NULL).
 */
#ifndef APG_CPU_CARTPOLE_LEARNT_TRAIN_H_
#define APG_CPU_CARTPOLE_LEARNT_TRAIN_H_

#include "apg.h"

#ifdef __cplusplus
extern "C" {
#endif

int apg_cartpole_learnt_mlp_train_step_cpu(const float *in_state, const float *state0,
                                           float dt, const ApgCartpoleLearnt *model,
                                           const ApgCartpolePolicy *policy, int B, int H,
                                           float *loss_partials, float *loss,
                                           const ApgCartpolePolicyGrads *grads,
                                           float *actions_out, float *workspace,
                                           const ApgCartpoleSgdUpdate *update);

#ifdef __cplusplus
}
#endif
#endif /* APG_CPU_CARTPOLE_LEARNT_TRAIN_H_ */
