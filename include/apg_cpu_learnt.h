/*
 * apg_cpu_learnt.h - host twins of the learnt cart-pole entry points of apg.h
 * (LearntCartpoleDynamics, neural_control/dynamics/cartpole_dynamics.py:
 * 122-140), in libapg_cpu.so next to the twins of apg_cpu.h and under the same
 * rules: HOST pointers (the ApgCartpoleLearnt fields included), synchronous,
 * the per-lane header of the kernels (csrc/cartpole_learnt_math.h) looped over
 * the batch, signatures of apg.h minus the stream.  grad_params are summed in
 * sample order; `workspace` is not used (may be NULL).
 */
#ifndef APG_CPU_LEARNT_H_
#define APG_CPU_LEARNT_H_

#include "apg.h"

#ifdef __cplusplus
extern "C" {
#endif

int apg_cartpole_learnt_step_fwd_cpu(const float *state, const float *action, float dt,
                                     const ApgCartpoleLearnt *model, int B,
                                     float *next_state);
int apg_cartpole_learnt_step_bwd_cpu(const float *state, const float *action, float dt,
                                     const ApgCartpoleLearnt *model, int B,
                                     const float *grad_next, float *grad_state,
                                     float *grad_action, float *grad_params,
                                     float *workspace);
int apg_cartpole_learnt_rollout_fwd_bwd_cpu(const float *state0, const float *actions,
                                            float dt, const ApgCartpoleLearnt *model,
                                            int B, int H, int layout,
                                            float *loss_partials, float *loss,
                                            float *grad_actions, float *grad_state0,
                                            float *states_out);

#ifdef __cplusplus
}
#endif
#endif /* APG_CPU_LEARNT_H_ */
