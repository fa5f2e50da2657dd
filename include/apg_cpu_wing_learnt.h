/*
 * apg_cpu_wing_learnt.h - host twin of the fused rollout through the learnt
 * fixed-wing simulator (apg_wing_learnt_rollout_fwd_bwd of apg.h;
 * LearntFixedWingDynamics, neural_control/dynamics/fixed_wing_dynamics.py:
 * 270-326), in libapg_cpu.so next to the twins of apg_cpu.h and under the same
 * rules: HOST pointers (the ApgWingLearnt fields included), synchronous, the
 * per-lane header of the kernel (csrc/wing_learnt_math.h) looped over the
 * batch, the signature of apg.h minus the stream.  `workspace` is not used
 * (may be NULL).
 */
#ifndef APG_CPU_WING_LEARNT_H_
#define APG_CPU_WING_LEARNT_H_

#include "apg.h"

#ifdef __cplusplus
extern "C" {
#endif

int apg_wing_learnt_rollout_fwd_bwd_cpu(const float *state0, const float *actions, const float *ref,
    float dt, const ApgWingLearnt *model, const ApgWingLossWeights *weights, int B, int H,
    int layout, float *loss_partials, float *loss, float *grad_actions, float *grad_state0,
    float *states_out, float *workspace);

#ifdef __cplusplus
}
#endif
#endif /* APG_CPU_WING_LEARNT_H_ */
