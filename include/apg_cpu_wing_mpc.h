/*
 * apg_cpu_wing_mpc.h - host twins of the fixed-wing shooting-MPC entry points of
 * apg.h (apg_wing_mpc_solve, apg_wing_mpc_closed_loop), in libapg_cpu.so next to
 * the twins of apg_cpu.h and under the same rules: HOST pointers, synchronous,
 * the per-lane headers of the kernels (csrc/wing_mpc_math.h,
 * csrc/wing_flight_rule.h) looped over the batch, signatures of apg.h minus the
 * stream.  A flight ends by its own flag (on the device: by its wave's vote;
 * the outputs are the same, an ended flight writes nothing).
 */
#ifndef APG_CPU_WING_MPC_H_
#define APG_CPU_WING_MPC_H_

#include "apg.h"

#ifdef __cplusplus
extern "C" {
#endif

int apg_wing_mpc_solve_cpu(const float *state0, const float *ref, float dt,
                           const ApgWingParams *model, const ApgWingLossWeights *weights,
                           const ApgWingMpcOptions *opt, int B, int H, float *u,
                           float *cost_out, float *cost_trace);
int apg_wing_mpc_closed_loop_cpu(const ApgWingFlight *flight, float dt,
                                 const ApgWingParams *plant, const ApgWingParams *model,
                                 const ApgWingLossWeights *weights,
                                 const ApgWingMpcOptions *opt, int B, int H, float *cost);

#ifdef __cplusplus
}
#endif
#endif /* APG_CPU_WING_MPC_H_ */
