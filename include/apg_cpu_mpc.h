/*
 * apg_cpu_mpc.h - host twins of the shooting-MPC entry points of apg.h
 * (apg_quad_mpc_solve, apg_quad_mpc_closed_loop), in libapg_cpu.so next to the
 * twins of apg_cpu.h and under the same rules: HOST pointers, synchronous, the
 * per-lane header of the kernels (csrc/quad_mpc_math.h) looped over the batch,
 * signatures of apg.h minus the stream.  apg_quad_mpc_closed_loop_cpu flies the
 * analytic plant only: `plant_learnt` must be NULL, `workspace` is not used (may
 * be NULL).  The cart-pole
 * twins (apg_cartpole_mpc_solve, apg_cartpole_mpc_closed_loop; per-lane header
 * csrc/cartpole_mpc_math.h) fly the learnt plant as well: `plant_learnt` then
 * holds HOST pointers.
 */
#ifndef APG_CPU_MPC_H_
#define APG_CPU_MPC_H_

#include "apg.h"

#ifdef __cplusplus
extern "C" {
#endif

int apg_quad_mpc_solve_cpu(const float *state0, const float *ref, int ref_cols, float dt,
                           const ApgQuadParams *model, const ApgQuadLossWeights *weights,
                           const ApgQuadMpcOptions *opt, int B, int H, float *u,
                           float *cost_out, float *cost_trace);
int apg_quad_mpc_closed_loop_cpu(const ApgQuadFlight *flight, float dt,
                                 const ApgQuadParams *plant,
                                 const ApgLearntResidual *plant_learnt,
                                 const ApgQuadParams *model,
                                 const ApgQuadLossWeights *weights,
                                 const ApgQuadMpcOptions *opt, int B, int H,
                                 float *cost, float *workspace);

/* The learnt-model solver (apg_quad_learnt_mpc_solve,
 * apg_quad_learnt_mpc_closed_loop; per-lane header csrc/quad_learnt_mpc_math.h).
 * These twins fly the learnt plant as well: `plant_learnt` and `model_learnt`
 * hold HOST pointers; `workspace` is not used (may be NULL). */
int apg_quad_learnt_mpc_workspace_floats_cpu(void);
int apg_quad_learnt_mpc_solve_cpu(const float *state0, const float *ref, int ref_cols, float dt,
                                  const ApgQuadParams *model,
                                  const ApgLearntResidual *model_learnt,
                                  const ApgQuadLossWeights *weights,
                                  const ApgQuadMpcOptions *opt, int B, int H, float *u,
                                  float *cost_out, float *cost_trace, float *workspace);
int apg_quad_learnt_mpc_closed_loop_cpu(const ApgQuadFlight *flight, float dt,
                                        const ApgQuadParams *plant,
                                        const ApgLearntResidual *plant_learnt,
                                        const ApgQuadParams *model,
                                        const ApgLearntResidual *model_learnt,
                                        const ApgQuadLossWeights *weights,
                                        const ApgQuadMpcOptions *opt, int B, int H,
                                        float *cost, float *workspace);

int apg_cartpole_mpc_solve_cpu(const float *state0, const float *u0, float dt,
                               const ApgCartpoleParams *model,
                               const ApgCartpoleMpcOptions *opt, int B, int H, float *u,
                               float *cost_out, float *cost_trace);
int apg_cartpole_mpc_closed_loop_cpu(const ApgCartpoleFlight *flight, float dt,
                                     const ApgCartpoleParams *plant,
                                     const ApgCartpoleLearnt *plant_learnt,
                                     const ApgCartpoleParams *model,
                                     const ApgCartpoleMpcOptions *opt, int B, int H,
                                     float *cost);

/* The learnt-model solver (apg_cartpole_learnt_mpc_solve,
 * apg_cartpole_learnt_mpc_closed_loop): `model` and `plant_learnt` hold HOST
 * pointers. */
int apg_cartpole_learnt_mpc_solve_cpu(const float *state0, const float *u0, float dt,
                                      const ApgCartpoleLearnt *model,
                                      const ApgCartpoleMpcOptions *opt, int B, int H, float *u,
                                      float *cost_out, float *cost_trace);
int apg_cartpole_learnt_mpc_closed_loop_cpu(const ApgCartpoleFlight *flight, float dt,
                                            const ApgCartpoleParams *plant,
                                            const ApgCartpoleLearnt *plant_learnt,
                                            const ApgCartpoleLearnt *model,
                                            const ApgCartpoleMpcOptions *opt, int B, int H,
                                            float *cost);

#ifdef __cplusplus
}
#endif
#endif /* APG_CPU_MPC_H_ */
