/*
 * apg_cpu_launch_chain.h - the decisions of the two-lane launch chain
 * (csrc/launch_chain.h, include/apg.h "launch chain") behind a C interface of
 * libapg_cpu.so, for the host tests: the same bookkeeping object that
 * libapg_hip.so turns into stream and event calls, with no GPU involved.
 * Buffers are named by their addresses only and never dereferenced.
 */
#ifndef APG_CPU_LAUNCH_CHAIN_H_
#define APG_CPU_LAUNCH_CHAIN_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ApgCpuChainReduce {
  const float *partials;
  int count;
  float *loss; /* NULL: no reduction */
} ApgCpuChainReduce;

/* What one chained launch enqueues, in this order: the fork event on the
 * caller's stream (`fork`), the stand-alone reduction `pre` on lane
 * `pre_lane`, the event edge from the tail of lane `edge_from` (-1: none),
 * the kernel on `lane` with the reduction `fold` inside. */
typedef struct ApgCpuChainStep {
  int lane, fork, pre_lane, edge_from;
  ApgCpuChainReduce pre, fold;
} ApgCpuChainStep;

void *apg_cpu_chain_new(void);
void apg_cpu_chain_free(void *chain);
int apg_cpu_chain_empty(const void *chain);
/* after_loss NULL: launched without `after`. */
void apg_cpu_chain_launch(void *chain, const float *partials, int count, float *loss,
                          const float *after_partials, int after_count,
                          float *after_loss, ApgCpuChainStep *step);
/* The reductions the flush enqueues on lane 0 / lane 1 (at most `cap` each are
 * written, n0 / n1 receive the numbers owed) and whether lane 1 is joined. */
void apg_cpu_chain_flush(void *chain, ApgCpuChainReduce *lane0, int *n0,
                         ApgCpuChainReduce *lane1, int *n1, int cap, int *join);

#ifdef __cplusplus
}
#endif
#endif /* APG_CPU_LAUNCH_CHAIN_H_ */
