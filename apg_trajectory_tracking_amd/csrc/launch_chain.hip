// launch_chain.hip - the two-lane deferred-loss launch chain (launch_chain.h
// decides, this file enqueues): the chained forms of the fused rollout entry
// points, apg_launch_chain_prepare and apg_launch_chain_flush.
//
// One Chain per caller stream: the lane-1 stream and four events (timing
// disabled), made once by apg_launch_chain_prepare outside any stream capture
// and kept for the life of the process.  Fork, cross-lane edges and join are
// hipEventRecord + hipStreamWaitEvent only, so the same calls serve eager
// launches and a capture of the caller's stream (lane 1 joins the capture
// through the fork event and leaves it at the flush).
#include <mutex>
#include <vector>

#include "apg_device.h"
#include "launch_chain.h"

namespace apg {

// quad.hip: apg_quad_rollout_fwd_bwd with the choice of the rows kernel's
// chained instantiation
int quad_rollout_fwd_bwd_launch(const float *state0, const float *actions,
                                const float *ref, int ref_cols, float dt,
                                const ApgQuadParams *params,
                                const ApgQuadLossWeights *weights, int B, int H,
                                int layout, float *loss_partials, float *loss,
                                float *grad_actions, float *grad_state0,
                                float *states_out, const ApgDeferredLoss *deferred,
                                hipStream_t st, bool chained);

namespace {

struct Chain {
  hipStream_t caller = nullptr;
  int device = -1;
  hipStream_t lane1 = nullptr;
  hipEvent_t fork = nullptr, join = nullptr, edge[2] = {nullptr, nullptr};
  bool lane1_forked = false;  // lane 1 has waited for this chain's fork event
  LaunchChain book;
  hipStream_t lane(int l) const { return l == 0 ? caller : lane1; }
};

std::mutex g_mutex;
std::vector<Chain *> g_chains;
int g_lane_priority_mode = 0;

Chain *chain_of(hipStream_t stream) {
  const int dev = device_slot();
  for (Chain *c : g_chains)
    if (c->caller == stream && c->device == dev) return c;
  return nullptr;
}

int hip_fail(hipError_t e, const char *what) {
  (void)hipGetLastError();
  set_error("%s: HIP error %d (%s)", what, (int)e, hipGetErrorString(e));
  return APG_ERR_HIP;
}

#define CHAIN_HIP(call, what)                                  \
  do {                                                         \
    hipError_t e_ = (call);                                    \
    if (e_ != hipSuccess) return hip_fail(e_, what);           \
  } while (0)

// Lane 1 must sit on another hardware queue than the caller's stream, or the
// two lanes run one after the other.  The runtime keeps its queue pools per
// stream priority: a lane of a DIFFERENT priority never shares the caller's
// queue (mode 0).  Modes 1 / 2 are for measuring that claim.
int lane_priority(hipStream_t caller, int *out) {
  int least = 0, greatest = 0, mine = 0;
  CHAIN_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest), "priority range");
  if (caller) CHAIN_HIP(hipStreamGetPriority(caller, &mine), "hipStreamGetPriority");
  if (g_lane_priority_mode == 1)
    *out = mine;
  else if (g_lane_priority_mode == 2)
    *out = mine != least ? least : 0;
  else
    *out = mine != greatest ? greatest : 0;
  return APG_OK;
}

int prepare(hipStream_t stream) {
  if (chain_of(stream)) return APG_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (stream && hipStreamIsCapturing(stream, &cs) == hipSuccess &&
      cs != hipStreamCaptureStatusNone) {
    set_error("apg_launch_chain_prepare: the stream is capturing (prepare before)");
    return APG_ERR_ARG;
  }
  (void)hipGetLastError();
  Chain *c = new Chain;
  c->caller = stream;
  c->device = device_slot();
  int prio = 0;
  if (int e = lane_priority(stream, &prio)) {
    delete c;
    return e;
  }
  hipError_t e = hipStreamCreateWithPriority(&c->lane1, hipStreamNonBlocking, prio);
  hipEvent_t *ev[4] = {&c->fork, &c->join, &c->edge[0], &c->edge[1]};
  for (int i = 0; i < 4 && e == hipSuccess; ++i)
    e = hipEventCreateWithFlags(ev[i], hipEventDisableTiming);
  if (e != hipSuccess) {
    for (hipEvent_t *p : ev)
      if (*p) (void)hipEventDestroy(*p);
    if (c->lane1) (void)hipStreamDestroy(c->lane1);
    delete c;
    return hip_fail(e, "apg_launch_chain_prepare");
  }
  g_chains.push_back(c);
  return APG_OK;
}

int enqueue_reduce(const ChainReduce &r, hipStream_t st) {
  return launch_reduce_partials(r.partials, r.count, r.loss, st);
}

// Fork / reductions / edge of one step; *st = the stream the kernel goes to.
int enqueue_step(Chain &c, const ChainStep &s, hipStream_t *st) {
  if (s.fork) {
    CHAIN_HIP(hipEventRecord(c.fork, c.caller), "fork record");
    c.lane1_forked = false;
  }
  auto use = [&](int l) -> int {
    if (l == 1 && !c.lane1_forked) {
      CHAIN_HIP(hipStreamWaitEvent(c.lane1, c.fork, 0), "fork wait");
      c.lane1_forked = true;
    }
    return APG_OK;
  };
  if (int e = use(s.lane)) return e;
  if (s.pre.loss)
    if (int e = enqueue_reduce(s.pre, c.lane(s.pre_lane))) return e;
  if (s.edge_from >= 0) {
    CHAIN_HIP(hipEventRecord(c.edge[s.edge_from], c.lane(s.edge_from)), "edge record");
    CHAIN_HIP(hipStreamWaitEvent(c.lane(s.lane), c.edge[s.edge_from], 0), "edge wait");
  }
  *st = c.lane(s.lane);
  return APG_OK;
}

int flush(hipStream_t stream) {
  std::lock_guard<std::mutex> lock(g_mutex);
  Chain *c = chain_of(stream);
  if (!c || c->book.empty()) return APG_OK;
  const ChainFlush f = c->book.flush();
  int err = APG_OK;
  for (int m = 0; m < 2; ++m)
    for (const ChainReduce &r : f.reduce[m])
      if (int e = enqueue_reduce(r, c->lane(m))) err = err ? err : e;
  // the join is enqueued whatever failed above: a capture must not be left
  // with lane 1 unjoined
  if (f.join) {
    hipError_t e = hipEventRecord(c->join, c->lane1);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->caller, c->join, 0);
    if (e != hipSuccess && !err) err = hip_fail(e, "apg_launch_chain_flush: join");
  }
  c->lane1_forked = false;
  return err;
}

// `enqueue(deferred, stream)`: the existing (serial) entry point with this
// launch's arguments, `loss` = NULL.
template <class Enqueue>
int chained(hipStream_t stream, const float *loss_partials, int B, float *loss,
            const ApgDeferredLoss *deferred, Enqueue enqueue) {
  if (!loss) {
    set_error("chained launch: loss is NULL (it receives the deferred sum)");
    return APG_ERR_ARG;
  }
  ChainLaunch L{loss_partials, B > 0 ? apg_loss_partials_count(B) : 0, loss, {}};
  if (deferred && deferred->prev_partials) {
    if (!deferred->prev_loss || deferred->prev_count < 0 ||
        deferred->prev_partials == loss_partials || deferred->prev_loss == loss) {
      set_error("deferred: prev_loss NULL, prev_count < 0 or the launch is "
                "chained after its own plan");
      return APG_ERR_ARG;
    }
    L.after = ChainReduce{deferred->prev_partials, deferred->prev_count,
                          deferred->prev_loss};
  }
  std::lock_guard<std::mutex> lock(g_mutex);
  Chain *c = chain_of(stream);
  if (!c) {
    set_error("chained launch: apg_launch_chain_prepare was not called for this stream");
    return APG_ERR_ARG;
  }
  const LaunchChain saved = c->book;
  const ChainStep s = c->book.launch(L);
  hipStream_t st = nullptr;
  int e = enqueue_step(*c, s, &st);
  if (!e) {
    const ApgDeferredLoss fold{s.fold.partials, s.fold.count, s.fold.loss};
    e = enqueue(s.fold.loss ? &fold : nullptr, st);
  }
  if (e) c->book = saved;  // the launch did not happen
  return e;
}

}  // namespace
}  // namespace apg

using namespace apg;

extern "C" {

int apg_launch_chain_prepare(apg_stream_t stream) {
  std::lock_guard<std::mutex> lock(g_mutex);
  return prepare((hipStream_t)stream);
}

int apg_launch_chain_flush(apg_stream_t stream) { return flush((hipStream_t)stream); }

int apg_launch_chain_set_lane_priority(int mode) {
  if (mode < 0 || mode > 2) {
    set_error("apg_launch_chain_set_lane_priority: mode must be 0, 1 or 2");
    return APG_ERR_ARG;
  }
  std::lock_guard<std::mutex> lock(g_mutex);
  g_lane_priority_mode = mode;
  return APG_OK;
}

int apg_quad_rollout_fwd_bwd_chained(const float *state0, const float *actions,
                                     const float *ref, int ref_cols, float dt,
                                     const ApgQuadParams *params,
                                     const ApgQuadLossWeights *weights, int B, int H,
                                     int layout, float *loss_partials, float *loss,
                                     float *grad_actions, float *grad_state0,
                                     float *states_out,
                                     const ApgDeferredLoss *deferred,
                                     apg_stream_t stream) {
  return chained((hipStream_t)stream, loss_partials, B, loss, deferred,
                 [&](const ApgDeferredLoss *d, hipStream_t st) {
                   return quad_rollout_fwd_bwd_launch(
                       state0, actions, ref, ref_cols, dt, params, weights, B, H,
                       layout, loss_partials, nullptr, grad_actions, grad_state0,
                       states_out, d, st, true);
                 });
}

int apg_wing_rollout_fwd_bwd_chained(const float *state0, const float *actions,
                                     const float *ref, float dt,
                                     const ApgWingParams *params,
                                     const ApgWingLossWeights *weights, int B, int H,
                                     int layout, float *loss_partials, float *loss,
                                     float *grad_actions, float *grad_state0,
                                     float *states_out,
                                     const ApgDeferredLoss *deferred,
                                     apg_stream_t stream) {
  return chained((hipStream_t)stream, loss_partials, B, loss, deferred,
                 [&](const ApgDeferredLoss *d, hipStream_t st) {
                   return apg_wing_rollout_fwd_bwd(
                       state0, actions, ref, dt, params, weights, B, H, layout,
                       loss_partials, nullptr, grad_actions, grad_state0,
                       states_out, d, st);
                 });
}

}  // extern "C"
