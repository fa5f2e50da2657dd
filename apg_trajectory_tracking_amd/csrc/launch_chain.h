// launch_chain.h - bookkeeping of a deferred-loss rollout chain that runs as
// two overlapping launch lanes (include/apg.h, "launch chain").
//
// Plain C++, no HIP call: launch_chain.hip turns a ChainStep into stream and
// event calls, cpu_twins.hip exposes the same decisions to the host tests
// (tests/test_launch_chain_cpu.py).
//
// A fused-rollout kernel folds exactly ONE earlier launch's loss reduction
// into itself (ApgDeferredLoss).  Launched `after` its predecessor on ONE
// stream, kernel i+1 reads kernel i's partials in its first instructions: a
// true dependency, the chain is serial.  Here the launches alternate between
// two lanes (lane 0 = the caller's stream, lane 1 = a stream the library owns)
// and a kernel reduces the oldest due launch of ITS OWN lane - kernel i+2
// reduces kernel i - so stream order alone guarantees the producer has
// finished, the two lanes share no edge, and the tail and the kernel boundary
// of one launch overlap the head of the next.
//
// A plan (one set of output buffers) is identified by its `loss` pointer.
#pragma once
#include <cstddef>
#include <vector>

namespace apg {

struct ChainReduce {
  const float *partials = nullptr;  // [count] of an earlier launch
  int count = 0;
  float *loss = nullptr;            // [1]; nullptr: no reduction
};

struct ChainLaunch {
  const float *partials;  // this launch's loss partials
  int count;
  float *loss;            // where this launch's loss goes once it is reduced
  ChainReduce after;      // the plan given as `after` (loss == nullptr: none)
};

// What to enqueue for one launch, in this order.
struct ChainStep {
  int lane = 0;
  bool fork = false;      // first launch of a chain: record the fork event on
                          // the caller's stream BEFORE anything else
  ChainReduce pre;        // stand-alone reduction to enqueue first ...
  int pre_lane = -1;      // ... on this lane: the launch is about to overwrite
                          // partials that nothing has reduced yet
  int edge_from = -1;     // lane whose tail `lane` must wait for (event edge),
                          // or -1: the launch's buffers were last written there
  ChainReduce fold;       // the reduction the kernel itself carries
};

// What flush() enqueues: per lane the reductions that are still owed, then -
// if lane 1 was used - its join into the caller's stream.
struct ChainFlush {
  std::vector<ChainReduce> reduce[2];
  bool join = false;
};

class LaunchChain {
 public:
  bool empty() const { return launches_ == 0; }
  bool lane1_used() const { return lane1_used_; }

  ChainStep launch(const ChainLaunch &L) {
    ChainStep s;
    s.fork = launches_ == 0;
    const int after_lane = L.after.loss ? writer_of(L.after.loss) : -1;
    if (after_lane >= 0)
      s.lane = 1 - after_lane;           // the lane `after` is not on
    else
      s.lane = launches_ == 0 ? 0 : 1 - last_lane_;
    // `after`'s reduction becomes due on its producer's lane (a plan this
    // chain has not launched was produced before the fork: any lane will do)
    if (L.after.loss) {
      Owed *o = after_lane >= 0 ? find(after_lane, L.after.loss) : nullptr;
      if (o)
        o->due = true;
      else if (after_lane < 0)
        owed_[s.lane].push_back({L.after, true});
      // (else: launched and already reduced - nothing is owed)
    }
    // this plan's earlier launch: still unreduced -> reduce it before its
    // partials are overwritten (the kernels refuse to fold their own buffer);
    // last written on the other lane -> order the two launches by an edge
    for (int m = 0; m < 2; ++m) {
      if (Owed *o = find(m, L.loss)) {
        s.pre = o->r, s.pre_lane = m;
        owed_[m].erase(owed_[m].begin() + (o - owed_[m].data()));
        break;
      }
    }
    const int w = writer_of(L.loss);
    if (w >= 0 && w != s.lane) s.edge_from = w;
    // the kernel's own reduction: the oldest due one of its lane
    for (size_t i = 0; i < owed_[s.lane].size(); ++i) {
      if (owed_[s.lane][i].due) {
        s.fold = owed_[s.lane][i].r;
        owed_[s.lane].erase(owed_[s.lane].begin() + i);
        break;
      }
    }
    owed_[s.lane].push_back({ChainReduce{L.partials, L.count, L.loss}, false});
    set_writer(L.loss, s.lane);
    last_lane_ = s.lane;
    lane1_used_ = lane1_used_ || s.lane == 1;
    ++launches_;
    return s;
  }

  ChainFlush flush() {
    ChainFlush f;
    for (int m = 0; m < 2; ++m)
      for (const Owed &o : owed_[m]) f.reduce[m].push_back(o.r);
    f.join = lane1_used_;
    *this = LaunchChain();
    return f;
  }

 private:
  struct Owed {
    ChainReduce r;
    bool due;  // a later launch named it as `after`
  };
  struct Writer {
    const float *loss;
    int lane;
  };

  Owed *find(int lane, const float *loss) {
    for (Owed &o : owed_[lane])
      if (o.r.loss == loss) return &o;
    return nullptr;
  }
  int writer_of(const float *loss) const {
    for (const Writer &w : writers_)
      if (w.loss == loss) return w.lane;
    return -1;
  }
  void set_writer(const float *loss, int lane) {
    for (Writer &w : writers_)
      if (w.loss == loss) {
        w.lane = lane;
        return;
      }
    writers_.push_back({loss, lane});
  }

  std::vector<Owed> owed_[2];     // reductions not yet enqueued, producer order
  std::vector<Writer> writers_;   // lane of each plan's latest launch
  int launches_ = 0;
  int last_lane_ = 0;
  bool lane1_used_ = false;
};

}  // namespace apg
