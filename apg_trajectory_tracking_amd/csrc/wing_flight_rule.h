// wing_flight_rule.h - FixedWingEvaluator.fly_to_point (scripts/
// evaluate_fixed_wing.py:45-131) for ONE flight, whatever the controller is:
// SimpleWingEnv.zero_reset or a given start, project_to_line
// (neural_control/trajectory/q_funcs.py:6-18), the target switch with the line
// moved to the current position, the miss distance on the segment prev -> pos,
// the failure test after the target test, and on failure the break
// (test_time) or the reset onto the line at des_speed with zero attitude and
// rates.  The controller goes on seeing the last SIMULATED state (`obs`) after a
// reset, as in the reference (:124 resets the environment only).
// Shared by wing_mpc_closed_loop_kernel (wing_mpc.hip, one flight per lane) and
// its host twin (cpu_twins.hip).  wing_closed_loop_kernel (mlp_wing.hip) has
// the same rule written inline around its MFMA policy, 32 flights per wave;
// oracle.torch_port.wing_closed_loop is its restatement.  The argument rules of
// an ApgWingFlight (wing_flight_check) and the reset speed are stated here for
// all three.
#pragma once
#include <math.h>

#include "apg_device.h"

namespace apg {
namespace {

// the speed of SimpleWingEnv.zero_reset and of a flight put back onto its line
constexpr float kWingDesSpeed = 11.5f;

struct WingFlightRule {
  float thresh_div, thresh_stable, des_speed;
  int n_targets, test_time, T;
};

// Argument rules of an ApgWingFlight, shared by the two device entry points and
// the host twin; NULL: fine, and `rule` is filled in.  What max_steps may be is
// the entry point's own rule (include/apg.h).
inline const char *wing_flight_check(const ApgWingFlight *f, int B, WingFlightRule *rule) {
  if (!f) return "flight is NULL";
  if (f->n_targets < 1) return "n_targets must be >= 1";
  if (B > 0 && f->max_steps > 0 &&
      (!f->targets || !f->div_linear || !f->div_pass || !f->div_fail || !f->steps))
    return "NULL buffer";
  *rule = WingFlightRule{f->thresh_div, f->thresh_stable, kWingDesSpeed, f->n_targets,
                         f->test_time ? 1 : 0, f->max_steps};
  return nullptr;
}

// a + ab (ab . (p - a)) / |ab|^2, and a itself for a degenerate line
__host__ __device__ __forceinline__ void wing_project_to_line(const float (&a)[3],
                                                              const float (&b)[3],
                                                              const float (&p)[3],
                                                              float (&out)[3]) {
  const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float n2 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2];
  const float d = ab[0] * (p[0] - a[0]) + ab[1] * (p[1] - a[1]) + ab[2] * (p[2] - a[2]);
  const float f = n2 > 0.f ? d / n2 : 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = a[j] + ab[j] * f;
}

__host__ __device__ __forceinline__ float wing_dist3(const float (&a)[3], const float (&b)[3]) {
  const float x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
  return sqrtf(x * x + y * y + z * z);
}

// One flight: the environment's state `s`, what the controller sees `obs`, the
// start of the current line, the position before the last step, the index of
// the current target, len(drone_traj) so far.
struct WingFlightBook {
  float s[12], obs[12], line[3], prev[3];
  int ti, steps;
  bool alive;
};

// what a step appends: div_to_linear, and to div_target when a target is
// passed / on divergence (-1: nothing)
struct WingFlightStep {
  float div, d_pass, d_fail;
};

// state0: the start, or NULL for zero_reset (zeros, u = kWingDesSpeed); load(i): its
// component i
template <class Load>
__host__ __device__ __forceinline__ void wing_flight_start(WingFlightBook &f, bool given,
                                                           Load &&load, bool live) {
#pragma unroll
  for (int i = 0; i < 12; ++i) f.s[i] = given ? load(i) : (i == 3 ? kWingDesSpeed : 0.f);
#pragma unroll
  for (int i = 0; i < 12; ++i) f.obs[i] = f.s[i];
#pragma unroll
  for (int j = 0; j < 3; ++j) f.line[j] = f.prev[j] = f.s[j];
  f.ti = 0, f.steps = 0;
  f.alive = live;
}

// After the environment's step k towards the target `tg` (f.s: the new state).
__host__ __device__ __forceinline__ WingFlightStep wing_flight_book(const WingFlightRule &r,
                                                                    WingFlightBook &f, int k,
                                                                    const float (&tg)[3]) {
  float(&s)[12] = f.s;
#pragma unroll
  for (int i = 0; i < 12; ++i) f.obs[i] = s[i];
  const bool stable = fabsf(s[6]) < r.thresh_stable && fabsf(s[7]) < r.thresh_stable;
  const float pos[3] = {s[0], s[1], s[2]};
  float on_line[3];
  wing_project_to_line(f.line, tg, pos, on_line);
  WingFlightStep out = {wing_dist3(on_line, pos), -1.f, -1.f};
  bool done = false;
  if (pos[0] > tg[0]) {  // passed the target: miss distance on the last segment
    float on_seg[3];
    wing_project_to_line(f.prev, pos, tg, on_seg);
    out.d_pass = wing_dist3(on_seg, tg);
    if (f.ti < r.n_targets - 1) {
      ++f.ti;
#pragma unroll
      for (int j = 0; j < 3; ++j) f.line[j] = pos[j];
    } else {
      done = true;
    }
  }
  if (!done && (!stable || out.div > r.thresh_div)) {
    out.d_fail = r.thresh_div;
    if (r.test_time) {
      out.d_fail = wing_dist3(pos, tg);
      done = true;
    } else {  // continue on the line, flying towards the (old) target
      const float v[3] = {tg[0] - on_line[0], tg[1] - on_line[1], tg[2] - on_line[2]};
      const float vn = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        s[j] = on_line[j];
        s[3 + j] = v[j] / vn * r.des_speed;
        s[6 + j] = 0.f;
        s[9 + j] = 0.f;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) f.prev[j] = pos[j];
  if (f.alive) f.steps = k + 1;
  f.alive = f.alive && !done;
  return out;
}

}  // namespace
}  // namespace apg
