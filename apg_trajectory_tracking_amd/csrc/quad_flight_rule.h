// quad_flight_rule.h - THE rule of a closed-loop quadrotor flight, the loop of
// QuadEvaluator.follow_trajectory("rand") (scripts/evaluate_drone.py:81-194),
// stated once for every controller that flies it:
//   start    zero_reset: position of reference row 0, everything else zero
//   window   rows cur+1 .. cur+H of the reference (Random.get_ref_traj,
//            neural_control/trajectory/random_traj.py:60-79); row 0 of the window
//            a step saw is reference[cur] after it: project_on_ref
//   step     controller, environment, divergence from window row 0, attitude
//            check |roll|, |pitch| < thresh_stable (drone_env.py:59-72)
//   failure  test_time: the flight ends; else reset to reference row
//            min(k+1, L-H) with zero body rates (get_current_full_state)
//   slide    while k+2 <= L-H the window advances by one row
//   log      div / steps / drone / actions / start_states (include/apg.h,
//            ApgQuadFlight), nothing written for a flight that has ended
// The two loops built from these pieces: quad_flight_half_wave (quad_flight.h,
// the network controllers' half-wave layout) and mpc_flight (quad_mpc_math.h,
// one flight per lane and the host twin).  The fixed wing and the cart-pole
// have other rules and their own loops.
#pragma once
#include "quad_math.h"

namespace apg {
namespace {

constexpr int kFlightH = 10;   // rows of the reference window

struct QuadFlightRule {
  int L, T, test_time;   // reference rows, iterations = min(max_steps, L + 1)
  float thresh_div, thresh_stable;

  __host__ __device__ __forceinline__ bool failed(const float (&s)[12], float dv) const {
    const bool stable = fabsf(s[3]) < thresh_stable && fabsf(s[4]) < thresh_stable;
    return dv > thresh_div || !stable;
  }
  // the reference row a failed flight is put back on after step k
  __host__ __device__ __forceinline__ int reset_row(int k) const {
    return k + 1 < L - kFlightH ? k + 1 : L - kFlightH;
  }
  // get_ref_traj advanced after step k: slide, fetch row k + 1 + H
  __host__ __device__ __forceinline__ bool window_advances(int k) const {
    return k + 2 <= L - kFlightH;
  }
};

// distance of the position s[0..2] from a reference row's
__host__ __device__ __forceinline__ float flight_divergence(const float (&ref)[3],
                                                            const float (&s)[12]) {
  float d2 = 0.f;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float e = ref[q] - s[q];
    d2 = fmaf(e, e, d2);
  }
  return sqrtf(d2);
}

// Argument rules of an ApgQuadFlight, shared by the device entry points and the
// host twin; NULL: fine, and `rule` is filled in
inline const char *quad_flight_check(const ApgQuadFlight *f, const ApgLearntResidual *learnt,
                                     int B, QuadFlightRule *rule) {
  if (!f) return "flight is NULL";
  if (learnt && (!learnt->linear_at || !learnt->w1 || !learnt->b1 || !learnt->w2 ||
                 !learnt->b2))
    return "learnt simulator: weight pointer is NULL";
  if (f->L <= kFlightH || f->max_steps < 1)
    return "closed loop needs L > 10 reference rows and max_steps >= 1";
  static_assert(kFlightH == 10, "the message above");
  if (B > 0 && (!f->traj || !f->div || !f->steps)) return "NULL buffer";
  rule->L = f->L, rule->test_time = f->test_time;
  rule->T = f->max_steps < f->L + 1 ? f->max_steps : f->L + 1;
  rule->thresh_div = f->thresh_div, rule->thresh_stable = f->thresh_stable;
  return nullptr;
}

}  // namespace
}  // namespace apg
