// cart_flight_rule.h - the bookkeeping of ONE closed-loop cart-pole episode
// (include/apg.h: apg_cartpole_mlp_closed_loop's contract), shared by the MPC
// closed-loop kernel of cartpole_mpc.hip and its host twin (cpu_twins.hip):
// CartPoleEnv._step's theta wrap, which steps are recorded, when a balance
// flight stops, the upright flag and the fp64 sums.  Restated from
// scripts/evaluate_cartpole.py:79-318 and neural_control/environments/
// cartpole_env.py:57-82, as cart_closed_loop_kernel (mlp_cartpole.hip) has it.
// The argument rules of an ApgCartpoleFlight (cart_flight_check) are stated
// here for every entry point, mlp_cartpole.hip's included.
#pragma once
#include <math.h>

#include "apg_device.h"

namespace apg {
namespace {

struct CartFlightBook {   // one episode's running record
  double vel_sum = 0.0, vel_sq = 0.0;   // sum / sum of squares of the recorded |x_dot|
  int steps = 0;                        // steps taken
  bool alive = true, upright = true;
};

struct CartFlightRule {
  int T, mode, burn_in;
  float thresh_div;

  // `if theta > pi: theta -= 2 pi; if theta <= -pi: theta += 2 pi`, both
  // comparisons with the ORIGINAL theta, in fp32: atan2f's -fp32(pi) becomes
  // +fp32(pi), +fp32(pi) stays
  __host__ __device__ __forceinline__ static float wrap(float th) {
    const float pi = 3.14159265358979323846f, two_pi = 2.f * pi;
    float out = th;
    if (th > pi) out = th - two_pi;
    if (th <= -pi) out = two_pi + th;
    return out;
  }

  // Books the state `s` that step k landed in (after the wrap).  Swing-up:
  // never stops; |x_dot| is recorded for steps k > burn_in, where theta > 1
  // clears the upright flag.  Balance: |x_dot| is recorded every step taken;
  // the episode stops after the first step whose theta is not inside
  // (-thresh_div, thresh_div).  Rows of an episode are written while
  // f.alive holds BEFORE this call.
  __host__ __device__ __forceinline__ void book(int k, const float (&s)[4],
                                                CartFlightBook &f) const {
    const double v = (double)fabsf(s[1]);
    bool done = false;
    if (mode == APG_CARTPOLE_SWINGUP) {
      if (k > burn_in) {
        f.vel_sum += v, f.vel_sq += v * v;
        if (s[2] > 1.f) f.upright = false;
      }
    } else if (f.alive) {
      f.vel_sum += v, f.vel_sq += v * v;
      if (!(-thresh_div < s[2] && s[2] < thresh_div)) {
        done = true;
        f.upright = false;
      }
    }
    if (f.alive) f.steps = k + 1;
    f.alive = f.alive && !done;
  }
};

// Argument rules of an ApgCartpoleFlight, shared by the four device entry
// points and the host twins; NULL: fine, and `rule` is filled in
inline const char *cart_flight_check(const ApgCartpoleFlight *f, int B, CartFlightRule *rule) {
  if (!f) return "flight is NULL";
  if (B < 1 || f->max_steps < 1) return "B and max_steps must be >= 1";
  if (f->mode != APG_CARTPOLE_BALANCE && f->mode != APG_CARTPOLE_SWINGUP) return "unknown mode";
  if (!f->state0 || !f->steps || !f->upright || !f->vel_sum || !f->vel_sq) return "NULL buffer";
  *rule = CartFlightRule{f->max_steps, f->mode, f->burn_in, f->thresh_div};
  return nullptr;
}

}  // namespace
}  // namespace apg
