// quad_flight.h - the closed-loop flight of quad_flight_rule.h in the half-wave
// layout of the in-kernel network policies (policy_mfma.h: a wave owns 32
// flights, lane l works for flight l & 31, both half-waves carry the same
// state).  mlp_closed_loop_kernel (mlp_rollout.hip) and lstm_closed_loop_kernel
// (lstm.hip) fill their tables and hand their policy in as a callable; the
// loop, the environment step and the log are here.
#pragma once
#include "policy_mfma.h"
#include "quad_math.h"
#include "learnt_residual.h"
#include "quad_flight_rule.h"

namespace apg {
namespace {

struct QuadFlightArgs {
  const float *traj;  // [L][9][B] (position, euler, velocity) rows
  float *div;         // [T][B]
  int *steps;         // [B] iterations executed
  float *drone;       // [T+1][12][B] or NULL: states after each step
  float *actions;     // [T][4][B] or NULL
  float *start;       // [T][12][B] or NULL: states the policy saw
  QuadConst c;
  int B;
  QuadFlightRule rule;
};

// Host side of the two entry points: the flight's argument rules
// (quad_flight_check) and the range of the unsigned 32-bit byte offsets the
// planes above are addressed with, then A's flight part (`c` excepted)
inline int set_flight(QuadFlightArgs &A, const ApgQuadFlight *f,
                      const ApgLearntResidual *learnt, int B) {
  if (const char *e = quad_flight_check(f, learnt, B, &A.rule)) {
    set_error("%s", e);
    return APG_ERR_ARG;
  }
  const long long drone = (long long)(A.rule.T + 1) * 12, traj = (long long)f->L * 9;
  if ((long long)B * 4 * (drone > traj ? drone : traj) >= (1ll << 32) - 64) {
    set_error("B * steps too large for 32-bit plane offsets; split the batch");
    return APG_ERR_ARG;
  }
  A.traj = f->traj, A.div = f->div, A.steps = f->steps, A.drone = f->drone;
  A.actions = f->actions, A.start = f->start_states, A.B = B;
  return APG_OK;
}

// policy(s, t, w, act): the state, its sin / cos, the window rows cur+1 .. cur+H
// (this half-wave's columns, raw values) -> the four clipped actions.
// LEARNT: the environment is a LearntDynamics whose packed weights are at
// learnt_lds (a second instantiation, so that the analytic loop keeps its
// registers).  THREADS: the workgroup's.
template <bool LEARNT, int THREADS, class Policy>
__device__ __forceinline__ void quad_flight_half_wave(const QuadFlightArgs &A,
                                                      const float *learnt_lds,
                                                      Policy &&policy) {
  constexpr int kH = kFlightH;
  const int lane = threadIdx.x & 63, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = (blockIdx.x * (THREADS / 64) + wave) * 32 + (lane & 31);
  const int B = A.B, T = A.rule.T;
  const bool live = b < B;
  const bool st_lo = live && hi == 0;
  const unsigned pitchB = (unsigned)B * 4u;
  const QuadConst c = A.c;
  // a NULL output becomes an empty buffer: every store to it is dropped
  const Planes Ptr(A.traj, A.rule.L * 9, pitchB), Pdv(A.div, T, pitchB);
  const Planes Pdr(A.drone, A.drone ? (T + 1) * 12 : 0, pitchB);
  const Planes Pac(A.actions, A.actions ? T * 4 : 0, pitchB);
  const Planes Pss(A.start, A.start ? T * 12 : 0, pitchB);
  const unsigned vb = live ? (unsigned)b * 4u : kDead;
  // window columns of this half-wave: lower (x, y, z, vx, -), upper (vy, vz,
  // vx, vy, vz) - policy channels 0-3 / 4-8 (see cfwd_weight); trajectory
  // columns 6..8 are the velocity
  unsigned vcol[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int lo = j < 3 ? j : 6, up = j < 2 ? 7 + j : 4 + j;
    vcol[j] = live ? vb + (unsigned)(hi ? up : lo) * pitchB : kDead;
  }
  float s[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = i < 3 ? Ptr.ld(vb, i * pitchB) : 0.f;  // zero_reset
  float w[kH][5];  // rows cur + 1 .. cur + H of the trajectory
#pragma unroll
  for (int r = 0; r < kH; ++r)
#pragma unroll
    for (int j = 0; j < 5; ++j) w[r][j] = Ptr.ld(vcol[j], ((1 + r) * 9) * pitchB);
#pragma unroll
  for (int i = 0; i < 12; ++i) Pdr.st(st_lo ? vb : kDead, i * pitchB, s[i]);
  bool alive = live;
  int steps = 0;

#pragma unroll 1
  for (int k = 0; k < T; ++k) {
    const unsigned pB = opaque(pitchB);
    const unsigned vrec = (alive && hi == 0) ? vb : kDead;
#pragma unroll
    for (int i = 0; i < 12; ++i) Pss.st(vrec, (k * 12 + i) * pB, s[i]);
    const Trig t = make_trig(&s[3]);
    float act[4];
    policy(s, t, w, act);
#pragma unroll
    for (int j = 0; j < 4; ++j) Pac.st(vrec, (k * 4 + j) * pB, act[j]);
    if (LEARNT) learnt_quad_step(s, act, c, t, learnt_lds, hi);
    else quad_step(s, act, c, t);
    // window row 0 is reference[cur] after get_ref_traj: project_on_ref (the
    // position columns are the lower half-wave's)
    float ref[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float oth = other_half(w[0][q]);
      ref[q] = hi ? oth : w[0][q];
    }
    const float dv = flight_divergence(ref, s);
    const bool failed = A.rule.failed(s, dv);
#pragma unroll
    for (int i = 0; i < 12; ++i) Pdr.st(vrec, ((k + 1) * 12 + i) * pB, s[i]);
    Pdv.st(vrec, k * pB, dv);
    if (alive) steps = k + 1;
    if (A.rule.test_time) {
      alive = alive && !failed;
      if (!__any(alive)) break;
    } else if (__any(failed)) {  // get_current_full_state: row cur, zero rates
      const int cur = A.rule.reset_row(k);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const float rv = Ptr.ld(vb, (cur * 9 + i) * pB);
        s[i] = failed ? rv : s[i];
      }
#pragma unroll
      for (int i = 9; i < 12; ++i) s[i] = failed ? 0.f : s[i];
    }
    if (A.rule.window_advances(k)) {
#pragma unroll
      for (int r = 0; r + 1 < kH; ++r)
#pragma unroll
        for (int j = 0; j < 5; ++j) w[r][j] = w[r + 1][j];
#pragma unroll
      for (int j = 0; j < 5; ++j) w[kH - 1][j] = Ptr.ld(vcol[j], ((k + 1 + kH) * 9) * pB);
    }
  }
  if (st_lo) A.steps[b] = steps;
}

}  // namespace
}  // namespace apg
