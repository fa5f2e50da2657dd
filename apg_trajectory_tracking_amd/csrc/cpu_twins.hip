// libapg_cpu.so (include/apg_cpu.h): the host twins of the dynamics entry
// points - the SAME per-trajectory headers the GPU kernels call per lane
// (quad_math.h, wing_math.h, cartpole_math.h), compiled for the host
// (hipcc --cuda-host-only) and looped over the batch.  Separate library,
// separate symbol names, never loaded by the Python package: not a fallback.
// The compositions (forward sweep, loss terms and their seeds, reverse sweep)
// follow the rollout kernels of quad.hip / wing.hip lane for lane; the
// cart-pole and plain fixed-wing ones are the kernels' own bodies
// (cartpole_rollout_math.h, wing_rollout_math.h).  tests/test_cpu_twins.py pins
// them to the golden vectors and, on a GPU, to the device entry points.
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "apg_cpu.h"
#include "apg_cpu_cartpole_fit.h"
#include "apg_cpu_cartpole_learnt_train.h"
#include "apg_cpu_cartpole_train.h"
#include "apg_cpu_launch_chain.h"
#include "apg_cpu_quad_fit.h"
#include "apg_cpu_wing_fit.h"
#include "apg_cpu_wing_learnt.h"
#include "cartpole_fit_math.h"
#include "cartpole_learnt_math.h"
#include "cartpole_math.h"
#include "cartpole_mpc_math.h"
#include "cartpole_rollout_math.h"
#include "cartpole_train_math.h"
#include "launch_chain.h"
#include "quad_fit_math.h"
#include "quad_learnt_mpc_math.h"
#include "quad_math.h"
#include "quad_mpc_math.h"
#include "static_dispatch.h"
#include "wing_learnt_math.h"
#include "wing_math.h"
#include "wing_mpc_math.h"
#include "wing_rollout_math.h"

using namespace apg;

namespace {

thread_local char g_err[512] = "";

int fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return APG_ERR_ARG;
}

// element addresses of the three layouts of apg.h
struct Idx {
  int layout;
  size_t B;
  // component i of an S-component per-trajectory vector (state, action, cotangent)
  size_t vec(int b, int i, int S) const {
    if (layout == APG_LAYOUT_AOS) return (size_t)b * S + i;
    if (layout == APG_LAYOUT_SOA) return (size_t)i * B + b;
    return ((size_t)(i >> 2) * B + b) * 4 + (i & 3);          // [S/4][B][4]
  }
  // column c of row k of an [H][C] per-trajectory sequence
  size_t seq(int b, int k, int c, int H, int C) const {
    if (layout == APG_LAYOUT_AOS) return ((size_t)b * H + k) * C + c;
    if (layout == APG_LAYOUT_SOA) return ((size_t)k * C + c) * B + b;
    return ((size_t)k * B + b) * C + c;                        // [H][B][C]
  }
  // component i of the state after step k (states_out)
  size_t states(int b, int k, int i, int H, int S) const {
    if (layout == APG_LAYOUT_PACKED)                           // [H][S/4][B][4]
      return (((size_t)k * (S / 4) + (i >> 2)) * B + b) * 4 + (i & 3);
    return seq(b, k, i, H, S);
  }
};

int check_common(const void *params, int B, int layout, bool packed_ok) {
  if (B < 0) return fail("B must be >= 0 (got %d)", B);
  if (layout != APG_LAYOUT_AOS && layout != APG_LAYOUT_SOA &&
      !(packed_ok && layout == APG_LAYOUT_PACKED))
    return fail("unknown layout %d", layout);
  if (!params) return fail("params is NULL");
  return APG_OK;
}

int check_h(int H) {
  if (H < 1 || H > APG_MAX_HORIZON)
    return fail("H must be in [1, %d] (got %d)", APG_MAX_HORIZON, H);
  return APG_OK;
}

// one partial per 64 trajectories, then their fixed-order sum
struct LossOut {
  float *partials, *loss;
  float wave = 0.f;
  void add(int b, int B, float v) {
    wave += v;
    if ((b & 63) == 63 || b == B - 1) partials[b >> 6] = wave, wave = 0.f;
  }
  void finish(int B) {
    if (!loss) return;
    float s = 0.f;
    for (int i = 0; i < (B + 63) / 64; ++i) s += partials[i];
    *loss = s;
  }
};

// The host twins of the fused simulator fits: fit_body and fit_reduce of
// residual_fit.h on the traits T, lane for lane.  The common checks, then per
// sample, in order: T::sample, the head and every hidden unit's cotangents
// added into ONE partial row; then the norms and fit_scatter per element.
// model_error: the outcome of the entry point's own model checks; make(): the
// model (asked for once the arguments hold); t: the residual's tensors, for the
// regulariser (T::REG).
template <class T, class Make>
int fit_host(const char *model_error, const float *state, const float *action,
             const float *target, const typename T::Eval *eval, float l2_lambda, int B,
             float *loss_partials, float *loss, float *grad, const typename T::Scale &scale,
             const ResidualTensors &t, Make &&make) {
  if (B < 0) return fail("B must be >= 0 (got %d)", B);
  if (model_error) return fail("%s", model_error);
  if ((target != nullptr) == (eval != nullptr))
    return fail("exactly one of target / eval_params must be given");
  if (!(l2_lambda >= 0.f)) return fail("l2_lambda must be >= 0");
  if (!grad) return fail("grad is NULL");
  for (int i = 0; i < T::GRADS; ++i) grad[i] = 0.f;
  if (B == 0) {
    if (loss) *loss = 0.f;
    return APG_OK;
  }
  if (!state || !action || !loss_partials)
    return fail("state / action / loss_partials must not be NULL");
  const auto m = make();
  std::vector<float> acc(T::ROW, 0.f);
  LossOut out{loss_partials, loss};
  for (int b = 0; b < B; ++b) {
    float s[T::S], a[T::A], tgt[T::S], lam[T::OUT], z[T::IN], hd[T::USED];
    for (int i = 0; i < T::S; ++i) s[i] = state[(size_t)b * T::S + i];
    for (int i = 0; i < T::A; ++i) a[i] = action[(size_t)b * T::A + i];
    if (!eval)
      for (int i = 0; i < T::S; ++i) tgt[i] = target[(size_t)b * T::S + i];
    const float l = T::sample(m, s, a, tgt, eval, lam, z, hd);
    for (int i = 0; i < T::USED; ++i) acc[i] += hd[i];
    for (int u = 0; u < kResHidden; ++u) {
      float gw[T::UNIT] = {0.f};
      residual_unit_grads<T::IN, T::OUT, T::RW2, T::RB1, T::UW2, T::UB1>(
          m.rows + u * T::RES_ROW, z, lam, gw);
      for (int j = 0; j < T::UNIT; ++j) acc[T::HEAD + j * kResHidden + u] += gw[j];
    }
    out.add(b, B, l);
  }
  out.finish(B);
  float norms[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (T::REG)
    if (l2_lambda > 0.f) {
      const float *tens[4] = {t.w2, t.b2, t.w1, t.b1};
      const int count[4] = {T::OUT * kResHidden, T::OUT, kResHidden * T::IN, kResHidden};
      for (int q = 0; q < 4; ++q) {
        float ss = 0.f;
        for (int i = 0; i < count[q]; ++i) ss = fmaf(tens[q][i], tens[q][i], ss);
        norms[q] = sqrtf(ss);
      }
      if (loss) *loss += fit_penalty(l2_lambda, norms);
    }
  for (int c = 0; c < T::ROW; ++c) fit_scatter<T>(c, acc[c], scale, t, norms, l2_lambda, grad);
  return APG_OK;
}

int run_deferred(const ApgDeferredLoss *d) {
  if (!d) return APG_OK;
  if (!d->prev_loss || d->prev_count < 0 || (d->prev_count > 0 && !d->prev_partials))
    return fail("deferred: prev_loss NULL, prev_count < 0 or prev_partials NULL");
  float s = 0.f;
  for (int i = 0; i < d->prev_count; ++i) s += d->prev_partials[i];
  *d->prev_loss = s;
  return APG_OK;
}

// cartpole_rollout_math.h / wing_rollout_math.h looped over the batch, the
// stash a vector: what the rollout kernels do per lane
template <class Step, class Adjoint>
void cart_rollout_batch(const float *state0, const float *actions, int B, int H, const Idx &ix,
                        LossOut out, float *grad_actions, float *grad_state0,
                        float *states_out, Step &&step, Adjoint &&adjoint) {
  std::vector<float> pre((size_t)H * 4);
  auto ST = [&](int k, int i) -> float & { return pre[k * 4 + i]; };
  for (int b = 0; b < B; ++b) {
    auto action = [&](int k) { return actions[ix.seq(b, k, 0, H, 1)]; };
    auto emit_state = [&](int k, const float (&x)[4]) {
      for (int i = 0; states_out && i < 4; ++i) states_out[ix.seq(b, k, i, H, 4)] = x[i];
    };
    auto emit_grad = [&](int k, float g) { grad_actions[ix.seq(b, k, 0, H, 1)] = g; };
    float s0[4], s[4], lam[4];
    for (int i = 0; i < 4; ++i) s0[i] = state0[ix.vec(b, i, 4)];
    out.add(b, B, cart_rollout_forward(H, s0, s, action, ST, step, emit_state));
    cart_rollout_reverse(H, s0, s, lam, action, ST, adjoint, emit_grad);
    for (int i = 0; grad_state0 && i < 4; ++i) grad_state0[ix.vec(b, i, 4)] = lam[i];
  }
  out.finish(B);
}

template <class Step, class Adjoint>
void wing_rollout_batch(const float *state0, const float *actions, const float *ref,
                        const ApgWingLossWeights &w, int B, int H, const Idx &ix, LossOut out,
                        float *grad_actions, float *grad_state0, float *states_out,
                        Step &&step, Adjoint &&adjoint) {
  std::vector<float> pre((size_t)H * 12);
  auto ST = [&](int k, int i) -> float & { return pre[k * 12 + i]; };
  for (int b = 0; b < B; ++b) {
    auto action = [&](int k, float (&a)[4]) {
      for (int j = 0; j < 4; ++j) a[j] = actions[ix.seq(b, k, j, H, 4)];
    };
    auto rf = [&](int k, float (&rp)[3]) {
      for (int i = 0; i < 3; ++i) rp[i] = ref[ix.seq(b, k, i, H, 3)];
    };
    auto emit_state = [&](int k, const float (&x)[12]) {
      for (int i = 0; states_out && i < 12; ++i) states_out[ix.seq(b, k, i, H, 12)] = x[i];
    };
    auto emit_grad = [&](int k, const float (&ga)[4]) {
      for (int j = 0; j < 4; ++j) grad_actions[ix.seq(b, k, j, H, 4)] = ga[j];
    };
    float s[12], lam[12];
    for (int i = 0; i < 12; ++i) s[i] = state0[ix.vec(b, i, 12)];
    out.add(b, B, wing_rollout_forward(H, s, w.pos, w.action, action, rf, ST, step, emit_state));
    wing_rollout_reverse(H, s, lam, w.pos, w.action, action, rf, ST, adjoint, emit_grad);
    for (int i = 0; grad_state0 && i < 12; ++i) grad_state0[ix.vec(b, i, 12)] = lam[i];
  }
  out.finish(B);
}

}  // namespace

extern "C" {

int apg_cpu_version(void) { return APG_VERSION_MAJOR * 1000 + APG_VERSION_MINOR; }
const char *apg_cpu_last_error_string(void) { return g_err; }

// ------------------------------------------------------------------ quad
int apg_quad_step_fwd_cpu(const float *state, const float *action, float dt,
                          const ApgQuadParams *params, int B, int layout,
                          float *next_state) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state || !action)) return fail("NULL input pointer");
  if (!next_state) return fail("next_state is NULL");
  const QuadConst c = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  for (int b = 0; b < B; ++b) {
    float s[12], a[4];
    for (int i = 0; i < 12; ++i) s[i] = state[ix.vec(b, i, 12)];
    for (int i = 0; i < 4; ++i) a[i] = action[ix.vec(b, i, 4)];
    const Trig t = make_trig(&s[3]);
    quad_step(s, a, c, t);
    for (int i = 0; i < 12; ++i) next_state[ix.vec(b, i, 12)] = s[i];
  }
  return APG_OK;
}

int apg_quad_step_bwd_cpu(const float *state, const float *action, float dt,
                          const ApgQuadParams *params, int B, int layout,
                          const float *grad_next, float *grad_state,
                          float *grad_action) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state || !action)) return fail("NULL input pointer");
  if (!grad_next) return fail("grad_next is NULL");
  const QuadConst c = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  for (int b = 0; b < B; ++b) {
    float s[12], lam[12], ga[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 12; ++i) s[i] = state[ix.vec(b, i, 12)];
    for (int i = 0; i < 12; ++i) lam[i] = grad_next[ix.vec(b, i, 12)];
    const Trig t = make_trig(&s[3]);
    quad_step_adjoint(lam, ga, action[ix.vec(b, 0, 4)], &s[9], c, t);
    if (grad_state)
      for (int i = 0; i < 12; ++i) grad_state[ix.vec(b, i, 12)] = lam[i];
    if (grad_action)
      for (int i = 0; i < 4; ++i) grad_action[ix.vec(b, i, 4)] = ga[i];
  }
  return APG_OK;
}

int apg_quad_rollout_fwd_bwd_cpu(const float *state0, const float *actions,
                                 const float *ref, int ref_cols, float dt,
                                 const ApgQuadParams *params,
                                 const ApgQuadLossWeights *weights, int B, int H,
                                 int layout, float *loss_partials, float *loss,
                                 float *grad_actions, float *grad_state0,
                                 float *states_out,
                                 const ApgDeferredLoss *deferred) {
  if (int e = check_common(params, B, layout, true)) return e;
  if (B > 0 && (!state0 || !actions)) return fail("NULL input pointer");
  if (!weights) return fail("weights is NULL");
  if (int e = run_deferred(deferred)) return e;
  if (int e = check_h(H)) return e;
  if (ref_cols != 9 && ref_cols != 6)
    return fail("ref_cols must be 9 ([pos, euler, vel]) or 6 ([pos, vel])");
  if (layout == APG_LAYOUT_PACKED && H != 5 && H != 10)
    return fail("APG_LAYOUT_PACKED: H must be 5 or 10 (got %d)", H);
  if (layout == APG_LAYOUT_PACKED && ref_cols != 6)
    return fail("APG_LAYOUT_PACKED: ref rows are [pos, vel] (ref_cols = 6)");
  if (!ref || !loss_partials || !grad_actions)
    return fail("ref / loss_partials / grad_actions must not be NULL");
  const QuadConst c = make_const(*params, dt);
  const ApgQuadLossWeights &w = *weights;
  const Idx ix{layout, (size_t)B};
  const int vc = ref_cols == 9 ? 6 : 3;
  LossOut out{loss_partials, loss};
  std::vector<Trig> trig(H);
  std::vector<float> st((size_t)H * 12), wold((size_t)H * 3);
  for (int b = 0; b < B; ++b) {
    float s[12];
    for (int i = 0; i < 12; ++i) s[i] = state0[ix.vec(b, i, 12)];
    for (int k = 0; k < H; ++k) {
      for (int i = 0; i < 3; ++i) wold[k * 3 + i] = s[9 + i];
      trig[k] = make_trig(&s[3]);
      float a[4];
      for (int j = 0; j < 4; ++j) a[j] = actions[ix.seq(b, k, j, H, 4)];
      quad_step(s, a, c, trig[k]);
      for (int i = 0; i < 12; ++i) st[k * 12 + i] = s[i];
      if (states_out)
        for (int i = 0; i < 12; ++i) states_out[ix.states(b, k, i, H, 12)] = s[i];
    }
    // quad_mpc_loss (neural_control/drone_loss.py:12-39) and its seeds, then the
    // adjoint of step k - as quad_rollout_kernel's reverse sweep
    float lam[12] = {0.f}, l = 0.f;
    for (int k = H - 1; k >= 0; --k) {
      const float *x = &st[k * 12];
      float a[4], ga[4], lp = 0.f, lv = 0.f, lw = 0.f, lr = 0.f;
      for (int j = 0; j < 4; ++j) a[j] = actions[ix.seq(b, k, j, H, 4)];
      for (int i = 0; i < 3; ++i) {
        const float dp = x[i] - ref[ix.seq(b, k, i, H, ref_cols)];
        const float dv = x[6 + i] - ref[ix.seq(b, k, vc + i, H, ref_cols)];
        const float wn = x[9 + i];
        lp += dp * dp, lv += dv * dv, lw += wn * wn;
        lam[i] += 2.f * w.pos * dp;
        lam[6 + i] += 2.f * w.vel * dv;
        lam[9 + i] += 2.f * w.av * wn;
      }
      const float da0 = a[0] - 0.5f;
      ga[0] = 2.f * w.thrust * da0;
      for (int j = 1; j < 4; ++j) {
        const float d = a[j] - 0.5f;
        lr += d * d;
        ga[j] = 2.f * w.rates * d;
      }
      l += w.pos * lp + w.vel * lv + w.av * lw + w.rates * lr + w.thrust * da0 * da0;
      const float wo[3] = {wold[k * 3], wold[k * 3 + 1], wold[k * 3 + 2]};
      quad_step_adjoint(lam, ga, a[0], wo, c, trig[k]);
      for (int j = 0; j < 4; ++j) grad_actions[ix.seq(b, k, j, H, 4)] = ga[j];
    }
    if (grad_state0)
      for (int i = 0; i < 12; ++i) grad_state0[ix.vec(b, i, 12)] = lam[i];
    out.add(b, B, l);
  }
  out.finish(B);
  return APG_OK;
}

int apg_quad_rollout_fwd_cpu(const float *state0, const float *actions, float dt,
                             const ApgQuadParams *params, int B, int H, int layout,
                             float *states_out) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state0 || !actions)) return fail("NULL input pointer");
  if (H < 1) return fail("H must be >= 1 (got %d)", H);
  if (!states_out) return fail("states_out is NULL");
  const QuadConst c = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  for (int b = 0; b < B; ++b) {
    float s[12];
    for (int i = 0; i < 12; ++i) s[i] = state0[ix.vec(b, i, 12)];
    for (int k = 0; k < H; ++k) {
      float a[4];
      for (int j = 0; j < 4; ++j) a[j] = actions[ix.seq(b, k, j, H, 4)];
      quad_step(s, a, c, make_trig(&s[3]));
      for (int i = 0; i < 12; ++i) states_out[ix.seq(b, k, i, H, 12)] = s[i];
    }
  }
  return APG_OK;
}

// ------------------------------------------------------------------ wing
int apg_wing_step_fwd_cpu(const float *state, const float *action, float dt,
                          const ApgWingParams *params, int B, int layout,
                          float *next_state) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state || !action)) return fail("NULL input pointer");
  if (!next_state) return fail("next_state is NULL");
  const WingConst k = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  for (int b = 0; b < B; ++b) {
    float s[12], a[4];
    for (int i = 0; i < 12; ++i) s[i] = state[ix.vec(b, i, 12)];
    for (int i = 0; i < 4; ++i) a[i] = action[ix.vec(b, i, 4)];
    wing_step(s, a, k);
    for (int i = 0; i < 12; ++i) next_state[ix.vec(b, i, 12)] = s[i];
  }
  return APG_OK;
}

int apg_wing_step_bwd_cpu(const float *state, const float *action, float dt,
                          const ApgWingParams *params, int B, int layout,
                          const float *grad_next, float *grad_state,
                          float *grad_action) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state || !action)) return fail("NULL input pointer");
  if (!grad_next) return fail("grad_next is NULL");
  const WingConst k = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  for (int b = 0; b < B; ++b) {
    float s[12], a[4], sd[12], lam[12], ga[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 12; ++i) s[i] = state[ix.vec(b, i, 12)];
    for (int i = 0; i < 4; ++i) a[i] = action[ix.vec(b, i, 4)];
    for (int i = 0; i < 12; ++i) lam[i] = grad_next[ix.vec(b, i, 12)];
    WingAux x;
    wing_rates(s, a, k, x, sd);
    wing_step_adjoint(lam, ga, s, x, sd, k);
    if (grad_state)
      for (int i = 0; i < 12; ++i) grad_state[ix.vec(b, i, 12)] = lam[i];
    if (grad_action)
      for (int i = 0; i < 4; ++i) grad_action[ix.vec(b, i, 4)] = ga[i];
  }
  return APG_OK;
}

int apg_wing_rollout_fwd_bwd_cpu(const float *state0, const float *actions,
                                 const float *ref, float dt,
                                 const ApgWingParams *params,
                                 const ApgWingLossWeights *weights, int B, int H,
                                 int layout, float *loss_partials, float *loss,
                                 float *grad_actions, float *grad_state0,
                                 float *states_out,
                                 const ApgDeferredLoss *deferred) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state0 || !actions)) return fail("NULL input pointer");
  if (!weights) return fail("weights is NULL");
  if (int e = run_deferred(deferred)) return e;
  if (int e = check_h(H)) return e;
  if (!ref || !loss_partials || !grad_actions)
    return fail("ref / loss_partials / grad_actions must not be NULL");
  const WingConst k = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  wing_rollout_batch(
      state0, actions, ref, *weights, B, H, ix, LossOut{loss_partials, loss}, grad_actions,
      grad_state0, states_out, [&](float (&s)[12], const float (&a)[4]) { wing_step(s, a, k); },
      [&](float (&lam)[12], float (&ga)[4], const float (&pre)[12], const float (&a)[4]) {
        WingAux x;
        float sd[12];
        wing_rates(pre, a, k, x, sd);
        wing_step_adjoint(lam, ga, pre, x, sd, k);
      });
  return APG_OK;
}

int apg_wing_rollout_fwd_cpu(const float *state0, const float *actions, float dt,
                             const ApgWingParams *params, int B, int H, int layout,
                             float *states_out) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state0 || !actions)) return fail("NULL input pointer");
  if (H < 1) return fail("H must be >= 1 (got %d)", H);
  if (!states_out) return fail("states_out is NULL");
  const WingConst k = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  for (int b = 0; b < B; ++b) {
    float s[12];
    for (int i = 0; i < 12; ++i) s[i] = state0[ix.vec(b, i, 12)];
    for (int n = 0; n < H; ++n) {
      float a[4];
      for (int j = 0; j < 4; ++j) a[j] = actions[ix.seq(b, n, j, H, 4)];
      wing_step(s, a, k);
      for (int i = 0; i < 12; ++i) states_out[ix.seq(b, n, i, H, 12)] = s[i];
    }
  }
  return APG_OK;
}

// -------------------------------------------------------------- cartpole
int apg_cartpole_step_fwd_cpu(const float *state, const float *action, float dt,
                              const ApgCartpoleParams *params, int B, int layout,
                              float *next_state) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state || !action)) return fail("NULL input pointer");
  if (!next_state) return fail("next_state is NULL");
  const CartConst c = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  for (int b = 0; b < B; ++b) {
    float s[4];
    for (int i = 0; i < 4; ++i) s[i] = state[ix.vec(b, i, 4)];
    cart_step(s, action[b], c);
    for (int i = 0; i < 4; ++i) next_state[ix.vec(b, i, 4)] = s[i];
  }
  return APG_OK;
}

int apg_cartpole_step_bwd_cpu(const float *state, const float *action, float dt,
                              const ApgCartpoleParams *params, int B, int layout,
                              const float *grad_next, float *grad_state,
                              float *grad_action) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state || !action)) return fail("NULL input pointer");
  if (!grad_next) return fail("grad_next is NULL");
  const CartConst c = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  for (int b = 0; b < B; ++b) {
    float s[4], lam[4];
    for (int i = 0; i < 4; ++i) s[i] = state[ix.vec(b, i, 4)];
    for (int i = 0; i < 4; ++i) lam[i] = grad_next[ix.vec(b, i, 4)];
    const float xd = s[1], thd = s[3];
    const CartAux x = cart_step(s, action[b], c);
    const float ga = cart_step_adjoint(lam, xd, thd, x, c);
    if (grad_state)
      for (int i = 0; i < 4; ++i) grad_state[ix.vec(b, i, 4)] = lam[i];
    if (grad_action) grad_action[b] = ga;
  }
  return APG_OK;
}

int apg_cartpole_rollout_fwd_bwd_cpu(const float *state0, const float *actions,
                                     float dt, const ApgCartpoleParams *params,
                                     int B, int H, int layout,
                                     float *loss_partials, float *loss,
                                     float *grad_actions, float *grad_state0,
                                     float *states_out) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state0 || !actions)) return fail("NULL input pointer");
  if (int e = check_h(H)) return e;
  if (!loss_partials || !grad_actions)
    return fail("loss_partials / grad_actions must not be NULL");
  const CartConst c = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  cart_rollout_batch(
      state0, actions, B, H, ix, LossOut{loss_partials, loss}, grad_actions, grad_state0,
      states_out, [&](float (&s)[4], float a) { cart_step(s, a, c); },
      [&](float (&lam)[4], const float (&pre)[4], float a) {
        return cart_step_adjoint(lam, pre[1], pre[3], cart_step_aux(pre, a, c), c);
      });
  return APG_OK;
}

int apg_cartpole_rollout_fwd_cpu(const float *state0, const float *actions, float dt,
                                 const ApgCartpoleParams *params, int B, int H,
                                 int layout, float *states_out) {
  if (int e = check_common(params, B, layout, false)) return e;
  if (B > 0 && (!state0 || !actions)) return fail("NULL input pointer");
  if (H < 1) return fail("H must be >= 1 (got %d)", H);
  if (!states_out) return fail("states_out is NULL");
  const CartConst c = make_const(*params, dt);
  const Idx ix{layout, (size_t)B};
  for (int b = 0; b < B; ++b) {
    float s[4];
    for (int i = 0; i < 4; ++i) s[i] = state0[ix.vec(b, i, 4)];
    for (int k = 0; k < H; ++k) {
      cart_step(s, actions[ix.seq(b, k, 0, H, 1)], c);
      for (int i = 0; i < 4; ++i) states_out[ix.seq(b, k, i, H, 4)] = s[i];
    }
  }
  return APG_OK;
}

}  // extern "C"

// ------------------------------------------------------- cartpole, learnt
namespace {

// the module's tensors -> step constants and the residual's unit rows (the
// kernels' LDS image); false: no residual
bool learnt_setup(const ApgCartpoleLearnt &m, float dt, CartLearntParams &p, CartConst &c,
                  std::vector<float> &rows) {
  p = CartLearntParams{*m.max_force_mag, *m.masspole, *m.length,
                       *m.friction,      *m.total_mass, *m.polemass_length};
  c = make_learnt_const(p, dt);
  if (!m.w1) return false;
  rows.resize(kCartResFloats);
  for (int t = 0; t < kCartResFloats; ++t) rows[t] = cart_residual_packed(t, m.w1, m.b1, m.w2);
  return true;
}

int check_learnt(const ApgCartpoleLearnt *m, int B, bool need_residual) {
  if (B < 0) return fail("B must be >= 0 (got %d)", B);
  if (const char *e = cart_learnt_check(m, need_residual)) return fail("%s", e);
  return APG_OK;
}

}  // namespace

extern "C" {

int apg_cartpole_learnt_step_fwd_cpu(const float *state, const float *action, float dt,
                                     const ApgCartpoleLearnt *model, int B,
                                     float *next_state) {
  if (int e = check_learnt(model, B, false)) return e;
  if (B > 0 && (!state || !action)) return fail("NULL input pointer");
  if (!next_state) return fail("next_state is NULL");
  CartLearntParams p;
  CartConst c;
  std::vector<float> rows;
  const bool res = learnt_setup(*model, dt, p, c, rows);
  for (int b = 0; b < B; ++b) {
    float s[4] = {state[b * 4], state[b * 4 + 1], state[b * 4 + 2], state[b * 4 + 3]};
    cart_learnt_step(s, action[b], c, res ? rows.data() : nullptr);
    for (int i = 0; i < 4; ++i) next_state[b * 4 + i] = s[i];
  }
  return APG_OK;
}

int apg_cartpole_learnt_step_bwd_cpu(const float *state, const float *action, float dt,
                                     const ApgCartpoleLearnt *model, int B,
                                     const float *grad_next, float *grad_state,
                                     float *grad_action, float *grad_params,
                                     float *workspace) {
  (void)workspace;
  if (int e = check_learnt(model, B, false)) return e;
  if (!grad_params) return fail("grad_params is NULL");
  if (B > 0 && (!state || !action || !grad_next)) return fail("NULL input pointer");
  CartLearntParams p;
  CartConst c;
  std::vector<float> rows;
  const bool res = learnt_setup(*model, dt, p, c, rows);
  float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  std::vector<float> gw(kCartResFloats, 0.f);   // unit-row order
  for (int b = 0; b < B; ++b) {
    float s[4], lam[4];
    for (int i = 0; i < 4; ++i) s[i] = state[b * 4 + i], lam[i] = grad_next[b * 4 + i];
    const float a = action[b];
    const float z[5] = {s[0], s[1], s[2], s[3], a}, lam0[4] = {lam[0], lam[1], lam[2], lam[3]};
    float tmp[4] = {s[0], s[1], s[2], s[3]};
    const CartAux x = cart_step(tmp, a, c);
    cart_param_adjoint(lam, a, s[1], s[3], x, p, dt, g);
    const float ga = cart_learnt_step_adjoint(lam, s, a, x, c, res ? rows.data() : nullptr);
    if (grad_state)
      for (int i = 0; i < 4; ++i) grad_state[b * 4 + i] = lam[i];
    if (grad_action) grad_action[b] = ga;
    if (res)
      for (int m = 0; m < kCartResHidden; ++m) {
        float u[kCartResRow];
        for (int j = 0; j < kCartResRow; ++j) u[j] = gw[m * kCartResRow + j];
        cart_residual_unit_grads(&rows[m * kCartResRow], z, lam0, u);
        for (int j = 0; j < kCartResRow; ++j) gw[m * kCartResRow + j] = u[j];
      }
  }
  for (int i = 0; i < kCartPhysGrads; ++i) grad_params[i] = g[i];
  for (int m = 0; m < kCartResHidden; ++m) {
    const float *u = &gw[m * kCartResRow];
    for (int j = 0; j < 5; ++j) grad_params[kCartGW1 + m * 5 + j] = u[j];
    grad_params[kCartGB1 + m] = u[5];
    for (int o = 0; o < 4; ++o) grad_params[kCartGW2 + o * kCartResHidden + m] = u[6 + o];
  }
  return APG_OK;
}

int apg_cartpole_learnt_rollout_fwd_bwd_cpu(const float *state0, const float *actions,
                                            float dt, const ApgCartpoleLearnt *model,
                                            int B, int H, int layout,
                                            float *loss_partials, float *loss,
                                            float *grad_actions, float *grad_state0,
                                            float *states_out) {
  if (int e = check_learnt(model, B, true)) return e;
  if (layout != APG_LAYOUT_AOS && layout != APG_LAYOUT_SOA)
    return fail("unknown layout %d", layout);
  if (B > 0 && (!state0 || !actions)) return fail("NULL input pointer");
  if (int e = check_h(H)) return e;
  if (!loss_partials || !grad_actions)
    return fail("loss_partials / grad_actions must not be NULL");
  CartLearntParams p;
  CartConst c;
  std::vector<float> rows;
  learnt_setup(*model, dt, p, c, rows);
  const Idx ix{layout, (size_t)B};
  cart_rollout_batch(
      state0, actions, B, H, ix, LossOut{loss_partials, loss}, grad_actions, grad_state0,
      states_out, [&](float (&s)[4], float a) { cart_learnt_step(s, a, c, rows.data()); },
      [&](float (&lam)[4], const float (&pre)[4], float a) {
        return cart_learnt_step_adjoint(lam, pre, a, cart_step_aux(pre, a, c), c, rows.data());
      });
  return APG_OK;
}

// apg_cpu_cartpole_fit.h: fit_host on CartFit (cartpole_fit_math.h)
int apg_cartpole_learnt_fit_fwd_bwd_cpu(const float *state, const float *action, float dt,
                                        const ApgCartpoleLearnt *model, const float *target,
                                        const ApgCartpoleParams *eval_params, int B,
                                        float *loss_partials, float *loss, float *grad,
                                        float *workspace) {
  (void)workspace;
  const CartConst ce = eval_params ? make_const(*eval_params, dt) : CartConst{};
  std::vector<float> rows;
  return fit_host<CartFit>(cart_learnt_check(model, true), state, action, target,
                           eval_params ? &ce : nullptr, 0.f, B, loss_partials, loss, grad,
                           FitNoScale{}, ResidualTensors{}, [&] {
                             CartFitModel m;
                             m.dt = dt;
                             learnt_setup(*model, dt, m.p, m.c, rows);
                             m.rows = rows.data();
                             return m;
                           });
}

}  // extern "C"

namespace {

// apg_cpu_cartpole_train.h: the kernels' shared body (policy_step_body,
// cartpole_train.hip) sample for sample - the layers of cartpole_train_math.h
// one unit at a time, the rollout of cartpole_rollout_math.h through the two
// step functions of `simulator` (AnalyticCart / LearntCart below; asked for
// once the other arguments hold and its own check has passed), every gradient
// element summed in sample order - then the last stage (gradient out, momentum
// SGD) element by element.  `sim`: the entry point's simulator argument, for
// the NULL check.
template <class Simulator>
int cart_policy_step_host(const float *in_state, const float *state0, const void *sim,
                          const ApgCartpolePolicy *policy, int B, int H,
                          float *loss_partials, float *loss,
                          const ApgCartpolePolicyGrads *grads, float *actions_out,
                          const ApgCartpoleSgdUpdate *update, Simulator &&simulator) {
  if (B < 1) return fail("B must be >= 1 (got %d)", B);
  if (int e = check_h(H)) return e;
  if (!sim || !policy || !grads) return fail("params / policy / grads is NULL");
  const ApgCartpolePolicy &P = *policy;
  if (!P.w0 || !P.b0 || !P.w1 || !P.b1 || !P.w2 || !P.b2 || !P.w3 || !P.b3 || !P.w_out ||
      !P.b_out)
    return fail("policy weight pointer is NULL");
  auto tensors = [](const ApgCartpolePolicyGrads &g, float *(&t)[10]) {
    float *v[10] = {g.w0, g.b0, g.w1, g.b1, g.w2, g.b2, g.w3, g.b3, g.w_out, g.b_out};
    bool all = true;
    for (int q = 0; q < 10; ++q) t[q] = v[q], all = all && v[q];
    return all;
  };
  float *tg[10], *tp[10], *tm[10];
  if (!tensors(*grads, tg)) return fail("grads: pointer is NULL");
  if (update && (!tensors(update->param, tp) || !tensors(update->momentum_buf, tm)))
    return fail("update: parameter / momentum pointer is NULL");
  if (update && !(update->lr == update->lr && update->momentum == update->momentum))
    return fail("update: lr / momentum is NaN");
  if (!in_state || !state0 || !loss_partials)
    return fail("in_state / state0 / loss_partials must not be NULL");
  if (int e = simulator.check()) return e;
  const auto step = simulator.step();
  const auto adjoint = simulator.adjoint();
  std::vector<float> G((size_t)cpt_grads(H), 0.f), pre((size_t)H * 4), out((size_t)H);
  // y = tanh(W x + b), one unit at a time
  auto fwd = [](const float *W, const float *b, int N, int K, const float *x, float *y) {
    for (int u = 0; u < N; ++u) {
      float z[1] = {b[u]};
      cpt_dense<1>(
          z, K, [&](int, int j) { return W[u * K + j]; }, [&](int j) { return x[j]; });
      y[u] = tanhf(z[0]);
    }
  };
  // a layer's reverse: its weights' and bias' cotangents from dz [N] and its
  // input x [K]; then (x_is_tanh) the cotangent of the input's pre-activation
  // over x
  auto bwd = [&](const float *W, int N, int K, const float *dz, float *x, int gw, int gb,
                 bool x_is_tanh) {
    float acc[kCptH1];
    for (int j = 0; x_is_tanh && j < K; ++j) {
      float z[1] = {0.f};
      cpt_dense<1>(
          z, N, [&](int, int m) { return W[m * K + j]; }, [&](int m) { return dz[m]; });
      acc[j] = z[0];
    }
    for (int m = 0; m < N; ++m) {
      float once = G[gb + m], again = 0.f;   // (the bias takes dz once per sample)
      for (int j = 0; j < K; ++j) {
        float g1[1] = {G[gw + m * K + j]};
        cpt_wgrad<1>(g1, j == 0 ? once : again, dz[m], [&](int) { return x[j]; });
        G[gw + m * K + j] = g1[0];
      }
      G[gb + m] = once;
    }
    for (int j = 0; x_is_tanh && j < K; ++j) x[j] = cpt_dtanh(acc[j], x[j]);
  };
  LossOut lo{loss_partials, loss};
  auto ST = [&](int k, int i) -> float & { return pre[k * 4 + i]; };
  for (int b = 0; b < B; ++b) {
    float x[kCptIn], h0[kCptH0], h1[kCptH1], h2[kCptH2], h3[kCptH3];
    x[0] = 0.f;                            // Net.forward zeroes column 0
    for (int i = 1; i < kCptIn; ++i) x[i] = in_state[(size_t)b * kCptIn + i];
    fwd(P.w0, P.b0, kCptH0, kCptIn, x, h0);
    fwd(P.w1, P.b1, kCptH1, kCptH0, h0, h1);
    fwd(P.w2, P.b2, kCptH2, kCptH1, h1, h2);
    fwd(P.w3, P.b3, kCptH3, kCptH2, h2, h3);
    fwd(P.w_out, P.b_out, H, kCptH3, h3, out.data());
    for (int k = 0; actions_out && k < H; ++k) actions_out[(size_t)b * H + k] = out[k];
    auto action = [&](int k) { return out[k]; };
    float s0[4], s[4], lam[4];
    for (int i = 0; i < 4; ++i) s0[i] = state0[(size_t)b * 4 + i];
    lo.add(b, B, cart_rollout_forward(H, s0, s, action, ST, step,
                                      [](int, const float (&)[4]) {}));
    cart_rollout_reverse(H, s0, s, lam, action, ST, adjoint,
                         [&](int k, float g) { out[k] = cpt_dtanh(g, out[k]); });
    bwd(P.w_out, H, kCptH3, out.data(), h3, kCptGWout, kCptGWout + kCptH3 * H, true);
    bwd(P.w3, kCptH3, kCptH2, h3, h2, kCptGW3, kCptGB3, true);
    bwd(P.w2, kCptH2, kCptH1, h2, h1, kCptGW2, kCptGB2, true);
    bwd(P.w1, kCptH1, kCptH0, h1, h0, kCptGW1, kCptGB1, true);
    bwd(P.w0, kCptH0, kCptIn, h0, x, kCptGW0, kCptGB0, false);
  }
  lo.finish(B);
  for (int e = 0; e < cpt_grads(H); ++e) {
    int q, off;
    cpt_locate(e, H, q, off);
    tg[q][off] = G[e];
    if (update) cpt_sgd(G[e], update->lr, update->momentum, tp[q][off], tm[q][off]);
  }
  return APG_OK;
}

// what cart_policy_step_host rolls out through: the analytic step on host
// parameters, or LearntCartpoleDynamics on the module's tensors
struct AnalyticCart {
  CartConst c;
  int check() const { return APG_OK; }
  auto step() const {
    return [c = c](float (&v)[4], float a) { cart_step(v, a, c); };
  }
  auto adjoint() const {
    return [c = c](float (&l)[4], const float (&p)[4], float a) {
      return cart_step_adjoint(l, p[1], p[3], cart_step_aux(p, a, c), c);
    };
  }
};

struct LearntCart {
  const ApgCartpoleLearnt *model;
  float dt;
  CartConst c;
  std::vector<float> rows;
  int check() {
    if (const char *e = cart_learnt_check(model, /*need_residual=*/true)) return fail("%s", e);
    CartLearntParams p;
    learnt_setup(*model, dt, p, c, rows);
    return APG_OK;
  }
  auto step() const {
    return [this](float (&v)[4], float a) { cart_learnt_step(v, a, c, rows.data()); };
  }
  auto adjoint() const {
    return [this](float (&l)[4], const float (&p)[4], float a) {
      return cart_learnt_step_adjoint(l, p, a, cart_step_aux(p, a, c), c, rows.data());
    };
  }
};

}  // namespace

extern "C" {

int apg_cartpole_mlp_train_step_cpu(const float *in_state, const float *state0, float dt,
                                    const ApgCartpoleParams *params,
                                    const ApgCartpolePolicy *policy, int B, int H,
                                    float *loss_partials, float *loss,
                                    const ApgCartpolePolicyGrads *grads, float *actions_out,
                                    float *workspace, const ApgCartpoleSgdUpdate *update) {
  (void)workspace;
  return cart_policy_step_host(in_state, state0, params, policy, B, H, loss_partials, loss,
                               grads, actions_out, update,
                               AnalyticCart{params ? make_const(*params, dt) : CartConst{}});
}

int apg_cartpole_learnt_mlp_train_step_cpu(const float *in_state, const float *state0,
                                           float dt, const ApgCartpoleLearnt *model,
                                           const ApgCartpolePolicy *policy, int B, int H,
                                           float *loss_partials, float *loss,
                                           const ApgCartpolePolicyGrads *grads,
                                           float *actions_out, float *workspace,
                                           const ApgCartpoleSgdUpdate *update) {
  (void)workspace;
  return cart_policy_step_host(in_state, state0, model, policy, B, H, loss_partials, loss,
                               grads, actions_out, update, LearntCart{model, dt});
}

}  // extern "C"

// ------------------------------------- rollout through the learnt fixed wing
// apg_cpu_wing_learnt.h: wing_learnt_rollout_kernel (wing_learnt.hip) lane for
// lane - the table and the packed unit rows built as its pack kernel does
extern "C" {

int apg_wing_learnt_rollout_fwd_bwd_cpu(const float *state0, const float *actions,
                                        const float *ref, float dt, const ApgWingLearnt *model,
                                        const ApgWingLossWeights *weights, int B, int H,
                                        int layout, float *loss_partials, float *loss,
                                        float *grad_actions, float *grad_state0,
                                        float *states_out, float *workspace) {
  (void)workspace;
  if (B < 0) return fail("B must be >= 0 (got %d)", B);
  if (layout != APG_LAYOUT_AOS && layout != APG_LAYOUT_SOA)
    return fail("unknown layout %d", layout);
  if (!model || !model->theta || !model->inertia || !model->w1 || !model->b1 || !model->w2 ||
      !model->b2)
    return fail("model or one of its pointers is NULL");
  if (!weights) return fail("weights is NULL");
  if (int e = check_h(H)) return e;
  if (B == 0) {
    if (loss) *loss = 0.f;
    return APG_OK;
  }
  if (!state0 || !actions || !ref || !loss_partials || !grad_actions)
    return fail("state0 / actions / ref / loss_partials / grad_actions must not be NULL");
  const WingGeneralConst k = wing_learnt_table(model->theta, model->inertia, dt);
  std::vector<float> rows(kWingResFloats);
  for (int t = 0; t < kWingResFloats; ++t)
    rows[t] = wing_residual_packed(t, model->w1, model->b1, model->w2, model->b2);
  const float *rw = rows.data();
  const Idx ix{layout, (size_t)B};
  wing_rollout_batch(
      state0, actions, ref, *weights, B, H, ix, LossOut{loss_partials, loss}, grad_actions,
      grad_state0, states_out,
      [&](float (&s)[12], const float (&a)[4]) { wing_learnt_step(s, a, k, rw); },
      [&](float (&lam)[12], float (&ga)[4], const float (&pre)[12], const float (&a)[4]) {
        wing_learnt_step_adjoint(lam, ga, pre, a, k, rw);
      });
  return APG_OK;
}

// apg_cpu_wing_fit.h: fit_host on WingFit (wing_learnt_math.h) - the table and
// the packed unit rows built as the pack kernel does
int apg_wing_learnt_fit_fwd_bwd_cpu(const float *state, const float *action, float dt,
                                    const ApgWingLearnt *model, const float *target,
                                    const ApgWingParams *eval_params, float l2_lambda, int B,
                                    float *loss_partials, float *loss, float *grad,
                                    float *workspace) {
  (void)workspace;
  const bool ok = model && model->theta && model->inertia && model->w1 && model->b1 &&
                  model->w2 && model->b2;
  const WingConst ke = eval_params ? make_const(*eval_params, dt) : WingConst{};
  WingGeneralConst k;
  std::vector<float> rows(kWingResFloats);
  return fit_host<WingFit>(
      ok ? nullptr : "model or one of its pointers is NULL", state, action, target,
      eval_params ? &ke : nullptr, l2_lambda, B, loss_partials, loss, grad, FitNoScale{},
      ok ? ResidualTensors{model->w1, model->b1, model->w2, model->b2} : ResidualTensors{},
      [&] {
        k = wing_learnt_table(model->theta, model->inertia, dt);
        for (int t = 0; t < kWingResFloats; ++t)
          rows[t] = wing_residual_packed(t, model->w1, model->b1, model->w2, model->b2);
        return WingFitModel<const WingGeneralConst, const float *>{&k, rows.data()};
      });
}

// apg_cpu_quad_fit.h: fit_host on QuadFit (quad_fit_math.h) - the model packed
// as the pack kernel does
int apg_quad_learnt_fit_fwd_bwd_cpu(const float *state, const float *action, float dt,
                                    const ApgQuadParams *params,
                                    const ApgLearntResidual *model, const float *target,
                                    const ApgQuadParams *eval_params, float l2_lambda, int B,
                                    float *loss_partials, float *loss, float *grad,
                                    float *workspace) {
  (void)workspace;
  const bool ok = model && model->linear_at && model->w1 && model->b1 && model->w2 && model->b2;
  const QuadConst ce = eval_params ? make_const(*eval_params, dt) : QuadConst{};
  QuadConst c;
  std::vector<float> pack(kQuadPackFloats);
  return fit_host<QuadFit>(
      !params ? "params is NULL" : ok ? nullptr : "model or one of its pointers is NULL", state,
      action, target, eval_params ? &ce : nullptr, l2_lambda, B, loss_partials, loss, grad,
      params ? make_fit_inertia(*params, dt) : QuadFitInertia{},
      ok ? ResidualTensors{model->w1, model->b1, model->w2, model->b2} : ResidualTensors{},
      [&] {
        c = make_const(*params, dt);
        for (int t = 0; t < kQuadPackFloats; ++t) pack[t] = quad_fit_packed(t, *model);
        return QuadFitModel<const float *>{c, pack.data()};
      });
}

}  // extern "C"

// ------------------------------------------------------------ shooting MPC
// apg_cpu_mpc.h: the solver and the flight of quad_mpc_math.h looped over the
// batch, on the analytic model (MpcAnalytic) and on the learnt one (MpcLearnt,
// quad_learnt_mpc_math.h)
namespace {

int check_mpc(const ApgQuadParams *model, const ApgQuadLossWeights *weights,
              const ApgQuadMpcOptions *opt, int B, int H, bool h5) {
  if (B < 0) return fail("B must be >= 0 (got %d)", B);
  if (!model || !weights) return fail("model / weights is NULL");
  if (const char *e = mpc_check_options(opt)) return fail("%s", e);
  if (H != 10 && !(h5 && H == 5))
    return fail(h5 ? "H must be 5 or 10 (got %d)" : "H must be 10 (got %d)", H);
  return APG_OK;
}

template <int H, class Model>
void mpc_solve_batch(const float *state0, const float *ref, int ref_cols, const Model &c,
                     const ApgQuadLossWeights &w, const ApgQuadMpcOptions &o, int B, float *u,
                     float *cost_out, float *cost_trace) {
  const size_t Bs = (size_t)B;
  const int vc = ref_cols == 9 ? 6 : 3;
  for (int b = 0; b < B; ++b) {
    float s0[12], r[H][6], ul[H][4];
    for (int i = 0; i < 12; ++i) s0[i] = state0[i * Bs + b];
    for (int k = 0; k < H; ++k) {
      for (int i = 0; i < 3; ++i) {
        r[k][i] = ref[((size_t)k * ref_cols + i) * Bs + b];
        r[k][3 + i] = ref[((size_t)k * ref_cols + vc + i) * Bs + b];
      }
      for (int j = 0; j < 4; ++j) ul[k][j] = u[((size_t)k * 4 + j) * Bs + b];
    }
    cost_out[b] = mpc_solve<H>(s0, r, ul, c, w, o, [&](int i, float J) {
      if (cost_trace) cost_trace[(size_t)i * Bs + b] = J;
    });
    for (int k = 0; k < H; ++k)
      for (int j = 0; j < 4; ++j) u[((size_t)k * 4 + j) * Bs + b] = ul[k][j];
  }
}

// the block the kernels read, filled as learnt_pack_kernel fills it (`m` as
// learnt_mpc_check_model or quad_flight_check passed it; NULL: no block)
std::vector<float> learnt_pack_host(const ApgLearntResidual *m) {
  std::vector<float> pack(m ? kLearntFloats : 0);
  for (size_t t = 0; t < pack.size(); ++t) pack[t] = learnt_packed((int)t, *m);
  return pack;
}

// the solve behind both twins, after check_mpc, on the model `m`.  objection:
// what the entry point's own model check said (NULL: nothing), raised here in
// its place among the shared checks
template <class Model>
int quad_mpc_solve_twin(const char *objection, const float *state0, const float *ref,
                        int ref_cols, const Model &m, const ApgQuadLossWeights &w,
                        const ApgQuadMpcOptions &o, int B, int H, float *u, float *cost_out,
                        float *cost_trace) {
  if (objection) return fail("%s", objection);
  if (ref_cols != 9 && ref_cols != 6)
    return fail("ref_cols must be 9 ([pos, euler, vel]) or 6 ([pos, vel])");
  if (B == 0) return APG_OK;
  if (!state0 || !ref || !u || !cost_out) return fail("NULL buffer");
  with_horizon(H, [&](auto h) {
    mpc_solve_batch<h()>(state0, ref, ref_cols, m, w, o, B, u, cost_out, cost_trace);
  });
  return APG_OK;
}

// the closed loop behind both twins, after check_mpc: the plant's checks and
// block, then the flights on the model `m`; objection as above
template <class Model>
int quad_mpc_loop_twin(const char *objection, const ApgQuadFlight *flight, float dt,
                       const ApgQuadParams *plant, const ApgLearntResidual *plant_learnt,
                       const Model &m, const ApgQuadLossWeights &w, const ApgQuadMpcOptions &o,
                       int B, float *cost) {
  if (!plant) return fail("plant is NULL");
  if (objection) return fail("%s", objection);
  QuadFlightRule rule;
  if (const char *e = quad_flight_check(flight, plant_learnt, B, &rule)) return fail("%s", e);
  const QuadConst cp = make_const(*plant, dt);
  const std::vector<float> plant_pack = learnt_pack_host(plant_learnt);
  const float *pl = plant_learnt ? plant_pack.data() : nullptr;   // NULL: quad_step alone
  const size_t Bs = (size_t)B;
  for (size_t b = 0; b < Bs; ++b)
    flight->steps[b] = mpc_flight(
        [&](int r, int col) { return flight->traj[((size_t)r * 9 + col) * Bs + b]; },
        [&](float (&s)[12], const float (&u0)[4]) {
          const Trig t = make_trig(&s[3]);
          if (pl) learnt_quad_step_lane(s, u0, cp, t, pl);
          else quad_step(s, u0, cp, t);
        },
        m, w, o, rule,
        MpcFlightLog{flight->div, flight->drone, flight->actions, flight->start_states, cost,
                     Bs, b});
  return APG_OK;
}

}  // namespace

extern "C" {

int apg_quad_mpc_solve_cpu(const float *state0, const float *ref, int ref_cols, float dt,
                           const ApgQuadParams *model, const ApgQuadLossWeights *weights,
                           const ApgQuadMpcOptions *opt, int B, int H, float *u,
                           float *cost_out, float *cost_trace) {
  if (int e = check_mpc(model, weights, opt, B, H, true)) return e;
  const QuadConst c = make_const(*model, dt);
  return quad_mpc_solve_twin(nullptr, state0, ref, ref_cols, MpcAnalytic{c}, *weights, *opt, B,
                             H, u, cost_out, cost_trace);
}

int apg_quad_mpc_closed_loop_cpu(const ApgQuadFlight *flight, float dt,
                                 const ApgQuadParams *plant,
                                 const ApgLearntResidual *plant_learnt,
                                 const ApgQuadParams *model,
                                 const ApgQuadLossWeights *weights,
                                 const ApgQuadMpcOptions *opt, int B, int H, float *cost,
                                 float *workspace) {
  (void)workspace;
  if (int e = check_mpc(model, weights, opt, B, H, false)) return e;
  const QuadConst cm = make_const(*model, dt);
  return quad_mpc_loop_twin(
      plant_learnt ? "the host twin flies the analytic plant only" : nullptr, flight, dt, plant,
      plant_learnt, MpcAnalytic{cm}, *weights, *opt, B, cost);
}

int apg_quad_learnt_mpc_workspace_floats_cpu(void) { return 2 * kLearntFloats; }

int apg_quad_learnt_mpc_solve_cpu(const float *state0, const float *ref, int ref_cols, float dt,
                                  const ApgQuadParams *model,
                                  const ApgLearntResidual *model_learnt,
                                  const ApgQuadLossWeights *weights,
                                  const ApgQuadMpcOptions *opt, int B, int H, float *u,
                                  float *cost_out, float *cost_trace, float *workspace) {
  (void)workspace;
  if (int e = check_mpc(model, weights, opt, B, H, true)) return e;
  const char *objection = learnt_mpc_check_model(model_learnt);
  const std::vector<float> pack = learnt_pack_host(objection ? nullptr : model_learnt);
  const QuadConst c = make_const(*model, dt);
  float pre[10 * kMpcPreRow];
  return quad_mpc_solve_twin(objection, state0, ref, ref_cols,
                             MpcLearnt<const float *>{c, pack.data(), pre}, *weights, *opt, B, H,
                             u, cost_out, cost_trace);
}

int apg_quad_learnt_mpc_closed_loop_cpu(const ApgQuadFlight *flight, float dt,
                                        const ApgQuadParams *plant,
                                        const ApgLearntResidual *plant_learnt,
                                        const ApgQuadParams *model,
                                        const ApgLearntResidual *model_learnt,
                                        const ApgQuadLossWeights *weights,
                                        const ApgQuadMpcOptions *opt, int B, int H,
                                        float *cost, float *workspace) {
  (void)workspace;
  if (int e = check_mpc(model, weights, opt, B, H, false)) return e;
  const char *objection = learnt_mpc_check_model(model_learnt);
  const std::vector<float> pack = learnt_pack_host(objection ? nullptr : model_learnt);
  const QuadConst cm = make_const(*model, dt);
  float pre[kFlightH * kMpcPreRow];
  return quad_mpc_loop_twin(objection, flight, dt, plant, plant_learnt,
                            MpcLearnt<const float *>{cm, pack.data(), pre}, *weights, *opt, B,
                            cost);
}

}  // extern "C"

// ------------------------------------------------- shooting MPC, cart-pole
// apg_cpu_mpc.h: the solver and the flight of cartpole_mpc_math.h looped over
// the batch, on the analytic model (CartMpcAnalytic) and on the learnt one
// (CartMpcLearnt)
namespace {

template <int H, class Model>
void cart_mpc_solve_batch(const float *state0, const float *u0, const Model &c,
                          const ApgCartpoleMpcOptions &o, int B, float *u, float *cost_out,
                          float *cost_trace) {
  const size_t Bs = (size_t)B;
  for (size_t b = 0; b < Bs; ++b) {
    float s0[4], ul[H];
    for (int i = 0; i < 4; ++i) s0[i] = state0[i * Bs + b];
    for (int k = 0; k < H; ++k) ul[k] = u0 ? u0[k * Bs + b] : 0.f;
    const float J = cart_mpc_solve<H>(s0, ul, c, o, [&](int i, float Ji) {
      if (cost_trace) cost_trace[(size_t)i * Bs + b] = Ji;
    });
    if (cost_out) cost_out[b] = J;
    if (u)
      for (int k = 0; k < H; ++k) u[k * Bs + b] = ul[k];
  }
}

template <class Model>
int cart_mpc_solve_twin(const float *state0, const float *u0, const Model &c,
                        const ApgCartpoleMpcOptions &o, int B, int H, float *u,
                        float *cost_out, float *cost_trace) {
  if (B == 0) return APG_OK;
  if (!state0) return fail("state0 is NULL");
  if (H == 5)
    cart_mpc_solve_batch<5>(state0, u0, c, o, B, u, cost_out, cost_trace);
  else
    cart_mpc_solve_batch<10>(state0, u0, c, o, B, u, cost_out, cost_trace);
  return APG_OK;
}

template <int H, class Model>
void cart_mpc_loop_batch(const ApgCartpoleFlight &out, const CartConst &cp, const float *rows,
                         const Model &cm, const ApgCartpoleMpcOptions &o,
                         const CartFlightRule &rule, int B, float *cost) {
  const size_t Bs = (size_t)B;
  for (size_t b = 0; b < Bs; ++b) {
    float s0[4];
    for (int i = 0; i < 4; ++i) s0[i] = out.state0[i * Bs + b];
    const CartFlightBook f = cart_mpc_flight<H>(
        s0, [&](float (&s)[4], float a) { cart_learnt_step(s, a, cp, rows); },
        [](bool alive) { return alive; }, cm, o, rule,
        CartMpcFlightLog{out.states, out.actions, cost, Bs, b}, true);
    out.steps[b] = f.steps, out.upright[b] = f.upright ? 1 : 0;
    out.vel_sum[b] = f.vel_sum, out.vel_sq[b] = f.vel_sq;
  }
}

// the closed loop behind both twins, after the model's own check: the plant's
// checks and setup, then the flights on the model `cm`
template <class Model>
int cart_mpc_loop_twin(const ApgCartpoleFlight *flight, float dt,
                       const ApgCartpoleParams *plant, const ApgCartpoleLearnt *plant_learnt,
                       const Model &cm, const ApgCartpoleMpcOptions &o, int B, int H,
                       float *cost) {
  CartFlightRule rule;
  if (!plant && !plant_learnt) return fail("plant is NULL");
  if (const char *e = cart_mpc_check_learnt(plant_learnt)) return fail("%s", e);
  if (const char *e = cart_flight_check(flight, B, &rule)) return fail("%s", e);
  CartConst cp;
  std::vector<float> rows;
  if (plant_learnt) {
    CartLearntParams p;
    learnt_setup(*plant_learnt, dt, p, cp, rows);
  } else {
    cp = make_const(*plant, dt);
  }
  const float *r = plant_learnt ? rows.data() : nullptr;   // NULL: cart_step alone
  if (H == 5)
    cart_mpc_loop_batch<5>(*flight, cp, r, cm, o, rule, B, cost);
  else
    cart_mpc_loop_batch<10>(*flight, cp, r, cm, o, rule, B, cost);
  return APG_OK;
}

}  // namespace

extern "C" {

int apg_cartpole_mpc_solve_cpu(const float *state0, const float *u0, float dt,
                               const ApgCartpoleParams *model,
                               const ApgCartpoleMpcOptions *opt, int B, int H, float *u,
                               float *cost_out, float *cost_trace) {
  if (B < 0) return fail("B must be >= 0 (got %d)", B);
  if (const char *e = cart_mpc_check(model, opt, H)) return fail("%s", e);
  return cart_mpc_solve_twin(state0, u0, CartMpcAnalytic{make_const(*model, dt)}, *opt, B, H,
                             u, cost_out, cost_trace);
}

int apg_cartpole_mpc_closed_loop_cpu(const ApgCartpoleFlight *flight, float dt,
                                     const ApgCartpoleParams *plant,
                                     const ApgCartpoleLearnt *plant_learnt,
                                     const ApgCartpoleParams *model,
                                     const ApgCartpoleMpcOptions *opt, int B, int H,
                                     float *cost) {
  if (const char *e = cart_mpc_check(model, opt, H)) return fail("%s", e);
  return cart_mpc_loop_twin(flight, dt, plant, plant_learnt,
                            CartMpcAnalytic{make_const(*model, dt)}, *opt, B, H, cost);
}

int apg_cartpole_learnt_mpc_solve_cpu(const float *state0, const float *u0, float dt,
                                      const ApgCartpoleLearnt *model,
                                      const ApgCartpoleMpcOptions *opt, int B, int H, float *u,
                                      float *cost_out, float *cost_trace) {
  if (B < 0) return fail("B must be >= 0 (got %d)", B);
  if (const char *e = cart_mpc_check(model, opt, H)) return fail("%s", e);
  CartLearntParams p;
  CartConst c;
  std::vector<float> rows;
  learnt_setup(*model, dt, p, c, rows);
  return cart_mpc_solve_twin(state0, u0, CartMpcLearnt{c, rows.data()}, *opt, B, H, u,
                             cost_out, cost_trace);
}

int apg_cartpole_learnt_mpc_closed_loop_cpu(const ApgCartpoleFlight *flight, float dt,
                                            const ApgCartpoleParams *plant,
                                            const ApgCartpoleLearnt *plant_learnt,
                                            const ApgCartpoleLearnt *model,
                                            const ApgCartpoleMpcOptions *opt, int B, int H,
                                            float *cost) {
  if (const char *e = cart_mpc_check(model, opt, H)) return fail("%s", e);
  CartLearntParams p;
  CartConst c;
  std::vector<float> rows;
  learnt_setup(*model, dt, p, c, rows);
  return cart_mpc_loop_twin(flight, dt, plant, plant_learnt, CartMpcLearnt{c, rows.data()},
                            *opt, B, H, cost);
}

}  // extern "C"

// ------------------------------------------------ shooting MPC, fixed wing
// apg_cpu_wing_mpc.h: the solver and the flight of wing_mpc_math.h looped over
// the batch; the forward sweep's stash is a local array in place of the LDS
extern "C" {

int apg_wing_mpc_solve_cpu(const float *state0, const float *ref, float dt,
                           const ApgWingParams *model, const ApgWingLossWeights *weights,
                           const ApgWingMpcOptions *opt, int B, int H, float *u,
                           float *cost_out, float *cost_trace) {
  if (const char *e = wing_mpc_check(model, weights, opt, B, H)) return fail("%s", e);
  if (B == 0) return APG_OK;
  if (!state0 || !ref || !u || !cost_out) return fail("NULL buffer");
  constexpr int kH = 10;
  const WingConst c = make_const(*model, dt);
  const size_t Bs = (size_t)B;
  float pre[kH][12];
  for (size_t b = 0; b < Bs; ++b) {
    float s0[12], ul[kH][4];
    for (int i = 0; i < 12; ++i) s0[i] = state0[i * Bs + b];
    for (int k = 0; k < kH; ++k)
      for (int j = 0; j < 4; ++j) ul[k][j] = u[((size_t)k * 4 + j) * Bs + b];
    cost_out[b] = wing_mpc_solve<kH>(
        s0,
        [&](int k, float (&rp)[3]) {
          for (int i = 0; i < 3; ++i) rp[i] = ref[((size_t)k * 3 + i) * Bs + b];
        },
        ul, c, *weights, *opt, [&](int k, int i) -> float & { return pre[k][i]; },
        [&](int i, float J) {
          if (cost_trace) cost_trace[(size_t)i * Bs + b] = J;
        });
    for (int k = 0; k < kH; ++k)
      for (int j = 0; j < 4; ++j) u[((size_t)k * 4 + j) * Bs + b] = ul[k][j];
  }
  return APG_OK;
}

int apg_wing_mpc_closed_loop_cpu(const ApgWingFlight *flight, float dt,
                                 const ApgWingParams *plant, const ApgWingParams *model,
                                 const ApgWingLossWeights *weights,
                                 const ApgWingMpcOptions *opt, int B, int H, float *cost) {
  WingFlightRule rule;
  if (const char *e = wing_mpc_check(model, weights, opt, B, H)) return fail("%s", e);
  if (const char *e = wing_mpc_check_flight(plant, flight, B, &rule)) return fail("%s", e);
  if (B == 0) return APG_OK;
  constexpr int kH = 10;
  const WingConst cp = make_const(*plant, dt), cm = make_const(*model, dt);
  const ApgWingFlight &f = *flight;
  const size_t Bs = (size_t)B;
  float pre[kH][12];
  for (size_t b = 0; b < Bs; ++b)
    f.steps[b] = wing_mpc_flight<kH>(
        f.state0 != nullptr, [&](int i) { return f.state0[i * Bs + b]; },
        [&](int ti, float (&t)[3]) {
          for (int j = 0; j < 3; ++j) t[j] = f.targets[((size_t)ti * 3 + j) * Bs + b];
        },
        [&](float (&s)[12], const float (&a)[4]) { wing_step<true>(s, a, cp); }, cm, *weights,
        *opt, rule,
        WingMpcFlightLog{f.div_linear, f.div_pass, f.div_fail, f.drone, f.seen, cost, Bs, b},
        [&](int k, int i) -> float & { return pre[k][i]; }, [](bool alive) { return alive; },
        true);
  return APG_OK;
}

}  // extern "C"

// ---- the launch chain's bookkeeping (apg_cpu_launch_chain.h) ---------------
extern "C" {

void *apg_cpu_chain_new(void) { return new LaunchChain; }
void apg_cpu_chain_free(void *chain) { delete static_cast<LaunchChain *>(chain); }
int apg_cpu_chain_empty(const void *chain) {
  return static_cast<const LaunchChain *>(chain)->empty();
}

void apg_cpu_chain_launch(void *chain, const float *partials, int count, float *loss,
                          const float *after_partials, int after_count,
                          float *after_loss, ApgCpuChainStep *step) {
  ChainLaunch L{partials, count, loss, {}};
  if (after_loss) L.after = ChainReduce{after_partials, after_count, after_loss};
  const ChainStep s = static_cast<LaunchChain *>(chain)->launch(L);
  step->lane = s.lane, step->fork = s.fork;
  step->pre_lane = s.pre_lane, step->edge_from = s.edge_from;
  step->pre = ApgCpuChainReduce{s.pre.partials, s.pre.count, s.pre.loss};
  step->fold = ApgCpuChainReduce{s.fold.partials, s.fold.count, s.fold.loss};
}

void apg_cpu_chain_flush(void *chain, ApgCpuChainReduce *lane0, int *n0,
                         ApgCpuChainReduce *lane1, int *n1, int cap, int *join) {
  const ChainFlush f = static_cast<LaunchChain *>(chain)->flush();
  ApgCpuChainReduce *out[2] = {lane0, lane1};
  int *n[2] = {n0, n1};
  for (int m = 0; m < 2; ++m) {
    *n[m] = (int)f.reduce[m].size();
    for (int i = 0; i < *n[m] && i < cap; ++i)
      out[m][i] = ApgCpuChainReduce{f.reduce[m][i].partials, f.reduce[m][i].count,
                                    f.reduce[m][i].loss};
  }
  *join = f.join;
}

}  // extern "C"
