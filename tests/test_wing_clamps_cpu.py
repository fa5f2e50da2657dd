"""The fixed-wing arithmetic where its alpha / beta clamps are active, without a
GPU: everything that shares csrc/wing_math.h and csrc/wing_learnt_math.h on the
host - tests/host_math (hm_wing_step, hm_wing_rollout) and the CPU twins of the
step, rollout, learnt-rollout and simulator-fit entry points - on the inputs of
tests/wing_clamp_cases.py: both clamps active, alone and together, switching
along the horizon, within 0.1 % of a bound on either side, u < 0 and u = +-0.

The float64 oracle arbitrates and the float32 oracle is the yardstick
(conftest.assert_no_worse_than_fp32 with its defaults, per trajectory; the 1e-4
bar); no bound of its own.  Every test asserts that its input covers the clamps
and that at most 1 % of it is set aside as too near a kink, and prints what it
measured.

What they catch, tried on a scratch copy of the headers: with beta_free forced
to 1 (the gradient let through an active beta clamp) every step, rollout and
learnt-rollout test here fails, and of the rest of the CPU suite only the
single-step golden tests; the fit tests cannot see that mask - the fit returns
parameter cotangents only, which depend on the clamped angles and not on the
masks - and fail, with all the others, once the beta clamp itself is taken
out of the forward pass.  A reverse sweep that recomputes alpha without its
clamp fails every rollout and learnt-rollout test here."""
import ctypes

import numpy as np
import pytest
import torch

import wing_clamp_cases as wc
from conftest import rel_err
from test_host_math import _f, _p, _wing_params, _wing_step, hw  # noqa: F401
from test_wing_fit_cpu import eval_params, twin_fit
from test_wing_learnt_rollout_cpu import tw, twin_rollout  # noqa: F401

AOS, SOA = 1, 0          # APG_LAYOUT_AOS / APG_LAYOUT_SOA (include/apg.h)


def _F(x):
    return ctypes.c_float(x)


# ---------------------------------------------------------------- references
@pytest.mark.parametrize("tag", ["def", "mod"])
def test_the_two_float64_oracles_agree_on_the_clamp_batch(tag):
    """oracle/apg_oracle_wing.c (branches on the clamp) and torch_port.WingOracle
    (torch.clamp under autograd) take the same branches: the same rollout and
    gradients.  To 1e-7, not to float64's rounding: the port keeps the inertia
    matrix as a float32 tensor, as the reference does (one parameter rounded at
    6e-8), the C restatement reads it in double."""
    from oracle import torch_port as tp
    ref = wc.rollout_reference(258, 13, tag)
    d = ref["d"]
    st, loss, ga, gs = tp.rollout_fwd_bwd(
        tp.WingOracle(wc.PARAMS[tag], dtype=torch.float64), tp.fixed_wing_mpc_loss,
        d["state0"].double(), d["actions"].double(), d["ref"].double(), wc.DT)
    f64 = ref["f64"]
    errs = (rel_err(f64[0], st.numpy()), abs(f64[1] - float(loss)) / float(loss),
            rel_err(f64[2], ga.numpy()), rel_err(f64[3], gs.numpy()))
    print("C oracle vs torch port, float64:", ["%.3g" % e for e in errs])
    assert max(errs) < 1e-7
    # the float32 yardstick too, at float32's own accuracy
    st32 = tp.unroll(tp.WingOracle(wc.PARAMS[tag]), d["state0"], d["actions"], wc.DT)
    assert rel_err(st32.numpy()[ref["keep"]], f64[0][ref["keep"]]) < 1e-5


# ---------------------------------------------------------------------- step
@pytest.mark.parametrize("tag", ["def", "mod"])
def test_host_math_step_and_jacobian(hw, tag):  # noqa: F811
    def run(s, a, cot):
        return _wing_step(hw, s, a, wc.DT, wc.PARAMS[tag], cot=cot)
    wc.check_step(run, tag, f"hm_wing_step/{tag}")


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("tag", ["def", "mod"])
def test_cpu_twin_step_and_jacobian(tw, tag, layout):  # noqa: F811
    par = _wing_params(wc.PARAMS[tag])
    to = (lambda x: _f(x)) if layout == AOS else (lambda x: _f(np.asarray(x).T))
    back = (lambda x: x) if layout == AOS else (lambda x: x.T)

    def run(s, a, cot):
        s, a, cot = to(s), to(a), to(cot)
        B = cot.size // 12
        nxt, gs, ga = np.empty_like(s), np.empty_like(s), np.empty_like(a)
        assert tw.apg_wing_step_fwd_cpu(_p(s), _p(a), _F(wc.DT), ctypes.byref(par), B, layout,
                                        _p(nxt)) == 0
        assert tw.apg_wing_step_bwd_cpu(_p(s), _p(a), _F(wc.DT), ctypes.byref(par), B, layout,
                                        _p(cot), _p(gs), _p(ga)) == 0
        return back(nxt), back(gs), back(ga)
    wc.check_step(run, tag, f"step twin/{tag}/{'aos' if layout == AOS else 'soa'}")


# ------------------------------------------------------------------- rollout
B_ROLL = 2050


@pytest.mark.parametrize("H", [6, 13, 20])
@pytest.mark.parametrize("tag", ["def", "mod"])
def test_host_math_rollout(hw, tag, H):  # noqa: F811
    from apg_trajectory_tracking_amd import functional as F
    ref = wc.rollout_reference(B_ROLL, H, tag)
    d = ref["d"]
    s0, act, r = _f(d["state0"].numpy()), _f(d["actions"].numpy()), _f(d["ref"].numpy())
    st = np.empty((B_ROLL, H, 12), np.float32)
    ga, gs = np.empty_like(act), np.empty_like(s0)
    w = F.wing_loss_weights()
    loss = hw.hm_wing_rollout(_p(s0), _p(act), _p(r), _F(wc.DT),
                              ctypes.byref(_wing_params(wc.PARAMS[tag])), ctypes.byref(w),
                              B_ROLL, H, _p(st), _p(ga), _p(gs))
    wc.check_rollout(dict(states=st, loss=loss, grad_actions=ga, grad_state0=gs), ref,
                     f"hm_wing_rollout/{tag}/H{H}")


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("H", [6, 13, 20])
@pytest.mark.parametrize("tag", ["def", "mod"])
def test_cpu_twin_rollout(tw, tag, H, layout):  # noqa: F811
    from apg_trajectory_tracking_amd import _capi, functional as F
    ref = wc.rollout_reference(B_ROLL, H, tag)
    d = ref["d"]
    B = B_ROLL
    s0, act, r = d["state0"].numpy(), d["actions"].numpy(), d["ref"].numpy()
    if layout == SOA:
        s0, act, r = s0.T, act.transpose(1, 2, 0), r.transpose(1, 2, 0)
    s0, act, r = _f(s0), _f(act), _f(r)
    part = np.empty(_capi.loss_partials_count(B), np.float32)
    loss = np.empty(1, np.float32)
    ga, gs = np.empty_like(act), np.empty_like(s0)
    st = np.empty((B, H, 12) if layout == AOS else (H, 12, B), np.float32)
    par, w = _wing_params(wc.PARAMS[tag]), F.wing_loss_weights()
    assert tw.apg_wing_rollout_fwd_bwd_cpu(
        _p(s0), _p(act), _p(r), _F(wc.DT), ctypes.byref(par), ctypes.byref(w), B, H, layout,
        _p(part), _p(loss), _p(ga), _p(gs), _p(st), None) == 0
    st2 = np.empty_like(st)
    assert tw.apg_wing_rollout_fwd_cpu(_p(s0), _p(act), _F(wc.DT), ctypes.byref(par), B, H,
                                       layout, _p(st2)) == 0
    assert np.array_equal(st2, st)
    if layout == SOA:
        st, ga, gs = st.transpose(2, 0, 1), ga.transpose(2, 0, 1), gs.T
    wc.check_rollout(dict(states=st, loss=loss[0], grad_actions=ga, grad_state0=gs), ref,
                     f"rollout twin/{tag}/H{H}/{'aos' if layout == AOS else 'soa'}")


# ------------------------------------------------------------ learnt rollout
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("H", [10, 20])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_learnt_rollout_twin(tw, which, H, layout):  # noqa: F811
    B = 258
    ref = wc.learnt_rollout_reference(which, B, H)
    d = ref["d"]
    res = twin_rollout(tw, wc.learnt_weights(which), d["state0"], d["actions"], d["ref"],
                       layout=layout)
    wc.check_learnt_rollout(dict(res, loss=res["loss"][0]), ref,
                            f"learnt rollout twin/{which}/H{H}/{layout}")


# ----------------------------------------------------------------------- fit
@pytest.mark.parametrize("mode", ["params", "target"])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_fit_twin(tw, which, mode):  # noqa: F811
    ref = wc.fit_reference(which)
    kw = dict(params=eval_params()) if mode == "params" else dict(target=ref["target32"])
    res = twin_fit(tw, wc.learnt_weights(which), ref["state"], ref["action"], wc.DT, **kw)
    wc.check_fit(res, ref, mode, f"fit twin/{which}/{mode}")
