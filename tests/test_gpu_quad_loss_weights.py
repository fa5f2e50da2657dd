"""Every quadrotor kernel that reads ApgQuadLossWeights under NON-default
weights (tests/quad_loss_cases.py: the five one-hot sets and `balanced`),
against the float64 oracle with the weighted loss written out in plain torch.

Everywhere else the suite passes the defaults, where av = rates = 0.1 (a kernel
that reads one for the other is bit-identical) and the av / rates / thrust
terms are below the bars.  tests/test_quad_loss_cases_cpu.py holds the
conditions that let these tests see such a fault: under `balanced` every term
is 10-40 % of the loss, and exchanging av and rates moves the float64 loss and
every compared gradient by >= 100 x the bar applied here.

Bars: loss and every wave's partial within 1e-5 of float64, dL/dactions and
dL/dstate0 within 1e-4 per trajectory (conftest.per_trajectory_err); where the
float64 quantity is identically zero (dL/dstate0 under the one-hot rates and
thrust sets) the device tensor must be exactly zero."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import quad_loss_cases as C
from conftest import rel_err

pytestmark = pytest.mark.gpu
LOSS_BAR, GRAD_BAR = 1e-5, 1e-4
SETS = list(C.NAMES) + ["balanced"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def N(t):
    return t.detach().double().cpu().numpy()


def to_layout(layout, s0, a, ref, dev):
    from apg_trajectory_tracking_amd import synthetic as sy
    if layout == "soa":
        out = (sy.to_soa_state(s0), sy.to_soa_seq(a), sy.to_soa_seq(ref))
    elif layout == "packed":
        out = (sy.to_packed_state(s0), sy.to_packed_seq(a), sy.to_packed_seq(ref))
    else:
        out = (s0, a, ref)
    return tuple(t.to(dev) for t in out)


def from_layout(layout, res):
    """grad_actions [B,H,4], grad_state0 [B,12] as float64 numpy."""
    from apg_trajectory_tracking_amd import synthetic as sy
    ga, gs = res["grad_actions"], res["grad_state0"]
    if layout == "soa":
        ga, gs = sy.from_soa_seq(ga), sy.from_soa_state(gs)
    elif layout == "packed":
        ga, gs = sy.from_packed_seq(ga), sy.from_packed_state(gs)
    return N(ga), N(gs)


def check_rollout(layout, res, want, tag, keep=None):
    """loss, partials, dL/dactions, dL/dstate0 of a fused rollout against the
    float64 dict of quad_loss_cases.oracle_rollout; `keep`: the trajectories
    whose gradients are compared (the learnt cases' kink rule)."""
    ga, gs = from_layout(layout, res)
    keep = slice(None) if keep is None else keep
    loss, parts = float(res["loss"]), N(res["loss_partials"])
    e = dict(loss=abs(loss - want["loss"]) / want["loss"],
             partials=float((np.abs(parts - want["partials"]) / want["partials"]).max()),
             grad_actions=float(C.traj_err(ga[keep], want["grad_actions"][keep]).max()),
             grad_state0=float(C.traj_err(gs[keep], want["grad_state0"][keep]).max()))
    print(tag, {k: float("%.3g" % v) for k, v in e.items()})
    assert parts.shape == want["partials"].shape, tag
    assert e["loss"] < LOSS_BAR and e["partials"] < LOSS_BAR, (tag, e)
    assert e["grad_actions"] < GRAD_BAR and e["grad_state0"] < GRAD_BAR, (tag, e)


def same_bits(a, b, keys=("loss", "loss_partials", "grad_actions", "grad_state0")):
    return all(torch.equal(a[k], b[k]) for k in keys)


# slab (aos) / register (soa) / rows (packed) kernels at H = 5, 10; the LDS
# kernel at every other horizon - here for the first time with packed [pos, vel]
# reference rows
ROWS = ([(lay, H, rc) for lay in ("aos", "soa") for H in (5, 10, 7, 23) for rc in (9, 6)]
        + [("packed", H, 6) for H in (5, 10)])
# B = 200 everywhere; the ragged second wave (B = 67) at H = 10
CASES = [r + (200,) for r in ROWS] + [r + (67,) for r in ROWS if r[1] == 10]


@pytest.mark.parametrize("layout,H,ref_cols,B", CASES)
def test_rollout_kernels_under_the_weight_sets(dev, layout, H, ref_cols, B):
    """Each row with want_states on and off (bit-identical loss and gradients)."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    s0, a, ref = C.rollout_batch(B, H)
    dyn = FlightmareDynamics(modified_params=dict(C.MOD))
    args = to_layout(layout, s0, a, C.packed_ref(ref) if ref_cols == 6 else ref, dev)
    for name in SETS:
        w = C.weight_sets(C.rollout_key(B, H))[name]
        want = C.rollout_oracle(B, H, w)
        full = F.quad_rollout_fwd_bwd(*args, C.ROLLOUT_DT, dyn.params, C.capi_weights(w),
                                      layout=layout, want_states=True)
        lean = F.quad_rollout_fwd_bwd(*args, C.ROLLOUT_DT, dyn.params, C.capi_weights(w),
                                      layout=layout, want_states=False)
        tag = f"{layout}/H{H}/ref{ref_cols}/B{B}/{name}"
        check_rollout(layout, full, want, tag)
        assert lean["states"] is None and same_bits(lean, full), tag


# ------------------------------------------- the loss kernel on given states
def loss_kernel(states, ref, actions, w, layout):
    """apg_quad_loss_fwd_bwd on [B,H,*] float32 device tensors in either layout
    -> loss, partials, dL/dstates [B,H,12], dL/dactions [B,H,4] (float64 numpy)."""
    from apg_trajectory_tracking_amd import _capi, synthetic as sy
    B, H, _ = states.shape
    soa = layout == "soa"
    s, r, a = ((sy.to_soa_seq(t) if soa else t.contiguous()) for t in (states, ref, actions))
    parts = torch.empty(_capi.loss_partials_count(B), device=s.device)
    loss = torch.empty(1, device=s.device)
    gs, ga = torch.empty_like(s), torch.empty_like(a)
    _capi.check(_capi.lib().apg_quad_loss_fwd_bwd(
        _capi.ptr(s), _capi.ptr(r), ref.shape[2], _capi.ptr(a),
        ctypes.byref(C.capi_weights(w)), B, H,
        _capi.LAYOUT_SOA if soa else _capi.LAYOUT_AOS, _capi.ptr(parts), _capi.ptr(loss),
        _capi.ptr(gs), _capi.ptr(ga), _capi.stream_of(s)), "apg_quad_loss_fwd_bwd")
    if soa:
        gs, ga = sy.from_soa_seq(gs), sy.from_soa_seq(ga)
    return float(loss), N(parts), N(gs), N(ga)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("B,H,ref_cols", [(200, 7, 9), (200, 7, 6), (67, 10, 9)])
def test_loss_kernel_under_the_weight_sets(dev, B, H, ref_cols, layout):
    """F.quad_loss / apg_quad_loss_fwd_bwd on materialised float32 states (the
    float64 oracle's, rounded): loss, partials, dL/dstates, dL/dactions against
    the weighted loss in float64 on the same float32 numbers."""
    from apg_trajectory_tracking_amd import functional as F
    s0, a, ref = C.rollout_batch(B, H)
    if ref_cols == 6:
        ref = C.packed_ref(ref)
    states = torch.from_numpy(C.rollout_oracle(B, H, C.DEFAULT)["states"]).float()
    ds, dr, da = states.to(dev), ref.to(dev), a.to(dev)
    for name in SETS:
        w = C.weight_sets(C.rollout_key(B, H))[name]
        fn = C.weighted_quad_mpc_loss(w)
        s64 = states.double().requires_grad_(True)
        a64 = a.double().requires_grad_(True)
        want = fn(s64, ref.double(), a64)
        want.backward()
        want = float(want.detach())
        wparts = C.wave_sums(fn.per_trajectory(s64.detach(), ref.double(), a64.detach()))
        loss, parts, gs, ga = loss_kernel(ds, dr, da, w, layout)
        e = dict(loss=abs(loss - want) / want,
                 partials=float((np.abs(parts - wparts) / wparts).max()),
                 grad_states=float(C.traj_err(gs, s64.grad.numpy()).max()),
                 grad_actions=float(C.traj_err(ga, a64.grad.numpy()).max()))
        tag = f"loss kernel {layout}/B{B}/H{H}/ref{ref_cols}/{name}"
        print(tag, {k: float("%.3g" % v) for k, v in e.items()})
        assert e["loss"] < LOSS_BAR and e["partials"] < LOSS_BAR, (tag, e)
        assert e["grad_states"] < GRAD_BAR and e["grad_actions"] < GRAD_BAR, (tag, e)
        if layout == "aos":         # the autograd entry point on the same kernel
            ts, ta = ds.clone().requires_grad_(True), da.clone().requires_grad_(True)
            out = F.quad_loss(ts, dr, ta, C.capi_weights(w))
            out.backward()
            assert float(out.detach()) == loss
            assert np.array_equal(N(ts.grad), gs) and np.array_equal(N(ta.grad), ga)


# ------------------------------------- the rollout through the learnt simulator
@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_learnt_rollout_under_the_weight_sets(dev, layout):
    """quad_learnt_rollout_kernel (golden weights, H = 10) under `balanced` and
    the one-hot av and rates sets against LearntQuadOracle in float64."""
    from apg_trajectory_tracking_amd import functional as F
    B, H = 200, 10
    dyn = C.learnt_module("golden", dev)
    args = to_layout(layout, *C.learnt_batch(B, H), dev)
    for name in ("balanced", "av", "rates"):
        w = C.weight_sets(C.learnt_key("golden", H))[name]
        want = C.learnt_oracle("golden", B, H, w)
        res = F.quad_learnt_rollout_fwd_bwd(dyn, *args, C.learnt_dt(), C.capi_weights(w),
                                            layout=layout)
        check_rollout(layout, res, want, f"learnt {layout}/{name}", keep=~want["kink"])


# ------------------------------------------------------- the policy kernels
def _policy_on_device(kind, dev):
    net, d, hc = C.policy_case(kind)
    gnet = copy.deepcopy(net).to(dev)
    s0, in_ref, ref = (d[k].to(dev) for k in ("state0", "in_ref", "ref"))
    return gnet, s0, in_ref, ref, hc


@pytest.mark.parametrize("kind", C.POLICY_KINDS)
def test_policy_kernels_under_balanced_weights(dev, kind):
    """quad_concurrent_policy_grads / quad_mlp_rollout_grads /
    quad_lstm_rollout_grads: loss within 1e-5 and every parameter gradient
    within 1e-4 (conftest.rel_err) of float64 autograd with the weighted loss -
    the bounds of tests/test_gpu_in_sweep.py and test_gpu_in_sweep_recurrent.py,
    on their smallest batch.  One-hot sets are not run here: they would move the
    cotangents out of the documented operand range."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dataset import state_preprocessing
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    w = C.balanced(C.policy_key(kind))
    want = C.policy_oracle(kind, w)
    gnet, s0, in_ref, ref, hc = _policy_on_device(kind, dev)
    par, cw = FlightmareDynamics().params, C.capi_weights(w)
    if kind == "concurrent":
        with torch.no_grad():
            normed = state_preprocessing(s0)
        loss, grads, _ = F.quad_concurrent_policy_grads(gnet, normed, s0, in_ref, ref,
                                                        C.POLICY_DT, par, weights=cw)
    elif kind == "recurrent":
        loss, grads, _ = F.quad_mlp_rollout_grads(gnet, s0, in_ref, ref, C.POLICY_DT, par,
                                                  weights=cw)
    else:
        loss, grads, _ = F.quad_lstm_rollout_grads(gnet, s0, in_ref, ref, C.POLICY_DT, par,
                                                   hc[0].to(dev), hc[1].to(dev), weights=cw)
    e_loss = abs(loss.item() - want["loss"]) / abs(want["loss"])
    errs = {k: rel_err(N(grads[k]).reshape(g.shape), g) for k, g in want["grads"].items()}
    print(f"policy {kind}: loss", float("%.3g" % e_loss),
          {k: float("%.3g" % v) for k, v in errs.items()})
    assert set(grads) == set(want["grads"])
    assert e_loss < 1e-5
    assert max(errs.values()) < 1e-4, errs


# --------------------------------------------------------- the shooting MPC
def test_mpc_solve_under_balanced_weights(dev):
    """apg_quad_mpc_solve against the restatement with the same weights, under
    the arbiter of tests/test_gpu_quad_mpc.py (check_solve)."""
    import quad_mpc_restatement as R
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    from test_quad_mpc_cpu import check_solve
    w = C.balanced("mpc")
    s0, ref, u0 = C.mpc_inputs()
    got = F.quad_mpc_solve(s0.to(dev), ref.to(dev), C.MPC_DT, FlightmareDynamics().params,
                           u0=u0.to(dev), weights=C.capi_weights(w), iters=C.MPC_ITERS,
                           want_trace=True)
    check_solve(got, C.mpc_restated(w, torch.float32), C.mpc_restated(w), "kernel balanced")
