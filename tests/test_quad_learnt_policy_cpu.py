"""The concurrent controller step through the learnt quadrotor simulator
(apg_quad_learnt_mlp_concurrent_train_step), what holds without a GPU:

  * the conditions of tests/quad_learnt_policy_cases.py on the float64 oracle
    alone - few trajectories sit on a ReLU kink, the float32 oracle is within a
    tenth of the GPU bars, and leaving out the residual or the action transform
    moves EVERY parameter gradient by more than a hundred times the bar (a
    missing or transposed residual adjoint cannot hide under the tolerance);
  * the entry's argument errors, reported before any device work;
  * the layout of the flat gradient buffer;
  * TrainDrone's choice between the fused step and the tape;
  * the forward kernel's registers as the compiler reports them.

Measured here (pytest -s prints them): kink share 0.005 / 0.010 / 0.017; float32
oracle loss <= 4.6e-7, gradients <= 1.4e-6; without the residual >= 0.035;
without the linear_at perturbation >= 0.14."""
import ctypes
import json

import numpy as np
import pytest
import torch

import quad_learnt_policy_cases as pc
from conftest import rel_err


# ------------------------------------------------------------ case conditions
@pytest.mark.parametrize("which", pc.SIMS)
def test_few_pool_rows_sit_on_a_kink(which):
    share = float(pc.pool_kinks(which).mean())
    print(which, "kink share", round(share, 4))
    assert share <= pc.MAX_KINK_SHARE
    # ... and every batch size finds its rows
    assert len(pc.batch_rows(which, max(pc.SIZES))) == max(pc.SIZES)


@pytest.mark.parametrize("which", pc.SIMS)
def test_float32_oracle_is_within_a_tenth_of_the_gpu_bars(which):
    for B in pc.SIZES:
        o64, o32 = pc.oracle(which, B), pc.oracle(which, B, torch.float32)
        e_loss = abs(o32["loss"] - o64["loss"]) / abs(o64["loss"])
        e = pc.moved(o32["grads"], o64["grads"])
        print(which, B, "loss", "%.2g" % e_loss, "grads", "%.2g" % max(e.values()))
        assert e_loss <= 0.1 * pc.LOSS_BAR, (which, B, e_loss)
        assert max(e.values()) <= 0.1 * pc.GRAD_BAR, (which, B, e)


@pytest.mark.parametrize("which", pc.SIMS)
@pytest.mark.parametrize("left_out", ["residual", "transform"])
def test_residual_and_transform_move_every_gradient(which, left_out):
    for B in pc.SIZES:
        full = pc.oracle(which, B)
        less = pc.oracle(which, B, **{left_out: False})
        e = pc.moved(less["grads"], full["grads"])
        print(which, B, "without the", left_out, "%.3g" % min(e.values()))
        assert set(e) == set(_names()) and min(e.values()) >= pc.MIN_MOVE, (which, B, e)


def _names():
    from apg_trajectory_tracking_amd import functional as F
    return F._MLP_PARAMS


# -------------------------------------------------------------- the C entry
def _call(lib, **kw):
    """The entry with host buffers of the right sizes (nothing may be touched:
    every case here is refused before any device work)."""
    from apg_trajectory_tracking_amd import _capi, functional as F
    B = kw.pop("B", 4)
    keep = []

    def buf(n, dtype=np.float32):
        a = np.zeros(max(int(n), 1), dtype)
        keep.append(a)
        return a.ctypes.data
    sizes = [int(np.prod(s)) for s in F._QUAD_POLICY_SHAPES.values()]
    struct = lambda cls, drop=(): cls(*[None if i in drop else buf(n)
                                        for i, n in enumerate(sizes)])
    learnt = _capi.ApgLearntResidual(buf(16), buf(1024), buf(64), buf(768), buf(12))
    for name in kw.pop("learnt_without", ()):
        setattr(learnt, name, None)
    upd = None
    if "update" in kw:
        u = kw.pop("update")
        upd = _capi.ApgMlpSgdUpdate(
            lr=0.1, momentum=0.9, param=struct(_capi.ApgMlpPolicyGrads, u.get("drop", ())),
            momentum_buf=struct(_capi.ApgMlpPolicyGrads), resident=u.get("resident", 0))
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import FlightmareDynamics
    a = dict(
        state0=buf(12 * B), ref=buf(10 * 9 * B), ref_cols=9, dt=0.1,
        params=ctypes.byref(FlightmareDynamics().params), learnt=ctypes.byref(learnt),
        weights=ctypes.byref(F.quad_loss_weights()),
        policy=ctypes.byref(struct(_capi.ApgMlpPolicy)), B=B, H=10, acts=buf(521 * B),
        relu_mask=buf(5 * B, np.uint32), d_zout=buf(40 * B), loss_partials=buf(64),
        loss=buf(1), grads=ctypes.byref(struct(_capi.ApgMlpPolicyGrads, kw.pop("grads_drop", ()))),
        states=None, workspace=buf(16), partials=buf(16),
        update=ctypes.byref(upd) if upd is not None else None, stream=None)
    a.update(kw)
    return lib.apg_quad_learnt_mlp_concurrent_train_step(*a.values())


def test_argument_errors_before_anything_runs():
    from apg_trajectory_tracking_amd import _capi
    lib = _capi.lib()
    msg = lib.apg_last_error_string
    assert _call(lib, learnt=None) == -1 and b"learnt is NULL" in msg()
    for name in ("w1", "b1", "w2", "b2"):
        assert _call(lib, learnt_without=(name,)) == -1 and b"w1 / b1 / w2 / b2" in msg(), name
    assert _call(lib, H=9) == -1 and b"horizon 10" in msg()
    assert _call(lib, H=20) == -1 and b"horizon 10" in msg()
    for cols in (3, 7, 12):
        assert _call(lib, ref_cols=cols) == -1 and b"ref_cols must be 9 or 6" in msg()
    assert _call(lib, grads=None) == -1 and b"gradient pointer" in msg()
    assert _call(lib, grads_drop=(4,)) == -1 and b"gradient pointer" in msg()
    assert _call(lib, update=dict(drop=(7,))) == -1 and b"update" in msg()
    for resident in (1, 2, 3, -1):
        assert _call(lib, update=dict(resident=resident)) == -1 and b"resident must be 0" in msg()
    assert _call(lib, B=0, update={}) == -1 and b"B = 0" in msg()
    assert _call(lib, B=-1) == -1 and b"B must be" in msg()


def test_workspace_holds_the_analytic_steps_and_the_packed_simulator():
    from apg_trajectory_tracking_amd import _capi
    lib = _capi.lib()
    # [W1 64 x 16 | b1 64 | W2^T 64 x 12 | b2 12 | linear_at 16], padded to whole 64s
    packed = -(-(1024 + 64 + 768 + 12 + 16) // 64) * 64
    assert (lib.apg_quad_learnt_mlp_step_workspace_floats()
            == lib.apg_quad_mlp_step_workspace_floats() + packed)


# ---------------------------------------------------------------- Python side
def test_flat_gradient_layout():
    """One buffer, the gradients as contiguous views in _MLP_PARAMS order (what
    the policy's own parameters are, in order), one free slot behind them."""
    from apg_trajectory_tracking_amd import functional as F
    net = pc.policy()
    # (the parameters that take part in the forward pass: the oracle's gradients)
    used = tuple(pc.oracle("golden", 1)["grads"])
    assert tuple(F._QUAD_POLICY_SHAPES) == F._MLP_PARAMS == used
    flat, views = F._flat_grads(torch.device("cpu"), F._QUAD_POLICY_SHAPES)
    at = 0
    named = dict(net.named_parameters())
    for name in used:
        p, v = named[name], views[name]
        assert v.shape == p.shape and v.is_contiguous()
        assert v.data_ptr() == flat.data_ptr() + 4 * at, name
        at += p.numel()
    assert flat.numel() == at + 1


def test_functional_refuses_what_the_step_does_not_serve():
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.models.hutter_model import Net
    net, dyn = pc.policy(), pc.module(pc.sim_weights("golden"), "cpu")
    # (stock shapes, but not on a CUDA device)
    assert F.quad_learnt_fusable(dyn) and not F.quad_learnt_policy_fusable(net, dyn)
    assert not F.quad_learnt_policy_fusable(Net(15, 10, 9, 4, conv=1), dyn)
    assert not F.quad_learnt_policy_fusable(net, object())
    _, b = pc.batch("golden", 4)
    with pytest.raises(ValueError, match="fused learnt-simulator step needs"):
        F.quad_learnt_concurrent_policy_grads(net, dyn, b["normed"], b["state0"], b["in_ref"],
                                              b["ref"], 0.1)


def _trainer(flag, monkeypatch, fusable=True):
    from apg_trajectory_tracking_amd import train_drone
    calls = []

    def step(net, dyn, normed, state0, in_ref, ref, dt, weights=None, index=None,
             update=None, out=None):
        calls.append(dict(index=index, update=update, dt=dt, dyn=dyn))
        flat, views = train_drone.F._flat_grads(torch.device("cpu"),
                                                train_drone.F._QUAD_POLICY_SHAPES)
        flat.zero_()
        return torch.tensor(3.5), views, flat
    monkeypatch.setattr(train_drone.F, "quad_learnt_concurrent_policy_grads", step)
    monkeypatch.setattr(train_drone.F, "quad_learnt_policy_fusable", lambda n, d: fusable)
    dyn = pc.module(pc.sim_weights("golden"), "cpu")
    t = train_drone.TrainDrone(dyn, None, dict(delta_t=0.1, horizon=10, train_mode="concurrent"))
    t.net = pc.policy()
    t.optimizer_controller = torch.optim.SGD(t.net.parameters(), lr=0.0, momentum=0.9)
    t.fused_learnt_policy = flag
    return t, calls


def test_the_trainer_keeps_the_tape_unless_told_otherwise(monkeypatch):
    from apg_trajectory_tracking_amd import train_drone
    assert train_drone.TrainDrone.fused_learnt_policy is False
    _, b = pc.batch("golden", 4)
    args = (b["normed"], b["state0"], b["in_ref"], b["ref"])
    t, calls = _trainer(False, monkeypatch)
    assert t.train_concurrent_fused(*args) is None and not calls
    assert t.train_concurrent_fused(None, None, None, None, probe=True) is False

    t, calls = _trainer(True, monkeypatch)
    loss = t.train_concurrent_fused(*args)
    assert float(loss) == 3.5 and len(calls) == 1
    assert calls[0]["index"] is None and calls[0]["dyn"] is t.train_dynamics
    assert calls[0]["update"] is None          # (host parameters: optimizer.step() follows)
    named = dict(t.net.named_parameters())
    assert all(named[n].grad is not None for n in _names())
    index = torch.tensor([2, 0])
    assert float(t.train_concurrent_fused(*args, index=index)) == 3.5 and len(calls) == 2
    assert calls[1]["index"] is index
    # the loops that ask first keep getting "no" for a learnt simulator
    assert t.train_concurrent_fused(None, None, None, None, probe=True) is False
    assert len(calls) == 2

    # whatever else must hold: the policy switch, the pair, the mode, the horizon
    for spoil in ("fused_policy", "pair", "mode", "horizon"):
        t, calls = _trainer(True, monkeypatch, fusable=spoil != "pair")
        if spoil == "fused_policy":
            t.fused_policy = False
        elif spoil == "mode":
            t.train_mode = "autoregressive"
        elif spoil == "horizon":
            t.horizon = 5
        assert t.train_concurrent_fused(*args) is None and not calls, spoil


# ------------------------------------------------------------------- resources
def test_the_forward_kernel_has_no_scratch_and_two_waves_per_simd():
    from apg_trajectory_tracking_amd import build
    build.build()
    with open(build.RESOURCES) as f:
        res = json.load(f)
    hits = {k: v for k, v in res.items() if "mlp_concurrent_learnt_fwd_kernel" in k}
    assert len(hits) == 1, list(hits)
    (v,) = hits.values()
    print(v)
    assert v["scratch"] == 0 and v["vgpr_spill"] == 0, v
    assert v["occupancy"] >= 2 and v["vgprs"] <= 256, v
