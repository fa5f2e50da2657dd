"""The concurrent controller step through the learnt fixed-wing simulator
(apg_wing_learnt_mlp_train_step), what holds without a GPU:

  * the conditions of tests/wing_learnt_policy_cases.py on the float64 oracle
    alone - few trajectories sit on a ReLU kink, the float32 oracle is within a
    tenth of the GPU bars, and a missing residual, a residual adjoint that is
    blind to the action, or a sparse inertia matrix each move EVERY parameter
    gradient by about fifty times the bar or more (they cannot hide under the
    tolerance);
  * the entry's argument errors, reported before any device work;
  * the published offsets of the flat gradient buffer;
  * TrainFixedWing's choice between the fused step and today's paths;
  * the forward kernel's registers as the compiler reports them.

Measured here (pytest -s prints them): kink share 0.0067 (w) / 0.005 (steps);
float32 oracle loss <= 3e-7, gradients <= 7.9e-7; without the residual >= 0.80;
with an action-blind residual >= 0.088; with the sparse inertia on `steps`
0.0112 / 0.00967 / 0.0109 / 0.0112 at B = 1 / 33 / 257 / 515 (the thin one: its
threshold is half the smallest, see the test)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import wing_learnt_policy_cases as pc


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
@pytest.mark.parametrize("variant", ["no_residual", "action_blind"])
def test_the_residual_and_its_action_columns_move_every_gradient(which, variant):
    for B in pc.SIZES:
        full, less = pc.oracle(which, B), pc.oracle(which, B, variant=variant)
        e = pc.moved(less["grads"], full["grads"])
        print(which, B, variant, "%.3g" % min(e.values()))
        assert set(e) == set(pc.NAMES) and min(e.values()) >= pc.MIN_MOVE, (which, B, e)


def test_the_full_inertia_matrix_moves_every_gradient():
    """On `steps` only: `w`'s inertia already has the sparse form.  The smallest
    shift of a gradient, measured on the float64 oracle: 0.0112 (B = 1), 0.00967
    (B = 33), 0.0109 (B = 257), 0.0112 (B = 515).  B = 33 falls just below
    MIN_MOVE = 1e-2, so this one threshold is half the smallest value measured,
    4.8e-3: still 48 times the gradient bar, which is the point of the check."""
    bar = 0.5 * 0.00967
    for B in pc.SIZES:
        full, less = pc.oracle("steps", B), pc.oracle("steps", B, variant="sparse_inertia")
        e = pc.moved(less["grads"], full["grads"])
        print("steps", B, "sparse inertia", "%.3g" % min(e.values()))
        assert set(e) == set(pc.NAMES) and min(e.values()) >= bar, (B, e)


# -------------------------------------------------------------- the C entry
def _shapes():
    from apg_trajectory_tracking_amd import functional as F
    return F._WING_POLICY_SHAPES


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
    sizes = [int(np.prod(s)) for s in _shapes().values()]
    struct = lambda cls, drop=(): cls(*[None if i in drop else buf(n)
                                        for i, n in enumerate(sizes)])
    model = _capi.ApgWingLearnt(buf(41), buf(9), buf(1024), buf(64), buf(768), buf(12))
    for name in kw.pop("model_without", ()):
        setattr(model, name, None)
    upd = None
    if "update" in kw:
        u = kw.pop("update")
        upd = _capi.ApgWingSgdUpdate(
            lr=u.get("lr", 0.1), momentum=u.get("momentum", 0.9),
            param=struct(_capi.ApgWingPolicyGrads, u.get("drop", ())),
            momentum_buf=struct(_capi.ApgWingPolicyGrads, u.get("drop_buf", ())))
    a = dict(
        feat=buf(9 * B), ref_in=buf(3 * B), state0=buf(12 * B), ref=buf(30 * B), dt=0.05,
        model=ctypes.byref(model), weights=ctypes.byref(F.wing_loss_weights()),
        policy=ctypes.byref(struct(_capi.ApgWingPolicy, kw.pop("policy_drop", ()))), B=B, H=10,
        acts=buf(412 * B), cot=buf(360 * B), loss_partials=buf(64), loss=buf(1),
        grads=ctypes.byref(struct(_capi.ApgWingPolicyGrads, kw.pop("grads_drop", ()))),
        states=None, workspace=buf(16),
        update=ctypes.byref(upd) if upd is not None else None, stream=None)
    a.update(kw)
    return lib.apg_wing_learnt_mlp_train_step(*a.values())


def test_argument_errors_before_anything_runs():
    from apg_trajectory_tracking_amd import _capi
    lib = _capi.lib()
    msg = lib.apg_last_error_string
    assert _call(lib, model=None) == -1 and b"model" in msg()
    for name in ("theta", "inertia", "w1", "b1", "w2", "b2"):
        assert _call(lib, model_without=(name,)) == -1 and b"model" in msg(), name
    assert _call(lib, policy=None) == -1 and b"policy is NULL" in msg()
    assert _call(lib, policy_drop=(10,)) == -1 and b"policy weight pointer" in msg()
    for H in (9, 20, 0):
        assert _call(lib, H=H) == -1 and b"horizon 10" in msg(), H
    assert _call(lib, B=-1) == -1 and b"B must be" in msg()
    assert _call(lib, weights=None) == -1 and b"weights is NULL" in msg()
    assert _call(lib, grads=None) == -1 and b"gradient pointer" in msg()
    assert _call(lib, grads_drop=(4,)) == -1 and b"gradient pointer" in msg()
    assert _call(lib, update=dict(drop=(7,))) == -1 and b"update" in msg()
    assert _call(lib, update=dict(drop_buf=(0,))) == -1 and b"update" in msg()
    for bad in (dict(lr=-1e-3), dict(lr=float("nan")), dict(lr=float("inf")),
                dict(momentum=-0.5), dict(momentum=float("nan"))):
        assert _call(lib, update=bad) == -1 and b"finite and >= 0" in msg(), bad
    assert _call(lib, B=0, update={}) == -1 and b"B = 0" in msg()


def test_published_offsets_are_the_flat_gradient_layout():
    """One buffer, the gradients as contiguous views in _WING_PARAMS order (what
    the policy's own parameters are, in order), one free slot behind them, each
    starting where include/apg.h's APG_WING_POLICY_G_* says."""
    import os
    import re
    from apg_trajectory_tracking_amd import _capi, functional as F
    net = pc.policy()
    used = tuple(pc.oracle("w", 1)["grads"])
    assert tuple(_shapes()) == F._WING_PARAMS == used == pc.NAMES
    # (the parameters that take part in the forward pass, in the module's order)
    assert tuple(n for n, _ in net.named_parameters() if n in used) == used
    flat, views = F._flat_grads(torch.device("cpu"), _shapes())
    named = dict(net.named_parameters())
    at = []
    for name in used:
        p, v = named[name], views[name]
        assert v.shape == p.shape and v.is_contiguous()
        at.append((v.data_ptr() - flat.data_ptr()) // 4)
    assert tuple(at) == _capi.WING_POLICY_G
    assert flat.numel() == _capi.WING_POLICY_GRADS + 1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "apg.h")).read()
    macros = dict(re.findall(r"#define APG_WING_POLICY_(G_\w+|GRADS) (\d+)", header))
    fields = [f for f, _ in _capi.ApgWingPolicyGrads._fields_]
    assert [int(macros["G_" + f.upper()]) for f in fields] == at
    assert int(macros["GRADS"]) == _capi.WING_POLICY_GRADS
    assert [f for f, _ in _capi.ApgWingPolicy._fields_] == fields


def test_functional_refuses_what_the_step_does_not_serve():
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.models.hutter_model import Net
    net, dyn = pc.policy(), pc.module(pc.sim_weights("w"), "cpu")
    # (stock shapes, but not on a CUDA device)
    assert F.wing_learnt_fusable(dyn) and not F.wing_learnt_policy_fusable(net, dyn)
    assert not F.wing_learnt_policy_fusable(Net(9, 1, 3, 80, conv=False), dyn)
    assert not F.wing_learnt_policy_fusable(net, object())
    _, b = pc.batch("w", 4)
    with pytest.raises(ValueError, match="fused learnt-simulator step needs"):
        F.wing_learnt_concurrent_policy_grads(net, dyn, b["normed"], b["in_ref"], b["state0"],
                                              b["ref"], pc.DT)


# ---------------------------------------------------------------- the trainer
def _real_predicate():
    from apg_trajectory_tracking_amd import functional as F
    return F.wing_learnt_policy_fusable


REAL_PREDICATE = _real_predicate()


def _trainer(flag, monkeypatch, fusable=True, dyn=None, horizon=10, net=None):
    from apg_trajectory_tracking_amd import train_fixed_wing as tf
    calls = []

    def step(net, dyn, normed, in_ref, state0, ref, dt, weights=None, index=None,
             update=None, out=None):
        calls.append(dict(index=index, update=update, dt=dt, dyn=dyn))
        flat, views = tf.F._flat_grads(torch.device("cpu"), tf.F._WING_POLICY_SHAPES)
        flat.zero_()
        return torch.tensor(3.5), views, flat
    monkeypatch.setattr(tf.F, "wing_learnt_concurrent_policy_grads", step)
    # (None: the predicate itself - on the host it refuses every pair; its shape
    # conditions are held on the device by tests/test_gpu_wing_learnt_policy.py)
    monkeypatch.setattr(tf.F, "wing_learnt_policy_fusable",
                        REAL_PREDICATE if fusable is None else lambda n, d: fusable)
    dyn = dyn if dyn is not None else pc.module(pc.sim_weights("w"), "cpu")
    t = tf.TrainFixedWing(dyn, None, dict(
        delta_t=pc.DT, delta_t_train=pc.DT, horizon=horizon, train_mode="concurrent",
        state_size=12, ref_dim=3, action_dim=4, sample_in="train_env"))
    t.net = net if net is not None else pc.policy()
    t.optimizer_controller = torch.optim.SGD(t.net.parameters(), lr=0.0, momentum=0.9)
    t.fused_learnt_policy = flag
    return t, calls


def test_the_trainer_keeps_todays_paths_unless_told_otherwise(monkeypatch):
    from apg_trajectory_tracking_amd import train_fixed_wing as tf
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    from apg_trajectory_tracking_amd.models.hutter_model import Net
    assert tf.TrainFixedWing.fused_learnt_policy is False
    _, b = pc.batch("w", 4)
    args = (b["normed"], b["state0"], b["in_ref"], b["ref"])
    # flag off: the tape (train_concurrent_fused declines, run_epoch's loader loop
    # then calls train_controller_model)
    t, calls = _trainer(False, monkeypatch)
    assert t.train_concurrent_fused(*args) is None and not calls
    assert t.train_concurrent_fused(None, None, None, None, probe=True) is False

    # flag on with the stock pair: the fused function
    t, calls = _trainer(True, monkeypatch)
    loss = t.train_concurrent_fused(*args)
    assert float(loss) == 3.5 and len(calls) == 1
    assert calls[0]["index"] is None and calls[0]["dyn"] is t.train_dynamics
    assert calls[0]["dt"] == pc.DT
    assert calls[0]["update"] is None          # (host parameters: optimizer.step() follows)
    named = dict(t.net.named_parameters())
    assert all(named[n].grad is not None for n in pc.NAMES)
    index = torch.tensor([2, 0])
    assert float(t.train_concurrent_fused(*args, index=index)) == 3.5 and len(calls) == 2
    assert calls[1]["index"] is index
    # the loops that ask first keep getting "no" for a learnt simulator
    assert t.train_concurrent_fused(None, None, None, None, probe=True) is False
    assert len(calls) == 2

    # flag on, but H = 20, a non-stock net, the policy switch off: today's paths
    t, calls = _trainer(True, monkeypatch, horizon=20)
    assert t.train_concurrent_fused(*args) is None and not calls
    t, calls = _trainer(True, monkeypatch, fusable=None, net=Net(9, 1, 3, 44, conv=False))
    assert t.train_concurrent_fused(*args) is None and not calls
    t, calls = _trainer(True, monkeypatch)
    t.fused_policy = False
    assert t.train_concurrent_fused(*args) is None and not calls
    # ... and an analytic simulator keeps wing_concurrent_policy_grads
    seen = []
    monkeypatch.setattr(tf.F, "wing_concurrent_policy_grads",
                        lambda *a, **k: seen.append(k) or (torch.tensor(1.5), {}, None))
    t, calls = _trainer(True, monkeypatch, fusable=None, dyn=FixedWingDynamics())
    assert t.train_concurrent_fused(None, None, None, None, probe=True) is True
    assert float(t.train_concurrent_fused(*args)) == 1.5 and len(seen) == 1 and not calls


def test_train_dynamics_hands_the_flag_to_the_trainer(monkeypatch):
    from apg_trajectory_tracking_amd import train_fixed_wing as tf
    seen = []
    monkeypatch.setattr(tf.TrainFixedWing, "initialize_model", lambda self, *a, **k: None)
    monkeypatch.setattr(tf.TrainFixedWing, "run_dynamics",
                        lambda self, cfg: seen.append(self.fused_learnt_policy))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = lambda: dict(delta_t=pc.DT, delta_t_train=pc.DT, horizon=10, train_mode="concurrent",
                       state_size=12, ref_dim=3, action_dim=4, modified_params={})
    tf.train_dynamics(None, cfg())
    tf.train_dynamics(None, cfg(), fused_learnt_policy=True)
    assert seen == [False, True]


# ------------------------------------------------------------------- resources
def test_the_forward_kernel_has_no_scratch_and_two_waves_per_simd():
    from apg_trajectory_tracking_amd import build
    build.build()
    with open(build.RESOURCES) as f:
        res = json.load(f)
    hits = {k: v for k, v in res.items() if "wing_learnt_policy_fwd_kernel" in k}
    assert len(hits) == 1, list(hits)
    (v,) = hits.values()
    print(v)
    assert v["scratch"] == 0 and v["vgpr_spill"] == 0, v
    assert v["occupancy"] >= 2 and v["vgprs"] + v["agprs"] <= 256, v
