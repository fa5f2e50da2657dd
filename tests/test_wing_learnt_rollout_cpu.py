"""The fused rollout through LearntFixedWingDynamics without a GPU: the host
twin of apg_wing_learnt_rollout_fwd_bwd (include/apg_cpu_wing_learnt.h - the
per-lane header of the kernel, csrc/wing_learnt_math.h, looped over the batch)
against the float64 oracle and against the recordings of the REAL module (G21,
tests/golden/make_golden_wing_learnt_rollout.py), its reduction to the analytic
rollout, the kernels' resources as the build reports them, and the trainer's
routing with the twin standing behind the functional.

Inputs: the two recorded weight sets of G16 (learnt_wing.npz: `w.`, and
`steps.w.` whose `I` is a general matrix) on synthetic.wing_batch(B, H, 0.05,
seed=40 + B).  Bound: the project's parity bar, conftest.rel_err < 1e-4; on
these inputs float32's own rounding stays near 1e-6."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.05
SETS = {"w": "w.", "steps": "steps.w."}
BAR = 1e-4


def weights(which):
    """{reference state_dict name: float32 array} of a recorded weight set."""
    g = load_golden("learnt_wing.npz")
    p = SETS[which]
    return {k[len(p):]: np.array(g[k]) for k in g.files if k.startswith(p)}


def batch(B, H):
    from apg_trajectory_tracking_amd import synthetic
    d = synthetic.wing_batch(B, H, DT, seed=40 + B)
    return d["state0"], d["actions"], d["ref"]


_ORACLE = {}


def oracle(which, B, H, dtype=torch.float64):
    """states, loss, dL/dactions, dL/dstate0 of the oracle's unroll (computed
    once per case, shared, never written to)."""
    key = (which, B, H, dtype)
    if key not in _ORACLE:
        from oracle import torch_port as tp
        ora = tp.LearntWingOracle(weights(which), dtype=dtype)
        s0, a, ref = batch(B, H)
        s0 = s0.to(dtype).requires_grad_(True)
        a = a.to(dtype).requires_grad_(True)
        states, cur = [], s0
        for k in range(H):
            cur = ora(cur, a[:, k], DT)
            states.append(cur)
        states = torch.stack(states, dim=1)
        loss = tp.fixed_wing_mpc_loss(states, ref.to(dtype), a)
        loss.backward()
        _ORACLE[key] = dict(states=states.detach().numpy(), loss=float(loss.detach()),
                            grad_actions=a.grad.numpy(), grad_state0=s0.grad.numpy())
    return _ORACLE[key]


@pytest.fixture(scope="module")
def tw():
    from apg_trajectory_tracking_amd import build as b
    return ctypes.CDLL(b.build_cpu())


def fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class HostModel:
    """ApgWingLearnt over HOST arrays: `w` a {state_dict name: array}."""

    def __init__(self, w):
        from apg_trajectory_tracking_amd import _capi
        theta = np.zeros(41, np.float32)
        for i, n in enumerate(_capi.WING_PARAM_FIELDS):
            if "cfg." + n in w:
                theta[i] = np.asarray(w["cfg." + n]).reshape(-1)[0]
        self.arrays = [theta] + [np.ascontiguousarray(w[k], np.float32) for k in (
            "I", "linear_state_1.weight", "linear_state_1.bias",
            "linear_state_2.weight", "linear_state_2.bias")]
        self.struct = _capi.ApgWingLearnt(*[a.ctypes.data for a in self.arrays])


def module_weights(dyn):
    return {k: v.detach().cpu().numpy() for k, v in dyn.state_dict().items()}


def twin_rollout(tw, w, state0, actions, ref, dt=DT, layout="aos", want_states=True,
                 want_grad_state0=True, want_loss=True, pos=10.0, action=0.1):
    """The twin behind the argument and result conventions of
    functional.wing_learnt_rollout_fwd_bwd; tensors [B,12] / [B,H,4] / [B,H,3]
    in, results in the same (AoS) shapes whatever `layout` the twin ran in."""
    from apg_trajectory_tracking_amd import _capi
    s0 = np.ascontiguousarray(np.asarray(state0, np.float32))
    a = np.ascontiguousarray(np.asarray(actions, np.float32))
    r = np.ascontiguousarray(np.asarray(ref, np.float32))
    B, H = a.shape[0], a.shape[1]
    soa = layout == "soa"
    if soa:
        s0, a, r = (np.ascontiguousarray(s0.T), np.ascontiguousarray(a.transpose(1, 2, 0)),
                    np.ascontiguousarray(r.transpose(1, 2, 0)))
    parts = np.zeros(_capi.loss_partials_count(B), np.float32)
    loss = np.full(1, np.nan, np.float32) if want_loss else None
    ga = np.full(a.shape, np.nan, np.float32)
    gs = np.full(s0.shape, np.nan, np.float32) if want_grad_state0 else None
    st = (np.full((H, 12, B) if soa else (B, H, 12), np.nan, np.float32)
          if want_states else None)
    m = HostModel(w)
    lw = _capi.ApgWingLossWeights(pos, action)
    rc = tw.apg_wing_learnt_rollout_fwd_bwd_cpu(
        fp(s0), fp(a), fp(r), ctypes.c_float(dt), ctypes.byref(m.struct), ctypes.byref(lw),
        B, H, _capi.LAYOUT_SOA if soa else _capi.LAYOUT_AOS, fp(parts), fp(loss), fp(ga),
        fp(gs), fp(st), None)
    assert rc == 0, rc
    if soa:
        ga = ga.transpose(2, 0, 1)
        gs = None if gs is None else gs.T
        st = None if st is None else st.transpose(2, 0, 1)
    return dict(loss=None if loss is None else loss.copy(), loss_partials=parts,
                grad_actions=ga, grad_state0=gs, states=st)


def check_against(res, want, what, bar=BAR):
    """The four outputs against `want` at the parity bar; prints the errors."""
    errs = dict(
        states=rel_err(res["states"], want["states"]),
        loss=abs(float(res["loss"][0]) - want["loss"]) / abs(want["loss"]),
        grad_actions=rel_err(res["grad_actions"], want["grad_actions"]),
        grad_state0=rel_err(res["grad_state0"], want["grad_state0"]))
    print(what, {k: float("%.3g" % v) for k, v in errs.items()})
    for k, v in errs.items():
        assert v < bar, (what, k, v)
    return errs


# ---------------------------------------------------------- twin vs oracle
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("B,H", [(1, 20), (67, 10), (67, 20)])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_twin_against_float64_oracle(tw, which, B, H, layout):
    s0, a, ref = batch(B, H)
    res = twin_rollout(tw, weights(which), s0, a, ref, layout=layout)
    want = oracle(which, B, H)
    check_against(res, want, f"twin/{which}/B{B}/H{H}/{layout}")
    # one partial per 64 trajectories, summed in order
    assert res["loss_partials"].shape == ((B + 63) // 64,)
    assert abs(float(res["loss_partials"].sum()) - want["loss"]) < BAR * abs(want["loss"])


def test_twin_optional_outputs_and_argument_errors(tw):
    """NULL grad_state0 / states_out / loss drop their writes and change nothing
    else; B = 0 zeroes the loss; H outside [1, APG_MAX_HORIZON], a NULL model
    pointer and an unknown layout are argument errors."""
    from apg_trajectory_tracking_amd import _capi
    B, H = 67, 10
    s0, a, ref = batch(B, H)
    w = weights("steps")
    full = twin_rollout(tw, w, s0, a, ref)
    bare = twin_rollout(tw, w, s0, a, ref, want_states=False, want_grad_state0=False,
                        want_loss=False)
    assert bare["loss"] is None and bare["grad_state0"] is None and bare["states"] is None
    assert np.array_equal(bare["grad_actions"], full["grad_actions"])
    assert np.array_equal(bare["loss_partials"], full["loss_partials"])
    m = HostModel(w)
    lw = _capi.ApgWingLossWeights(10.0, 0.1)
    s, ac, r = (np.ascontiguousarray(t.numpy(), np.float32) for t in (s0, a, ref))
    parts, loss = np.zeros(2, np.float32), np.full(1, 7.0, np.float32)
    ga = np.zeros_like(ac)

    def call(model, Bc, Hc, lay=_capi.LAYOUT_AOS):
        return tw.apg_wing_learnt_rollout_fwd_bwd_cpu(
            fp(s), fp(ac), fp(r), ctypes.c_float(DT), model, ctypes.byref(lw), Bc, Hc, lay,
            fp(parts), fp(loss), fp(ga), None, None, None)
    assert call(ctypes.byref(m.struct), 0, H) == 0 and loss[0] == 0.0
    for bad_h in (0, -3, _capi.MAX_HORIZON + 1):
        assert call(ctypes.byref(m.struct), B, bad_h) == -1
    assert call(ctypes.byref(m.struct), B, _capi.MAX_HORIZON + 1) == -1
    assert call(ctypes.byref(m.struct), -1, H) == -1
    assert call(ctypes.byref(m.struct), B, H, 7) == -1
    assert call(None, B, H) == -1
    broken = _capi.ApgWingLearnt(*[x.ctypes.data for x in m.arrays[:5]], None)
    assert call(ctypes.byref(broken), B, H) == -1
    assert not np.any(ga)           # nothing ran


# ---------------------------------------------------------- twin vs golden
def golden_case(g, which, B, H):
    p = f"{which}.B{B}.H{H}."
    return {k: g[p + k] for k in ("sel", "states", "grad_actions", "grad_state0")} | {
        "loss": float(g[p + "loss"])}


@pytest.mark.parametrize("B", [1, 67, 1003])
@pytest.mark.parametrize("H", [10, 20])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_twin_against_golden_of_the_real_module(tw, which, B, H):
    want = golden_case(load_golden("wing_learnt_rollout.npz"), which, B, H)
    s0, a, ref = batch(B, H)
    res = twin_rollout(tw, weights(which), s0, a, ref)
    sel = want["sel"]
    got = dict(loss=res["loss"], states=res["states"][sel],
               grad_actions=res["grad_actions"][sel], grad_state0=res["grad_state0"][sel])
    check_against(got, want, f"twin vs real module/{which}/B{B}/H{H}")


# ------------------------------------------- zero residual = analytic rollout
def test_zero_residual_reduces_to_the_analytic_rollout(tw):
    """All four residual tensors zero and the nominal parameters: the learnt
    rollout is apg_wing_rollout_fwd_bwd_cpu's to 1e-5 (the general-inertia
    table takes another arithmetic path, so not bit for bit)."""
    from apg_trajectory_tracking_amd import _capi, functional as F
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
        DEFAULT_CONFIG, LearntFixedWingDynamics)
    B, H = 67, 20
    s0, a, ref = batch(B, H)
    w = module_weights(LearntFixedWingDynamics())
    assert not any(np.any(w[k]) for k in w if k.startswith("linear_state"))
    res = twin_rollout(tw, w, s0, a, ref)
    s, ac, r = (np.ascontiguousarray(t.numpy(), np.float32) for t in (s0, a, ref))
    params, lw = F.wing_params(DEFAULT_CONFIG), _capi.ApgWingLossWeights(10.0, 0.1)
    parts, loss = np.zeros((B + 63) // 64, np.float32), np.zeros(1, np.float32)
    ga, gs, st = np.zeros_like(ac), np.zeros_like(s), np.zeros((B, H, 12), np.float32)
    assert tw.apg_wing_rollout_fwd_bwd_cpu(
        fp(s), fp(ac), fp(r), ctypes.c_float(DT), ctypes.byref(params), ctypes.byref(lw), B,
        H, _capi.LAYOUT_AOS, fp(parts), fp(loss), fp(ga), fp(gs), fp(st), None) == 0
    check_against(res, dict(states=st, loss=float(loss[0]), grad_actions=ga, grad_state0=gs),
                  "zero residual vs analytic twin", bar=1e-5)


def test_twin_repeats_the_device_signature(tw):
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    cpu = open(os.path.join(REPO, "include", "apg_cpu_wing_learnt.h")).read()
    gpu = open(os.path.join(REPO, "include", "apg.h")).read()
    decls = re.findall(r"\bint\s+(apg_\w+_cpu)\s*\(([^;]*?)\)\s*;", cpu, re.S)
    assert [d[0] for d in decls] == ["apg_wing_learnt_rollout_fwd_bwd_cpu"]
    name, args = decls[0]
    assert hasattr(tw, name)
    m = re.search(r"\bint\s+" + name[:-4] + r"\s*\(([^;]*?)\)\s*;", gpu, re.S)
    dev_args = norm(m.group(1))
    assert dev_args.endswith(", apg_stream_t stream")
    assert norm(args) == dev_args[:-len(", apg_stream_t stream")]


# -------------------------------------------------------------- resources
def test_rollout_kernels_have_no_scratch_and_no_spills():
    from apg_trajectory_tracking_amd import build
    build.build()
    with open(build.RESOURCES) as f:
        res = json.load(f)
    mine = {k: v for k, v in res.items() if "wing_learnt_rollout" in k}
    layouts = [k for k in mine if "wing_learnt_rollout_kernelILi" in k]
    assert len(layouts) >= 2, sorted(mine)
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)


# ------------------------------------------------ trainer routing, no GPU
class _TwinLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state0, action_seq, ref, dt, dyn, lib):
        res = twin_rollout(lib, module_weights(dyn), state0.detach().numpy(),
                           action_seq.detach().numpy(), ref.detach().numpy(), dt)
        ctx.save_for_backward(torch.from_numpy(np.ascontiguousarray(res["grad_actions"])),
                              torch.from_numpy(np.ascontiguousarray(res["grad_state0"])))
        return torch.tensor(float(res["loss"][0]))

    @staticmethod
    def backward(ctx, g):
        ga, gs = ctx.saved_tensors
        return (gs * g if ctx.needs_input_grad[0] else None, ga * g, None, None, None, None)


def _trainer(train_dynamics, H, tmp_path):
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    from apg_trajectory_tracking_amd.train_fixed_wing import TrainFixedWing
    cfg = dict(delta_t=DT, delta_t_train=DT, epoch_size=8, self_play=0, batch_size=8,
               state_size=12, horizon=H, ref_dim=3, action_dim=4, train_mode="concurrent",
               learning_rate_controller=1e-7, system="wing",
               save_name=str(tmp_path / "t"), sample_in="train_env")
    return TrainFixedWing(train_dynamics, FixedWingDynamics(), cfg)


def test_trainer_routes_to_the_fused_loss_when_fusable(tw, tmp_path, monkeypatch):
    """_fusable_learnt() for the stock module, an analytic simulator, a residual
    of another width and fused_learnt = False; the fused route calls
    functional.wing_learnt_rollout_loss (here: the twin behind it) and steps the
    optimizer with its gradients; every other case takes the loop it took
    before."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
        FixedWingDynamics, LearntFixedWingDynamics)
    B, H = 8, 10
    s0, a, ref = batch(B, H)
    learnt = LearntFixedWingDynamics()
    learnt.load_state_dict({k: torch.from_numpy(v) for k, v in weights("steps").items()})
    calls = []

    def fused(dyn, state0, action_seq, ref_states, dt, weights=None):
        calls.append(("fused", dt))
        return _TwinLoss.apply(state0, action_seq, ref_states, dt, dyn, tw)

    def analytic(*args, **kw):
        calls.append(("analytic",))
        return (args[1] ** 2).sum()
    monkeypatch.setattr(F, "wing_learnt_rollout_loss", fused)
    monkeypatch.setattr(F, "wing_rollout_loss", analytic)

    def run(t):
        raw = torch.logit(a.clone()).requires_grad_(True)
        t.optimizer_controller = torch.optim.SGD([raw], lr=1e-6)
        loss = t.train_controller_model(s0.clone(), torch.sigmoid(raw), None, ref)
        return float(loss), raw

    t = _trainer(learnt, H, tmp_path)
    assert t.fused_learnt is True and t._fusable_learnt()
    before = torch.logit(a.clone())
    loss, raw = run(t)
    assert calls == [("fused", DT)]
    want = oracle("steps", B, H)
    assert abs(loss - want["loss"]) < BAR * abs(want["loss"])
    g_raw = torch.from_numpy(want["grad_actions"]) * (a * (1 - a)).double()
    assert rel_err(raw.grad.numpy(), g_raw.numpy()) < BAR
    assert not torch.equal(before, raw.detach())          # the optimizer stepped
    assert torch.allclose(raw.detach(), before - 1e-6 * raw.grad, rtol=0, atol=1e-6)
    assert all(p.grad is None for p in learnt.parameters())

    # horizon beyond the kernel's limit, fused_learnt off, another width: the loop
    steps = []

    def stand_in(state, action, dt):
        steps.append(dt)
        return state + action.sum(1, keepdim=True)
    wide = LearntFixedWingDynamics()
    wide.linear_state_1 = torch.nn.Linear(16, 32)
    wide.linear_state_2 = torch.nn.Linear(32, 12)
    off = _trainer(learnt, H, tmp_path)
    off.fused_learnt = False
    far = _trainer(learnt, 49, tmp_path)
    for tr, dyn in ((off, learnt), (_trainer(wide, H, tmp_path), wide)):
        assert not tr._fusable_learnt()
        dyn.forward = stand_in
        del calls[:], steps[:]
        run(tr)
        assert calls == [] and steps == [DT] * H
        del dyn.forward
    assert not far._fusable_learnt()
    # an analytic simulator keeps its own fused rollout
    ana = _trainer(FixedWingDynamics(), H, tmp_path)
    assert not ana._fusable_learnt()
    del calls[:]
    run(ana)
    assert calls == [("analytic",)]
