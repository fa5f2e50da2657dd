"""The fused rollout through LearntFixedWingDynamics on the GPU
(csrc/wing_learnt.hip: apg_wing_learnt_rollout_fwd_bwd - H x (physics on the
module's live parameters + the 16 -> 64 -> 12 residual) + fixed_wing_mpc_loss +
the reverse sweep in one fused launch) against the float64 oracle, the module's
own step-by-step autograd unroll on the device, the host twin and the
recordings of the REAL module (G21); its parameters read live and without a
host read-back; the autograd Function through a policy; and TrainFixedWing's
controller phase on it.

Inputs and bound as tests/test_wing_learnt_rollout_cpu.py: the recorded weight
sets on synthetic.wing_batch(B, H, 0.05, seed=40 + B), conftest.rel_err < 1e-4."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from test_wing_learnt_rollout_cpu import (BAR, DT, batch, check_against, golden_case,
                                          oracle, tw, twin_rollout, weights)  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def module(which, dev):
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
        LearntFixedWingDynamics)
    dyn = LearntFixedWingDynamics()
    res = dyn.load_state_dict({k: torch.from_numpy(v) for k, v in weights(which).items()})
    assert not res.missing_keys and not res.unexpected_keys
    return dyn.to(dev)


def fused(dyn, s0, a, ref, layout="aos", **kw):
    """functional.wing_learnt_rollout_fwd_bwd on AoS inputs in either layout;
    results as float64-comparable numpy arrays in the AoS shapes."""
    from apg_trajectory_tracking_amd import functional as F
    if layout == "soa":
        args = (s0.t().contiguous(), a.permute(1, 2, 0).contiguous(),
                ref.permute(1, 2, 0).contiguous())
    else:
        args = (s0, a, ref)
    res = F.wing_learnt_rollout_fwd_bwd(dyn, *args, DT, layout=layout, want_states=True, **kw)
    out = {k: (None if v is None else v.detach().cpu().numpy()) for k, v in res.items()}
    if layout == "soa":
        out["grad_actions"] = out["grad_actions"].transpose(2, 0, 1)
        out["states"] = out["states"].transpose(2, 0, 1)
        if out["grad_state0"] is not None:
            out["grad_state0"] = out["grad_state0"].T
    return out


def unroll_loss(dyn, s0, actions, ref):
    """The parent's controller phase: the module step by step + the loss."""
    from apg_trajectory_tracking_amd.drone_loss import fixed_wing_mpc_loss
    states, cur = [], s0
    for k in range(actions.shape[1]):
        cur = dyn(cur, actions[:, k], dt=DT)
        states.append(cur)
    states = torch.stack(states, dim=1)
    return fixed_wing_mpc_loss(states, ref, actions), states


@pytest.mark.parametrize("H", [1, 10, 20])
@pytest.mark.parametrize("B", [1, 67, 1003, 4099])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_kernel_against_oracle_device_unroll_and_twin(dev, tw, which, B, H):
    """One lane, a ragged second wave, many workgroups with the partial-sum
    reduction; both layouts; states, loss, dL/dactions and dL/dstate0."""
    s0, a, ref = batch(B, H)
    dyn = module(which, dev)
    want = oracle(which, B, H)
    d0, da, dr = s0.to(dev), a.to(dev), ref.to(dev)
    host = twin_rollout(tw, weights(which), s0, a, ref)
    host = dict(host, loss=float(host["loss"][0]))
    # the module's own autograd unroll on the device
    us, ua = d0.clone().requires_grad_(True), da.clone().requires_grad_(True)
    ul, ustates = unroll_loss(dyn, us, ua, dr)
    ul.backward()
    stepwise = dict(states=ustates.detach().cpu().numpy(), loss=float(ul.detach()),
                    grad_actions=ua.grad.cpu().numpy(), grad_state0=us.grad.cpu().numpy())
    for layout in ("aos", "soa"):
        res = fused(dyn, d0, da, dr, layout)
        tag = f"{which}/B{B}/H{H}/{layout}"
        check_against(res, want, "kernel vs float64 oracle " + tag)
        check_against(res, stepwise, "kernel vs device unroll " + tag)
        check_against(res, host, "kernel vs host twin " + tag)
        parts = res["loss_partials"]
        assert parts.shape == ((B + 63) // 64,)
        assert abs(float(parts.astype(np.float64).sum()) - want["loss"]) < BAR * want["loss"]


def test_optional_outputs_and_argument_errors(dev):
    from apg_trajectory_tracking_amd import functional as F
    B, H = 67, 10
    s0, a, ref = (t.to(dev) for t in batch(B, H))
    dyn = module("steps", dev)
    full = F.wing_learnt_rollout_fwd_bwd(dyn, s0, a, ref, DT, want_states=True)
    bare = F.wing_learnt_rollout_fwd_bwd(dyn, s0, a, ref, DT, want_grad_state0=False)
    assert bare["grad_state0"] is None and bare["states"] is None
    assert torch.equal(bare["grad_actions"], full["grad_actions"])
    assert torch.equal(bare["loss"], full["loss"])
    empty = F.wing_learnt_rollout_fwd_bwd(
        dyn, s0[:0], a[:0], ref[:0], DT)
    assert float(empty["loss"]) == 0.0
    with pytest.raises(ValueError):
        F.wing_learnt_rollout_fwd_bwd(dyn, s0, torch.zeros(B, 49, 4, device=dev),
                                      torch.zeros(B, 49, 3, device=dev), DT)
    with pytest.raises(ValueError):
        F.wing_learnt_rollout_fwd_bwd(dyn, s0, a, ref, DT, layout="packed")
    with pytest.raises(ValueError):
        F.wing_learnt_rollout_fwd_bwd(dyn, s0, a, ref[:, :5], DT)
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
        LearntFixedWingDynamics)
    with pytest.raises(RuntimeError):        # a module that is not on the device
        F.wing_learnt_rollout_fwd_bwd(LearntFixedWingDynamics(), s0, a, ref, DT)


@pytest.mark.parametrize("B", [1, 67, 1003])
@pytest.mark.parametrize("H", [10, 20])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_kernel_against_golden_of_the_real_module(dev, which, B, H):
    want = golden_case(load_golden("wing_learnt_rollout.npz"), which, B, H)
    s0, a, ref = (t.to(dev) for t in batch(B, H))
    res = fused(module(which, dev), s0, a, ref)
    sel = want["sel"]
    got = dict(loss=res["loss"], states=res["states"][sel],
               grad_actions=res["grad_actions"][sel], grad_state0=res["grad_state0"][sel])
    check_against(got, want, f"kernel vs real module/{which}/B{B}/H{H}")


def test_live_parameters_without_a_host_read(dev, monkeypatch):
    """mass, rho and I change in place between two calls: the second call
    equals a fresh oracle built from the new values - and neither call reads a
    tensor back (Tensor.cpu / .tolist / .item raise while it runs)."""
    from oracle import torch_port as tp
    B, H = 67, 10
    s0, a, ref = batch(B, H)
    d0, da, dr = s0.to(dev), a.to(dev), ref.to(dev)
    dyn = module("steps", dev)

    def no_read(*args, **kw):
        raise AssertionError("host read-back on the call path")

    def guarded():
        from apg_trajectory_tracking_amd import functional as F
        with monkeypatch.context() as mp:
            for name in ("cpu", "tolist", "item", "numpy"):
                mp.setattr(torch.Tensor, name, no_read)
            res = F.wing_learnt_rollout_fwd_bwd(dyn, d0, da, dr, DT, want_states=True)
        return {k: v.detach().cpu().numpy() for k, v in res.items()}
    first = guarded()
    check_against(first, oracle("steps", B, H), "before the change")
    with torch.no_grad():
        dyn.cfg["mass"].mul_(1.15)
        dyn.cfg["rho"].sub_(0.1)
        dyn.I.add_(torch.tensor([[2e-3, 1e-3, 0.], [-5e-4, 3e-3, 4e-4],
                                 [0., -2e-4, -4e-3]], device=dev))
    second = guarded()
    ora = tp.LearntWingOracle({k: v.detach().cpu().numpy()
                               for k, v in dyn.state_dict().items()})
    s64 = s0.double().requires_grad_(True)
    a64 = a.double().requires_grad_(True)
    states, cur = [], s64
    for k in range(H):
        cur = ora(cur, a64[:, k], DT)
        states.append(cur)
    states = torch.stack(states, dim=1)
    loss = tp.fixed_wing_mpc_loss(states, ref.double(), a64)
    loss.backward()
    want = dict(states=states.detach().numpy(), loss=float(loss.detach()),
                grad_actions=a64.grad.numpy(), grad_state0=s64.grad.numpy())
    check_against(second, want, "after the change")
    moved = rel_err(second["states"], first["states"])
    print("the change moved the states by", moved)
    assert moved > 100 * BAR        # (the two calls are not the same answer)


def policy(H, dev, seed=5):
    from apg_trajectory_tracking_amd.models.hutter_model import Net
    torch.manual_seed(seed)
    return Net(9, 1, 3, 4 * H, conv=False).to(dev)


@pytest.mark.parametrize("B", [8, 64])
def test_rollout_loss_through_a_policy(dev, B):
    """wing_learnt_rollout_loss behind a policy: the policy's gradients equal
    those of the unrolled loss; the simulator's parameters receive none."""
    from apg_trajectory_tracking_amd import functional as F
    H = 10
    s0, _, ref = (t.to(dev) for t in batch(B, H))
    dyn = module("steps", dev)
    net = policy(H, dev)
    in_state, in_ref = s0[:, 3:], (ref[:, 0] - s0[:, :3]).contiguous()

    def actions():
        return torch.sigmoid(net(in_state, in_ref)).view(B, H, 4)
    net.zero_grad()
    lf = F.wing_learnt_rollout_loss(dyn, s0, actions(), ref, DT)
    lf.backward()
    # (conv_ref is registered but unused by a conv=False policy: no gradient)
    got = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    assert {"states_in.weight", "ref_in.weight", "fc1.weight", "fc_out.bias"} <= set(got)
    assert all(p.grad is None for p in dyn.parameters())
    net.zero_grad()
    lu, _ = unroll_loss(dyn, s0, actions(), ref)
    lu.backward()
    lf, lu = float(lf.detach()), float(lu.detach())
    assert abs(lf - lu) < BAR * abs(lu)
    want = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    assert set(want) == set(got)
    errs = {k: rel_err(got[k].cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("policy gradients, fused vs unrolled:", {k: float("%.3g" % v)
                                                   for k, v in errs.items()})
    assert max(errs.values()) < BAR, errs


def test_trainer_takes_the_fused_path(dev, tmp_path, monkeypatch):
    """One controller epoch of TrainFixedWing through a learnt simulator: the
    fused functional is called; loss and updated policy equal those of a twin
    trainer on the step-by-step loop (fused_learnt = False) from the same seed."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    from apg_trajectory_tracking_amd.train_fixed_wing import TrainFixedWing
    monkeypatch.chdir(tmp_path)
    cfg = dict(delta_t=0.05, delta_t_train=0.05, epoch_size=256, self_play=0,
               batch_size=64, state_size=12, horizon=20, ref_dim=3, action_dim=4,
               train_mode="concurrent", learning_rate_controller=1e-7,
               learning_rate_dynamics=2e-5, l2_lambda=0.01, system="wing",
               save_name="t", sample_in="train_env")
    calls = []
    real = F.wing_learnt_rollout_loss

    def spy(*args, **kw):
        calls.append(tuple(args[2].shape))
        return real(*args, **kw)
    monkeypatch.setattr(F, "wing_learnt_rollout_loss", spy)

    def one_epoch(fused_learnt):
        t = TrainFixedWing(module("steps", dev), FixedWingDynamics({"mass": 1.2}), dict(cfg))
        t.fused_learnt = fused_learnt
        torch.manual_seed(2)
        t.initialize_model(device=dev, seed=3)
        assert t._fusable_learnt() == fused_learnt
        start = [p.detach().clone() for p in t.net.parameters()]
        torch.manual_seed(4)
        loss = t.run_epoch(train="controller")
        return float(loss), start, [p.detach().clone() for p in t.net.parameters()]
    lf, start, pf = one_epoch(True)
    assert calls == [(64, 20, 4)] * 4
    del calls[:]
    lu, start_u, pu = one_epoch(False)
    assert calls == []
    assert all(torch.equal(x, y) for x, y in zip(start, start_u))
    assert np.isfinite(lf) and abs(lf - lu) < BAR * abs(lu), (lf, lu)
    assert any(not torch.equal(x, y) for x, y in zip(start, pf))
    errs = [rel_err(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(pf, pu)]
    moves = [rel_err((x - s).cpu().numpy(), (y - s).cpu().numpy())
             for x, y, s in zip(pf, pu, start)]
    print("updated policy, fused vs loop:", errs, "updates themselves:", moves)
    assert max(errs) < BAR, errs
