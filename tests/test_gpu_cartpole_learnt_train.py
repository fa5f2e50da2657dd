"""The fused controller step of the cart-pole through LearntCartpoleDynamics on
the GPU (apg_cartpole_learnt_mlp_train_step through
functional.cartpole_learnt_policy_train_step, TrainCartpole.run_epoch and
train_norm_dynamics): the recording of the real reference step (G20), the host
twin of test_cartpole_learnt_train_cpu.py at every shape that takes another path
through the kernels, the existing learnt rollout kernel on the same actions,
run-to-run determinism, the in-kernel momentum SGD, a graph capture of the whole
step and a replay after the simulator has changed, non-finite inputs, and the
trainer's choice between the fused step and the tape.  Both simulators of the
CPU file throughout.  Bounds: conftest.rel_err < 1e-4 on every gradient tensor,
the actions and the loss, 1e-5 on post-step weights, the update against its
formula at rtol 1e-6.  Every test prints what it saw."""
import numpy as np
import pytest
import torch

import test_cartpole_learnt_train_cpu as cpu
import test_cartpole_train_cpu as ref
from conftest import load_golden, rel_err
from test_cartpole_train_cpu import tw  # noqa: F401  (the host twins, a fixture)

pytestmark = pytest.mark.gpu
BAR, BAR_W = ref.BAR, ref.BAR_W
# 1 221 samples are 20 rows of the second stage; 16 451 are 258 chunks on 256
# workgroups (test_gpu_cartpole_train.py)
B_ROWS, B_CHUNKS = 1221, 16451
SHAPES = [(1, 5, .05), (8, 10, .05), (64, 5, .05), (67, 10, .05), (321, 10, .05),
          (67, 1, .05), (67, 48, .01), (B_ROWS, 10, .05), (B_CHUNKS, 5, .05)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def network(w, dev, cls=None):
    from apg_trajectory_tracking_amd.models.simple_model import Net
    net = (cls or Net)(4, w["fc_out.bias"].shape[0])
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in w.items()})
    return net.to(dev)


def frozen_copy(dyn):
    return {k: v.detach().clone() for k, v in dyn.state_dict().items()}


def assert_untouched(dyn, before):
    for k, v in dyn.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in dyn.parameters())


def step(net, dyn, dev, in_state, state0, dt, **kw):
    """functional.cartpole_learnt_policy_train_step, results as the twin's."""
    from apg_trajectory_tracking_amd import functional as F
    to = lambda x: x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)).to(dev)
    res = F.cartpole_learnt_policy_train_step(net, dyn, to(in_state), to(state0), dt,
                                              want_actions=True, **kw)
    assert list(res["grads"]) == [k for k, _ in net.named_parameters()]
    off = 0
    for k, v in res["grads"].items():               # views at the published offsets
        assert v.data_ptr() == res["flat"].data_ptr() + 4 * off and v.is_contiguous(), k
        off += v.numel()
    assert res["flat"].numel() == off + 1           # + the loss slot
    return dict(loss=float(res["loss"].item()), flat=N(res["flat"])[:-1],
                g={k: N(v) for k, v in res["grads"].items()}, actions=N(res["actions"]),
                raw=res)


def trainer(dev, net, dyn, states, labels, fused, batch, H, dt=.05, lr=1e-4):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.train_cartpole import TrainCartpole
    cfg = dict(delta_t=dt, batch_size=batch, state_size=4, horizon=H, action_dim=1,
               ref_dim=4, train_mode="concurrent", learning_rate_controller=lr,
               learning_rate_dynamics=1e-3, l2_lambda=0, system="cartpole")
    t = TrainCartpole(dyn, CartpoleDynamics(), cfg)

    class Data:
        num_sampled_states = states.shape[0]
    Data.states, Data.labels = states, labels
    t.initialize_model(base_model=net, state_data=Data, device=dev)
    t.shuffle = False
    t.init_optimizer()
    t.fused_learnt_policy = fused
    return t


def count_calls(monkeypatch):
    """(calls of the learnt functional, calls of the analytic one)"""
    from apg_trajectory_tracking_amd import functional as F
    mine, other = [], []
    real, real_other = F.cartpole_learnt_policy_train_step, F.cartpole_policy_train_step
    monkeypatch.setattr(F, "cartpole_learnt_policy_train_step",
                        lambda *p, **kw: mine.append(kw) or real(*p, **kw))
    monkeypatch.setattr(F, "cartpole_policy_train_step",
                        lambda *p, **kw: other.append(kw) or real_other(*p, **kw))
    return mine, other


# ---------------------------------------------------------------- 1: golden
@pytest.mark.parametrize("B", [8, 64])
def test_golden_through_the_functional_call(dev, B):
    from test_cartpole_eval_cpu import golden_net
    g = cpu.lref.g20()
    net = golden_net(load_golden("cartpole_closed_loop.npz"), "shipped").to(dev)
    dyn = cpu.lref.fitted(g).to(dev)
    before = frozen_copy(dyn)
    got = step(net, dyn, dev, g[f"ctrl{B}.state"], g[f"ctrl{B}.state"], cpu.lref.DT)
    want = float(g[f"ctrl{B}.loss"])
    e_l = abs(got["loss"] - want) / abs(want)
    errs = {k: rel_err(got["g"][k], g[f"ctrl{B}.grad.{k}"]) for k in ref.names()}
    print(f"gpu G20 ctrl{B} loss {e_l:.2e} worst gradient {max(errs.values()):.2e}")
    assert e_l < BAR
    for k, e in errs.items():
        assert e < BAR, (k, e)
    assert_untouched(dyn, before)


# ------------------------------------------------------------ 2: the host twin
@pytest.mark.parametrize("kind", cpu.SIMULATORS)
@pytest.mark.parametrize("B,H,dt", SHAPES)
def test_against_the_host_twin(dev, tw, kind, B, H, dt):  # noqa: F811
    """The same per-sample headers on both sides: what differs is the order of
    the sums over the batch, the device's tanh / sin / cos and fma contraction."""
    m = cpu.simulator(kind)
    s0 = cpu.case(kind, B, H, dt)
    x = s0 if B != 321 else cpu.case(kind, B + 1, H, dt)[:B]    # in_state != state0 once
    w = ref.seeded_weights(H)
    want = cpu.twin_step(tw, m, w, x, s0, dt)
    got = step(network(w, dev), m.to(dev), dev, x, s0, dt)
    errs = {"loss": abs(got["loss"] - want["loss"]) / abs(want["loss"]),
            "actions": rel_err(got["actions"], want["actions"]),
            "flat": rel_err(got["flat"], want["flat"][:-1])}
    errs.update((k, rel_err(got["g"][k], want["g"][k])) for k in ref.names())
    print(f"gpu vs twin {kind} B={B} H={H} dt={dt}",
          {k: float("%.3g" % v) for k, v in errs.items()})
    assert np.all(np.isfinite(got["flat"]))
    for k, v in errs.items():
        assert v < BAR, (k, v)


# ------------------------------------- 3: the existing learnt rollout kernel
@pytest.mark.parametrize("kind", cpu.SIMULATORS)
@pytest.mark.parametrize("B", [67, B_ROWS])
def test_same_arithmetic_as_the_learnt_rollout_kernel(dev, kind, B):
    """Per sample both kernels call the same two functions of
    cartpole_learnt_math.h; the sums over the batch are ordered differently."""
    from apg_trajectory_tracking_amd import functional as F
    H, dt = 10, .05
    dyn = cpu.simulator(kind).to(dev)
    s0 = torch.as_tensor(cpu.case(kind, B, H, dt)).to(dev)
    got = step(network(ref.seeded_weights(H), dev), dyn, dev, s0, s0, dt)
    roll = F.cartpole_learnt_rollout_fwd_bwd(dyn, s0, got["raw"]["actions"].contiguous(), dt)
    want = float(roll["loss"].item())
    e = abs(got["loss"] - want) / abs(want)
    print(f"train step vs rollout kernel {kind} B={B}: loss {got['loss']:.7g} rel {e:.2e}")
    assert e <= 1e-6


# ------------------------------------------------------------- 4: determinism
@pytest.mark.parametrize("B", [64, B_ROWS])
def test_two_calls_give_the_same_bits(dev, B):
    net = network(ref.seeded_weights(10), dev)
    dyn = cpu.simulator("seeded").to(dev)
    s0 = cpu.case("seeded", B, 10, .05)
    a, b = (step(net, dyn, dev, s0, s0, .05) for _ in range(2))
    assert a["raw"]["flat"].data_ptr() != b["raw"]["flat"].data_ptr()
    assert np.array_equal(a["flat"], b["flat"]) and a["loss"] == b["loss"]
    assert np.array_equal(a["actions"], b["actions"])
    assert np.any(a["flat"] != 0) and a["loss"] > 0


# ------------------------------------------------------------------ 5: update
@pytest.mark.parametrize("B", [8, 321])
def test_in_kernel_momentum_sgd_over_two_steps(dev, B):
    """One launch (B = 8) and with the second stage (B = 321); the simulator is
    read, never written, and gets no gradient."""
    lr, mom, H = 1e-4, 0.9, 10
    net = network(ref.seeded_weights(H), dev)
    dyn = cpu.simulator("fitted").to(dev)
    before = frozen_copy(dyn)
    s0 = torch.as_tensor(cpu.case("fitted", B, H, .05)).to(dev)
    params = dict(net.named_parameters())
    start = {k: p.detach().clone() for k, p in params.items()}
    bufs = {k: torch.zeros_like(p) for k, p in params.items()}
    want_p = {k: v.clone() for k, v in start.items()}
    want_m = {k: torch.zeros_like(v) for k, v in start.items()}
    for it in range(2):
        plain = step(net, dyn, dev, s0, s0, .05)
        versions = [p._version for p in params.values()]
        for k in want_p:
            # the formula as the rule states it: in double, rounded once each
            g = torch.as_tensor(plain["g"][k]).to(dev)
            want_m[k] = (mom * want_m[k].double() + g.double()).float()
            want_p[k] = (want_p[k].double() - lr * want_m[k].double()).float()
        got = step(net, dyn, dev, s0, s0, .05, update=(lr, mom, bufs))
        assert got["loss"] == plain["loss"]
        assert all(p._version > v for p, v in zip(params.values(), versions))
        for k, p in params.items():
            assert np.array_equal(got["g"][k], plain["g"][k]), k     # gradients all the same
            m, wm, wp = bufs[k], want_m[k], want_p[k]
            assert torch.allclose(m, wm, rtol=1e-6, atol=1e-6 * float(wm.abs().max())), k
            assert torch.allclose(p.detach(), wp, rtol=1e-6, atol=1e-9), k
            assert not torch.equal(p.detach(), wp + lr * wm), k      # it moved
    assert all(not torch.equal(p.detach(), start[k]) for k, p in params.items())
    assert_untouched(dyn, before)


# --------------------------------------------------------------- 6, 7: graph
@pytest.mark.parametrize("B", [64, 321])
def test_the_whole_step_is_capturable_and_a_replay_reads_the_live_simulator(dev, B):
    """Three replays of the captured step = three eager steps from the same
    start, bit for bit: parameters, momentum buffers, gradients, loss (H = 10:
    the workgroup's LDS is above 64 KB, so the capture includes whatever the
    entry point does about that).  Then the simulator's `length` and
    `linear_state_2.weight` are scaled in place and the policy reset: one more
    replay equals an eager step with the changed simulator - the graph holds
    pointers, not values."""
    from apg_trajectory_tracking_amd import functional as F
    lr, mom, H = 1e-4, 0.9, 10
    w = ref.seeded_weights(H)
    s0 = torch.as_tensor(cpu.case("seeded", B, H, .05)).to(dev)
    dyn = cpu.simulator("seeded").to(dev)

    def fresh():
        net = network(w, dev)
        return net, {k: torch.zeros_like(v) for k, v in net.named_parameters()}

    def reset(net, bufs, start):
        with torch.no_grad():
            for k, v in net.named_parameters():
                v.copy_(start[k])
                bufs[k].zero_()
    call = lambda net, bufs: F.cartpole_learnt_policy_train_step(
        net, dyn, s0, s0, .05, update=(lr, mom, bufs))
    eager_net, eager_bufs = fresh()
    for _ in range(3):
        eager = call(eager_net, eager_bufs)
    net, bufs = fresh()
    start = {k: v.detach().clone() for k, v in net.named_parameters()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                  # (the allocator's warm-up)
        call(net, bufs)
    torch.cuda.current_stream().wait_stream(side)
    reset(net, bufs, start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = call(net, bufs)
    torch.cuda.synchronize()
    for k, v in net.named_parameters():            # capturing ran nothing
        assert torch.equal(v.detach(), start[k]), k
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(res["loss"], eager["loss"]) and float(res["loss"]) > 0
    assert torch.equal(res["flat"][:-1], eager["flat"][:-1])
    for (k, v), e in zip(net.named_parameters(), eager_net.parameters()):
        assert torch.equal(v.detach(), e.detach()), k
        assert torch.equal(bufs[k], eager_bufs[k]), k
        assert not torch.equal(v.detach(), start[k]), k
    # 7: the simulator changes under the graph
    reset(net, bufs, start)
    graph.replay()
    torch.cuda.synchronize()
    old = res["loss"].clone(), res["flat"][:-1].clone()
    with torch.no_grad():
        dyn.cfg["length"].mul_(1.1)
        dyn.linear_state_2.weight.mul_(1.5)
    reset(net, bufs, start)
    graph.replay()
    torch.cuda.synchronize()
    reset(eager_net, eager_bufs, start)
    eager = call(eager_net, eager_bufs)
    assert torch.equal(res["loss"], eager["loss"])
    assert torch.equal(res["flat"][:-1], eager["flat"][:-1])
    for (k, v), e in zip(net.named_parameters(), eager_net.parameters()):
        assert torch.equal(v.detach(), e.detach()), k
    assert not torch.equal(res["loss"], old[0]) and not torch.equal(res["flat"][:-1], old[1])


# -------------------------------------------------------------- 8: non-finite
@pytest.mark.parametrize("B", [8, 321])
def test_a_non_finite_start_state_gives_non_finite_loss_and_gradients(dev, B):
    H = 10
    net = network(ref.seeded_weights(H), dev)
    dyn = cpu.simulator("fitted").to(dev)
    x = cpu.case("fitted", B, H, .05)
    s0 = x.copy()
    s0[B // 2, 2] = np.nan
    got = step(net, dyn, dev, x, s0, .05)
    assert not np.isfinite(got["loss"])
    for k, v in got["g"].items():
        assert not np.any(np.isfinite(v)), k
    assert np.all(np.isfinite(got["actions"]))      # (the policy saw finite inputs)


# ------------------------------------------------------------- 9: the trainer
def test_run_epoch_leaves_its_inputs_alone_and_steps_like_the_tape(dev, monkeypatch):
    """Two batches of 67 with in_state != state0, three epochs: the fused step
    (update inside the call) against the tape + optimizer.step()."""
    H, B = 10, 67
    w = ref.seeded_weights(H)
    mine, other = count_calls(monkeypatch)
    out = {}
    for fused in (True, False):
        labels = torch.as_tensor(cpu.case("seeded", 2 * B, H, .05)).to(dev)
        states = (labels * 0.5).contiguous()
        states[:, 0] = 3.0
        keep = states.clone(), labels.clone()
        dyn = cpu.simulator("seeded").to(dev)
        before, stamp = frozen_copy(dyn), dyn.timestamp
        t = trainer(dev, network(w, dev), dyn, states, labels, fused, B, H, lr=1e-6)
        assert t._fusable_learnt_policy(states[:B], labels[:B]) == fused
        assert not t._fusable_policy(states[:B], labels[:B])
        del mine[:], other[:]
        losses = [t.run_epoch("controller") for _ in range(3)]
        assert len(mine) == (6 if fused else 0) and not other
        assert all(c["update"] is not None for c in mine)
        assert torch.equal(states, keep[0]) and torch.equal(labels, keep[1])
        assert_untouched(dyn, before)
        assert dyn.timestamp == stamp          # as the fused rollout of the tape path
        out[fused] = (losses, {k: N(p.grad) for k, p in t.net.named_parameters()},
                      {k: N(v) for k, v in t.net.state_dict().items()})
    for a, b in zip(out[True][0], out[False][0]):
        assert abs(a - b) < BAR * abs(b), (a, b)
    worst_g = max((rel_err(out[True][1][k], v), k) for k, v in out[False][1].items())
    worst_w = max((rel_err(out[True][2][k], v), k) for k, v in out[False][2].items())
    print("three epochs fused vs tape: worst gradient %.3g (%s), worst weight %.3g (%s)"
          % (worst_g + worst_w))
    assert worst_g[0] < BAR and worst_w[0] < BAR_W


def test_step_hooks_leave_the_update_to_the_optimizer(dev, monkeypatch):
    H, B = 5, 8
    labels = torch.as_tensor(cpu.case("fitted", 2 * B, H, .05)).to(dev)
    mine, other = count_calls(monkeypatch)
    t = trainer(dev, network(ref.seeded_weights(H), dev), cpu.simulator("fitted").to(dev),
                labels.clone(), labels, True, B, H)
    seen = []
    t.optimizer_controller.register_step_post_hook(lambda *a, **k: seen.append(1))
    before = {k: v.clone() for k, v in t.net.state_dict().items()}
    t.run_epoch("controller")
    assert len(mine) == 2 and all(c["update"] is None for c in mine) and len(seen) == 2
    assert not other
    assert all(not torch.equal(v, before[k]) for k, v in t.net.state_dict().items())


def test_the_fused_step_is_taken_only_where_it_is_asked_for_and_applies(dev, monkeypatch):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.models.simple_model import Net

    class Other(Net):
        pass
    H, B = 10, 16
    w = ref.seeded_weights(H)
    mine, other = count_calls(monkeypatch)
    labels = torch.as_tensor(cpu.case("seeded", 2 * B, H, .05)).to(dev)
    for fused, cls in ((False, None), (True, Other)):
        t = trainer(dev, network(w, dev, cls), cpu.simulator("seeded").to(dev), labels.clone(),
                    labels, fused, B, H)
        assert not t._fusable_learnt_policy(labels[:B], labels[:B])
        t.run_epoch("controller")
    assert not mine and not other
    # an analytic simulator is not this step's either; nor are other inputs
    t = trainer(dev, network(w, dev), CartpoleDynamics(), labels.clone(), labels, True, B, H)
    assert not t._fusable_learnt_policy(labels[:B], labels[:B])
    t = trainer(dev, network(w, dev), cpu.simulator("seeded").to(dev), labels.clone(), labels,
                True, B, H)
    assert t._fusable_learnt_policy(labels[:B], labels[:B])
    assert not t._fusable_learnt_policy(labels[:B].double(), labels[:B])
    assert not t._fusable_learnt_policy(labels[:B].cpu(), labels[:B])
    assert not t._fusable_learnt_policy(labels[:B, :3], labels[:B])
    t.action_dim = 2
    assert not t._fusable_learnt_policy(labels[:B], labels[:B])


# ------------------------------------------------- 10: train_norm_dynamics
def test_train_norm_dynamics_with_the_fused_step_end_to_end(dev, monkeypatch, tmp_path):
    """One dynamics epoch and one controller epoch on 256 synthetic samples:
    the controller epoch goes through the new call, and both the controller's
    and the simulator's weights have moved."""
    from apg_trajectory_tracking_amd import train_cartpole as tc
    from apg_trajectory_tracking_amd.models.simple_model import Net
    monkeypatch.chdir(tmp_path)
    mine, other = count_calls(monkeypatch)
    seen = {}
    real_init = tc.TrainCartpole.initialize_model

    def init(self, base_model=None, **kw):
        torch.manual_seed(3)
        net = Net(4, 10)
        seen["net0"] = {k: v.detach().clone().to(dev) for k, v in net.state_dict().items()}
        real_init(self, base_model=net, **kw)
        seen["dyn0"] = frozen_copy(self.train_dynamics)
    monkeypatch.setattr(tc.TrainCartpole, "initialize_model", init)
    monkeypatch.setattr(tc.TrainCartpole, "evaluate_model", lambda self, epoch: (0.0, 0.0))
    monkeypatch.setattr(tc.TrainCartpole, "finalize", lambda self: None)
    cfg = dict(system="cartpole", delta_t=.05, state_size=4, batch_size=64, horizon=10,
               action_dim=1, ref_dim=4, train_mode="concurrent", nr_epochs=2,
               sample_data=256, learning_rate_controller=1e-6, learning_rate_dynamics=1e-3,
               l2_lambda=0, train_dyn_for_epochs=0, train_dyn_every=1, modified_params={},
               thresh_div_start=.2, thresh_div_end=.2, thresh_div_step=.05, resample_every=100,
               save_name=str(tmp_path / "cp"))
    t = tc.train_norm_dynamics(None, cfg, not_trainable=[], device=dev,
                               fused_learnt_policy=True)
    assert t.fused_learnt_policy is True
    assert t.results_dict["trained"] == ["dynamics", "controller"]
    assert len(mine) == 4 and not other            # 256 samples in batches of 64
    assert all(not torch.equal(v, seen["net0"][k]) for k, v in t.net.state_dict().items())
    moved = [k for k, v in t.train_dynamics.state_dict().items()
             if not torch.equal(v, seen["dyn0"][k])]
    print("simulator tensors that moved in the dynamics epoch:", moved)
    assert {"linear_state_1.weight", "linear_state_2.weight", "cfg.length"} <= set(moved)
