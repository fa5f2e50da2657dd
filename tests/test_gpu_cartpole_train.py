"""The fused controller step of the cart-pole on the GPU
(apg_cartpole_mlp_train_step through functional.cartpole_policy_train_step and
TrainCartpole.run_epoch): the recording of the real reference step (G6), the
host twin of test_cartpole_train_cpu.py at every shape that takes another path
through the kernels, run-to-run determinism, the in-kernel momentum SGD, a graph
capture of the whole step, non-finite inputs, and the trainer's choice between
the fused step and the tape.  Bounds: conftest.rel_err < 1e-4 on every gradient
tensor and the loss, 1e-5 on post-step weights, fused against unfused gradients
2e-5, the update against its formula at rtol 1e-6 (test_gpu_in_sweep.py).  Every
test prints what it saw."""
import numpy as np
import pytest
import torch

import test_cartpole_train_cpu as ref
from conftest import load_golden, rel_err
from test_cartpole_train_cpu import tw  # noqa: F401  (the host twin, a fixture)

pytestmark = pytest.mark.gpu
BAR, BAR_W = ref.BAR, ref.BAR_W
# The first kernel runs min(ceil(B / 64), 256) workgroups, one row each, and the
# second stage's threads add rows r, r + 8, ...: 1 221 samples are 20 rows (two or
# three rows per thread); 16 451 samples are 258 chunks on 256 workgroups (two of
# them take a second chunk) and 32 rows per thread.
B_ROWS, B_CHUNKS = 1221, 16451


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


def step(net, dev, in_state, state0, dt, **kw):
    """functional.cartpole_policy_train_step, results as the twin's."""
    from apg_trajectory_tracking_amd import functional as F
    to = lambda x: x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)).to(dev)
    res = F.cartpole_policy_train_step(net, to(in_state), to(state0), dt, ref.default_params(),
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


def trainer(dev, net, states, labels, fused, batch, H, dt=.05, lr=1e-4, train_dyn=None):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.train_cartpole import TrainCartpole
    cfg = dict(delta_t=dt, batch_size=batch, state_size=4, horizon=H, action_dim=1,
               ref_dim=4, train_mode="concurrent", learning_rate_controller=lr,
               learning_rate_dynamics=1e-3, l2_lambda=0, system="cartpole")
    t = TrainCartpole(train_dyn or CartpoleDynamics(), CartpoleDynamics(), cfg)

    class Data:
        num_sampled_states = states.shape[0]
    Data.states, Data.labels = states, labels
    t.initialize_model(base_model=net, state_data=Data, device=dev)
    t.shuffle = False
    t.init_optimizer()
    t.fused_policy = fused
    return t


def count_calls(monkeypatch):
    from apg_trajectory_tracking_amd import functional as F
    calls, real = [], F.cartpole_policy_train_step
    monkeypatch.setattr(F, "cartpole_policy_train_step",
                        lambda *p, **kw: calls.append(kw) or real(*p, **kw))
    return calls


# ---------------------------------------------------------------- 1: golden
def test_golden_through_the_functional_call(dev):
    g = load_golden("cartpole.npz")
    w, dt = ref.golden_weights(g, "w0."), float(g["dt"])
    got = step(network(w, dev), dev, g["state0"], g["state0"], dt)
    e_a = rel_err(got["actions"], g["train_actions"])
    e_l = abs(got["loss"] - float(g["train_loss"])) / float(g["train_loss"])
    errs = {k: rel_err(got["g"][k], g["g1." + k]) for k in ref.names()}
    print(f"gpu G6 actions {e_a:.2e} loss {e_l:.2e} worst gradient {max(errs.values()):.2e}")
    assert e_a < BAR and e_l < BAR
    for k, e in errs.items():
        assert e < BAR, (k, e)


def test_golden_through_run_epoch_fused_and_unfused(dev, monkeypatch):
    g = load_golden("cartpole.npz")
    w, dt = ref.golden_weights(g, "w0."), float(g["dt"])
    calls = count_calls(monkeypatch)
    out = {}
    for fused in (True, False):
        states = torch.as_tensor(g["state0"]).to(dev)
        labels = states.clone()
        t = trainer(dev, network(w, dev), states, labels, fused, 64, 5, dt)
        del calls[:]
        with pytest.raises(ZeroDivisionError):     # single batch: running_loss / 0
            t.run_epoch("controller")
        assert len(calls) == (1 if fused else 0)
        if fused:                                   # one process, plain momentum SGD
            assert calls[0]["update"] is not None
        # in_state and the data set's tensors are as they were
        assert torch.equal(states, labels) and np.array_equal(N(states), g["state0"])
        out[fused] = {k: N(p.grad) for k, p in t.net.named_parameters()}
        for k, p in t.net.named_parameters():
            assert rel_err(N(p.grad), g["g1." + k]) < BAR, (fused, k)
        for k, v in t.net.state_dict().items():
            assert rel_err(N(v), g["w1." + k]) < BAR_W, (fused, k)
    worst = max((rel_err(out[True][k], v), k) for k, v in out[False].items())
    print("G6 run_epoch fused vs unfused gradients: worst %.3g (%s)" % worst)
    assert worst[0] < 2e-5


# ------------------------------------------------------------ 2: the host twin
@pytest.mark.parametrize("B,H,dt", ref.SHAPES + [(B_ROWS, 10, .05), (B_CHUNKS, 5, .05)])
def test_against_the_host_twin(dev, tw, B, H, dt):  # noqa: F811
    """The same per-sample header on both sides: what differs is the order of
    the sums over the batch, the device's tanh / sin / cos and fma contraction."""
    s0 = ref.case(B, H, dt)
    x = s0 if B != 321 else ref.case(B + 1, H, dt)[:B]      # in_state != state0 once
    w = ref.seeded_weights(H)
    want = ref.twin_step(tw, w, x, s0, dt)
    got = step(network(w, dev), dev, x, s0, dt)
    errs = {"loss": abs(got["loss"] - want["loss"]) / abs(want["loss"]),
            "actions": rel_err(got["actions"], want["actions"]),
            "flat": rel_err(got["flat"], want["flat"][:-1])}
    errs.update((k, rel_err(got["g"][k], want["g"][k])) for k in ref.names())
    print(f"gpu vs twin B={B} H={H} dt={dt}", {k: float("%.3g" % v) for k, v in errs.items()})
    assert np.all(np.isfinite(got["flat"]))
    for k, v in errs.items():
        assert v < BAR, (k, v)


# ------------------------------------------------------------- 3: determinism
@pytest.mark.parametrize("B", [64, B_ROWS])
def test_two_calls_give_the_same_bits(dev, B):
    net = network(ref.seeded_weights(10), dev)
    s0 = ref.case(B, 10, .05)
    a, b = (step(net, dev, s0, s0, .05) for _ in range(2))
    assert a["raw"]["flat"].data_ptr() != b["raw"]["flat"].data_ptr()
    assert np.array_equal(a["flat"], b["flat"]) and a["loss"] == b["loss"]
    assert np.array_equal(a["actions"], b["actions"])
    assert np.any(a["flat"] != 0) and a["loss"] > 0


# ------------------------------------------------------------------ 4: update
@pytest.mark.parametrize("B", [8, 321])
def test_in_kernel_momentum_sgd_over_two_steps(dev, B):
    """One launch (B = 8) and with the second stage (B = 321)."""
    lr, mom, H = 1e-4, 0.9, 10
    net = network(ref.seeded_weights(H), dev)
    s0 = torch.as_tensor(ref.case(B, H, .05)).to(dev)
    params = dict(net.named_parameters())
    start = {k: p.detach().clone() for k, p in params.items()}
    bufs = {k: torch.zeros_like(p) for k, p in params.items()}
    want_p = {k: v.clone() for k, v in start.items()}
    want_m = {k: torch.zeros_like(v) for k, v in start.items()}
    for it in range(2):
        plain = step(net, dev, s0, s0, .05)
        versions = [p._version for p in params.values()]
        for k in want_p:
            # the formula as the rule states it: in double, rounded once each.
            # (In float32 the reference itself is off by an ulp of lr * buf, and
            # this loss has gradients of 1e3: where p - lr * buf cancels, that
            # ulp is above the 1e-9 the parameters are held to.)
            g = torch.as_tensor(plain["g"][k]).to(dev)
            want_m[k] = (mom * want_m[k].double() + g.double()).float()
            want_p[k] = (want_p[k].double() - lr * want_m[k].double()).float()
        got = step(net, dev, s0, s0, .05, update=(lr, mom, bufs))
        assert got["loss"] == plain["loss"]
        assert all(p._version > v for p, v in zip(params.values(), versions))
        for k, p in params.items():
            assert np.array_equal(got["g"][k], plain["g"][k]), k     # gradients all the same
            m, wm, wp = bufs[k], want_m[k], want_p[k]
            assert torch.allclose(m, wm, rtol=1e-6, atol=1e-6 * float(wm.abs().max())), k
            assert torch.allclose(p.detach(), wp, rtol=1e-6, atol=1e-9), k
            assert not torch.equal(p.detach(), wp + lr * wm), k      # it moved
    assert all(not torch.equal(p.detach(), start[k]) for k, p in params.items())


# ------------------------------------------------------------------- 5: graph
@pytest.mark.parametrize("B", [64, 321])
def test_the_whole_step_with_its_update_is_capturable(dev, B):
    """Three replays of the captured step = three eager steps from the same
    start, bit for bit: parameters, momentum buffers, gradients, loss."""
    from apg_trajectory_tracking_amd import functional as F
    lr, mom, H = 1e-4, 0.9, 10
    w = ref.seeded_weights(H)
    s0 = torch.as_tensor(ref.case(B, H, .05)).to(dev)
    p = ref.default_params()

    def fresh():
        net = network(w, dev)
        return net, {k: torch.zeros_like(v) for k, v in net.named_parameters()}
    eager_net, eager_bufs = fresh()
    for _ in range(3):
        eager = F.cartpole_policy_train_step(eager_net, s0, s0, .05, p,
                                             update=(lr, mom, eager_bufs))
    net, bufs = fresh()
    start = {k: v.detach().clone() for k, v in net.named_parameters()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                  # (the allocator's warm-up)
        F.cartpole_policy_train_step(net, s0, s0, .05, p, update=(lr, mom, bufs))
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for k, v in net.named_parameters():
            v.copy_(start[k])
            bufs[k].zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = F.cartpole_policy_train_step(net, s0, s0, .05, p, update=(lr, mom, bufs))
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


# -------------------------------------------------------------- 6: non-finite
@pytest.mark.parametrize("B", [8, 321])
def test_a_non_finite_start_state_gives_non_finite_loss_and_gradients(dev, B):
    H = 10
    net = network(ref.seeded_weights(H), dev)
    x = ref.case(B, H, .05)
    s0 = x.copy()
    s0[B // 2, 2] = np.nan
    got = step(net, dev, x, s0, .05)
    assert not np.isfinite(got["loss"])
    for k, v in got["g"].items():
        assert not np.any(np.isfinite(v)), k
    assert np.all(np.isfinite(got["actions"]))      # (the policy saw finite inputs)


# -------------------------------------------------------- 7, 8: the trainer
def test_run_epoch_leaves_its_inputs_alone_and_steps_like_the_tape(dev, monkeypatch):
    """Two batches of 67 with in_state != state0, three epochs: the fused step
    (update inside the call) against the tape + optimizer.step()."""
    H, B = 10, 67
    w = ref.seeded_weights(H)
    calls = count_calls(monkeypatch)
    out = {}
    for fused in (True, False):
        labels = torch.as_tensor(ref.case(2 * B, H, .05)).to(dev)
        states = (labels * 0.5).contiguous()
        states[:, 0] = 3.0
        keep = states.clone(), labels.clone()
        t = trainer(dev, network(w, dev), states, labels, fused, B, H, lr=1e-6)
        assert t._fusable_policy(states[:B], labels[:B]) == fused
        del calls[:]
        losses = [t.run_epoch("controller") for _ in range(3)]
        assert len(calls) == (6 if fused else 0)
        assert all(c["update"] is not None for c in calls)
        assert torch.equal(states, keep[0]) and torch.equal(labels, keep[1])
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
    labels = torch.as_tensor(ref.case(2 * B, H, .05)).to(dev)
    calls = count_calls(monkeypatch)
    t = trainer(dev, network(ref.seeded_weights(H), dev), labels.clone(), labels, True, B, H)
    seen = []
    t.optimizer_controller.register_step_post_hook(lambda *a, **k: seen.append(1))
    before = {k: v.clone() for k, v in t.net.state_dict().items()}
    t.run_epoch("controller")
    assert len(calls) == 2 and all(c["update"] is None for c in calls) and len(seen) == 2
    assert all(not torch.equal(v, before[k]) for k, v in t.net.state_dict().items())


def test_fused_policy_is_refused_where_it_does_not_apply(dev, monkeypatch):
    """A policy that is not the stock class and a learnt simulator take the tape
    whatever the flag says, and give what `fused_policy = False` gives, bit for
    bit."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    from apg_trajectory_tracking_amd.models.simple_model import Net

    class Other(Net):
        pass
    H, B = 10, 16
    w = ref.seeded_weights(H)
    calls = count_calls(monkeypatch)
    assert F.cartpole_policy_fusable(network(w, dev), H)
    assert not F.cartpole_policy_fusable(network(w, dev, Other), H)
    assert not F.cartpole_policy_fusable(network(w, dev), H + 1)
    frozen = network(w, dev)
    frozen.fc2.bias.requires_grad_(False)
    assert not F.cartpole_policy_fusable(frozen, H)
    assert not F.cartpole_policy_fusable(network(w, dev).double(), H)
    with pytest.raises(ValueError):
        F.cartpole_policy_train_step(network(w, dev, Other), torch.zeros(2, 4, device=dev),
                                     torch.zeros(2, 4, device=dev), .05, ref.default_params())
    del calls[:]                  # (that one was this test's own)
    for kind in ("other policy", "learnt simulator"):
        out = {}
        for fused in (True, False):
            labels = torch.as_tensor(ref.case(2 * B, H, .05)).to(dev)
            dyn = None
            if kind == "learnt simulator":
                torch.manual_seed(5)
                dyn = LearntCartpoleDynamics().to(dev)
            net = network(w, dev, Other if kind == "other policy" else None)
            t = trainer(dev, net, labels.clone(), labels, fused, B, H, train_dyn=dyn)
            assert not t._fusable_policy(labels[:B], labels[:B])
            loss = t.run_epoch("controller")
            out[fused] = (loss, {k: N(v) for k, v in t.net.state_dict().items()})
        assert out[True][0] == out[False][0], kind
        for k, v in out[False][1].items():
            assert np.array_equal(out[True][1][k], v), (kind, k)
    assert not calls
    # ... and inputs the call does not take: another dtype, another device
    t = trainer(dev, network(w, dev), labels.clone(), labels, True, B, H)
    assert t._fusable_policy(labels[:B], labels[:B])
    assert not t._fusable_policy(labels[:B].double(), labels[:B])
    assert not t._fusable_policy(labels[:B].cpu(), labels[:B])
    assert not t._fusable_policy(labels[:B, :3], labels[:B])
    t.action_dim = 2
    assert not t._fusable_policy(labels[:B], labels[:B])
