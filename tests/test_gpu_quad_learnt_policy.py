"""The concurrent controller step through the learnt quadrotor simulator on the
device (functional.quad_learnt_concurrent_policy_grads ->
apg_quad_learnt_mlp_concurrent_train_step): against the float64 oracle of
tests/quad_learnt_policy_cases.py (whose conditions
tests/test_quad_learnt_policy_cpu.py holds), against the existing learnt rollout
kernel on the step's own actions, and through TrainDrone.

B in {1, 33, 257, 515}: one lane pair, a ragged second wave, a ragged second
workgroup, three workgroups' partials.  Bars: loss 1e-5, every parameter
gradient 1e-4 (conftest.rel_err) - those of tests/test_gpu_in_sweep.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import quad_learnt_policy_cases as pc
from conftest import assert_no_worse_than_fp32, per_trajectory_err, rel_err
from quad_loss_cases import DEFAULT, LEARNT_INIT, learnt_dt, oracle_rollout

pytestmark = pytest.mark.gpu
H = pc.H


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def fresh_net(dev):
    return copy.deepcopy(pc.policy()).to(dev)


def step(dev, which, B, ref_cols=9, net=None, dyn=None, **kw):
    from apg_trajectory_tracking_amd import functional as F
    net = net if net is not None else fresh_net(dev)
    dyn = dyn if dyn is not None else pc.module(pc.sim_weights(which), dev)
    _, b = pc.batch(which, B, dev, ref_cols)
    out = {}
    loss, gr, flat = F.quad_learnt_concurrent_policy_grads(
        net, dyn, b["normed"], b["state0"], b["in_ref"], b["ref"], learnt_dt(), out=out, **kw)
    torch.cuda.synchronize()
    return dict(loss=loss, grads=gr, flat=flat, out=out, net=net, dyn=dyn, batch=b)


def check_against(got_loss, got_grads, want, what):
    e_loss = abs(float(got_loss) - want["loss"]) / abs(want["loss"])
    e = {k: rel_err(N(got_grads[k]), want["grads"][k]) for k in want["grads"]}
    print(what, "loss %.2g" % e_loss, "worst gradient %.2g" % max(e.values()))
    assert e_loss < pc.LOSS_BAR, (what, e_loss)
    assert set(e) == set(got_grads)
    for k, v in e.items():
        assert v < pc.GRAD_BAR, (what, k, v)
    return e


# ------------------------------------------------------------ against float64
@pytest.mark.parametrize("B", pc.SIZES)
@pytest.mark.parametrize("ref_cols", [9, 6])
@pytest.mark.parametrize("which", pc.SIMS)
def test_against_the_float64_oracle(dev, which, ref_cols, B):
    from apg_trajectory_tracking_amd import functional as F
    r = step(dev, which, B, ref_cols)
    check_against(r["loss"], r["grads"], pc.oracle(which, B), f"{which} C{ref_cols} B{B}")
    # the flat buffer: the gradients in _MLP_PARAMS order, then the loss slot
    assert tuple(r["grads"]) == F._MLP_PARAMS
    at = 0
    for k, v in r["grads"].items():
        assert v.data_ptr() == r["flat"].data_ptr() + 4 * at and v.is_contiguous(), k
        at += v.numel()
    assert r["flat"].numel() == at + 1


# ---------------------------------------- against the existing learnt rollout
def own_actions(r):
    """The step's actions from the activation plane it left: sigmoid(W_out h3 +
    b_out), [B, H, 4] float32 (the product in float64)."""
    h3 = r["out"]["acts"][239 + 128:239 + 192].double()            # [64][B]
    z = r["net"].fc_out.weight.detach().double() @ h3 + r["net"].fc_out.bias.detach().double()[:, None]
    return torch.sigmoid(z).t().reshape(-1, H, 4).float().contiguous()


@pytest.mark.parametrize("which", pc.SIMS)
@pytest.mark.parametrize("B", [33, 515])
def test_against_the_learnt_rollout_kernel_on_the_same_actions(dev, which, B):
    from apg_trajectory_tracking_amd import functional as F, synthetic
    from oracle import torch_port as tp
    r = step(dev, which, B)
    a = own_actions(r)                                                  # [B,H,4]
    b = r["batch"]
    o = F.quad_learnt_rollout_fwd_bwd(
        r["dyn"], synthetic.to_soa_state(b["state0"]).contiguous(),
        synthetic.to_soa_seq(a).contiguous(), synthetic.to_soa_seq(b["ref"]).contiguous(),
        learnt_dt(), layout="soa", want_states=True)
    torch.cuda.synchronize()
    e = per_trajectory_err(N(r["out"]["states"].permute(2, 0, 1)), N(o["states"].permute(2, 0, 1)))
    print(which, B, "states vs the rollout kernel: worst %.2g" % e.max())
    assert e.max() < 1e-5
    # d_zout = dL/dactions . a (1 - a): no further from float64 than the rollout kernel
    ora = tp.LearntQuadOracle(pc.sim_weights(which), initial_params=dict(LEARNT_INIT),
                              dtype=torch.float64)
    w64 = oracle_rollout(ora, DEFAULT, b["state0"].cpu(), a.cpu(), b["ref"].cpu(), learnt_dt())
    a64 = N(a).astype(np.float64)
    d64 = (w64["grad_actions"] * a64 * (1 - a64)).reshape(B, -1)
    d32 = N(synthetic.from_soa_seq(o["grad_actions"]) * a * (1 - a)).reshape(B, -1)
    ddev = N(r["out"]["d_zout"]).T
    assert_no_worse_than_fp32(ddev, d32, d64, f"d_zout {which} B{B}")


# ------------------------------------------- determinism, frozen simulator, index
def test_two_runs_give_the_same_bits_and_the_simulator_is_left_alone(dev):
    dyn = pc.module(pc.sim_weights("steps"), dev)
    before = {k: v.detach().clone() for k, v in dyn.state_dict().items()}
    net = fresh_net(dev)
    a, b = (step(dev, "steps", 515, net=net, dyn=dyn) for _ in range(2))
    assert torch.equal(a["flat"][:-1], b["flat"][:-1]) and torch.equal(a["loss"], b["loss"])
    for k in ("d_zout", "states"):
        assert torch.equal(a["out"][k], b["out"][k]), k
    for k, v in dyn.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in dyn.parameters())


@pytest.mark.parametrize("B", [33, 257])
def test_index_form_equals_the_gathered_batch(dev, B):
    from apg_trajectory_tracking_amd import functional as F
    from oracle import torch_port as tp
    r = step(dev, "golden", B)
    d = pc.pool()
    rows, _ = pc.batch("golden", B)
    whole = [t.to(dev).contiguous() for t in (
        tp.quad_state_features(d["state0"]), d["state0"], d["in_ref"], d["ref"])]
    index = torch.as_tensor(rows, dtype=torch.int64, device=dev)
    loss, gr, flat = F.quad_learnt_concurrent_policy_grads(
        r["net"], r["dyn"], *whole, learnt_dt(), index=index)
    torch.cuda.synchronize()
    assert torch.equal(loss, r["loss"]) and torch.equal(flat[:-1], r["flat"][:-1])


# ----------------------------------------------------------------------- update
def momentum_buffers(net, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    named = dict(net.named_parameters())
    from apg_trajectory_tracking_amd import functional as F
    return {n: (0.1 * torch.randn(named[n].shape, generator=g)).to(dev) for n in F._MLP_PARAMS}


@pytest.mark.parametrize("B", [33, 515])
def test_update_is_momentum_sgd_from_the_returned_gradients(dev, B):
    lr, m = 1e-3, 0.9
    net = fresh_net(dev)
    bufs = momentum_buffers(net, dev)
    named = dict(net.named_parameters())
    p0 = {n: named[n].detach().clone() for n in bufs}
    b0 = {n: v.clone() for n, v in bufs.items()}
    versions = {n: named[n]._version for n in bufs}
    r = step(dev, "strong", B, net=net, update=(lr, m, bufs))
    want = pc.oracle("strong", B)
    check_against(r["loss"], r["grads"], want, f"update B{B}")
    for n in bufs:
        buf = m * b0[n].double() + r["grads"][n].double()
        torch.testing.assert_close(bufs[n].double(), buf, rtol=1e-6, atol=0)
        # (p -= lr buf with the buffer as it is STORED, float32, as torch.optim.SGD does)
        torch.testing.assert_close(named[n].detach().double(),
                                   p0[n].double() - lr * buf.float().double(),
                                   rtol=1e-6, atol=1e-9)
        # ... and the float64 step
        p64 = N(p0[n]).astype(np.float64) - lr * (m * N(b0[n]).astype(np.float64) + want["grads"][n])
        assert rel_err(N(named[n]), p64) < 1e-5, n
        assert named[n]._version > versions[n], n      # (note_in_kernel_update)


# ------------------------------------------------------------------------ graph
def test_captured_step_follows_the_simulators_tensors(dev):
    from apg_trajectory_tracking_amd import functional as F
    which, B, lr, m = "golden", 257, 1e-4, 0.9
    w0 = pc.sim_weights(which)
    w1 = {k: v.copy() for k, v in w0.items()}
    w1["linear_state_2.weight"] = w1["linear_state_2.weight"] * 3
    w1["linear_at"] = (w1["linear_at"] + pc.at_perturbation(seed=10)).astype(np.float32)
    # rows off a kink under both simulators
    rows = pc.batch_rows(which, B, also=(pc.oracle_run(w1, pc.policy(), range(pc.POOL))["kink"],))
    d = pc.pool()
    r_ = torch.as_tensor(rows, dtype=torch.long)
    from oracle import torch_port as tp
    s0 = d["state0"][r_]
    ins = [t.contiguous().to(dev) for t in (tp.quad_state_features(s0), s0, d["in_ref"][r_],
                                            d["ref"][r_])]
    net, dyn = fresh_net(dev), pc.module(w0, dev)
    bufs = {n: torch.zeros_like(p) for n, p in net.named_parameters() if n in F._MLP_PARAMS}
    call = lambda upd: F.quad_learnt_concurrent_policy_grads(net, dyn, *ins, learnt_dt(),
                                                             update=upd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(None)                               # warm-up: attributes, input guard
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, gr, flat = call((lr, m, bufs))
    host_net = lambda: copy.deepcopy(net).cpu()
    n0 = host_net()
    graph.replay()
    torch.cuda.synchronize()
    check_against(loss, gr, pc.oracle_run(w0, n0, rows), "graph, first replay")
    for n, p in net.named_parameters():
        if n in bufs:     # one momentum step from zero buffers
            assert rel_err(N(p), N(dict(n0.named_parameters())[n]) - lr * N(gr[n])) < 1e-6, n
    # the simulator changes IN PLACE: the replayed launches read the new tensors
    with torch.no_grad():
        dyn.linear_state_2.weight.mul_(3)
        dyn.linear_at.copy_(torch.from_numpy(w1["linear_at"]))
    n1 = host_net()
    graph.replay()
    torch.cuda.synchronize()
    fresh = pc.oracle_run(w1, n1, rows)
    check_against(loss, gr, fresh, "graph, second replay")
    stale = pc.oracle_run(w0, n1, rows)
    e = pc.moved(stale["grads"], fresh["grads"])
    print("the simulator change moves the gradients by >= %.3g" % min(e.values()))
    assert min(e.values()) > 1e-2, e


# --------------------------------------------------------------------- canaries
def test_nothing_is_written_behind_an_output_buffer(dev):
    from apg_trajectory_tracking_amd import _capi, functional as F
    B, pad, mark = 33, 64, -7.25
    lib = _capi.lib()
    _, b = pc.batch("steps", B, dev)
    net, dyn = fresh_net(dev), pc.module(pc.sim_weights("steps"), dev)
    sizes = dict(acts=521 * B, relu_mask=5 * B, d_zout=40 * B,
                 loss_partials=max(1, lib.apg_quad_mlp_loss_partials_count(B)), loss=1,
                 flat=sum(int(np.prod(s)) for s in F._QUAD_POLICY_SHAPES.values()),
                 states=H * 12 * B, workspace=lib.apg_quad_learnt_mlp_step_workspace_floats(),
                 partials=lib.apg_quad_mlp_step_partials_floats(B), s0=12 * B, rf=H * 9 * B)
    bufs = {k: torch.full((n + pad,), mark, dtype=torch.float32, device=dev)
            for k, n in sizes.items()}
    view = lambda k, *shape: bufs[k][:sizes[k]].view(*shape)
    acts, s0, rf = F.quad_concurrent_prepare(
        b["normed"], b["state0"], b["in_ref"], b["ref"],
        out=(view("acts", 521, B), view("s0", 12, B), view("rf", H, 9, B)))
    params = F._net_params(net, F._MLP_PARAMS)
    pol = _capi.ApgMlpPolicy(*[p.data_ptr() for p in params])
    at, ptrs = 0, []
    for s in F._QUAD_POLICY_SHAPES.values():
        ptrs.append(bufs["flat"].data_ptr() + 4 * at)
        at += int(np.prod(s))
    grads = _capi.ApgMlpPolicyGrads(*ptrs)
    model = F._learnt_model(dyn)
    weights = F.quad_loss_weights()
    p = lambda k: bufs[k].data_ptr()
    rc = lib.apg_quad_learnt_mlp_concurrent_train_step(
        s0.data_ptr(), rf.data_ptr(), 9, learnt_dt(), ctypes.byref(dyn.params),
        ctypes.byref(model), ctypes.byref(weights), ctypes.byref(pol), B, H, p("acts"),
        p("relu_mask"), p("d_zout"), p("loss_partials"), p("loss"), ctypes.byref(grads),
        p("states"), p("workspace"), p("partials"), None,
        torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.apg_last_error_string()
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert bool((bufs[k][n:] == mark).all()), k
    # (and the call did what the functional does)
    want = pc.oracle("steps", B)
    got = {n: bufs["flat"][:sizes["flat"]].split(
        [int(np.prod(s)) for s in F._QUAD_POLICY_SHAPES.values()])[i].view(s)
        for i, (n, s) in enumerate(F._QUAD_POLICY_SHAPES.items())}
    check_against(bufs["loss"][0], got, want, "direct call")


# ---------------------------------------------------------------------- trainer
def make_trainer(dev, fused, data, lr=1e-3):
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import FlightmareDynamics
    from apg_trajectory_tracking_amd.train_drone import TrainDrone
    cfg = dict(delta_t=learnt_dt(), delta_t_train=learnt_dt(), epoch_size=33, self_play=0,
               batch_size=33, state_size=12, horizon=10, train_mode="concurrent", ref_dim=9,
               action_dim=4, learning_rate_controller=lr, learning_rate_dynamics=1e-4,
               system="quad", modified_params={})
    t = TrainDrone(pc.module(pc.sim_weights("steps"), dev), FlightmareDynamics(), cfg)

    class Data:
        num_sampled_states = 33
    Data.normed_states, Data.states = data["normed"], data["state0"]
    Data.in_ref_states, Data.ref_states = data["in_ref"], data["ref"]
    t.state_data = Data
    t.net = fresh_net(dev)
    t.shuffle = False
    t.init_optimizer()
    t.fused_learnt_policy = fused
    return t


def test_trainer_runs_the_fused_step_and_matches_the_tape(dev, monkeypatch):
    from apg_trajectory_tracking_amd import functional as F
    _, data = pc.batch("steps", 33, dev)
    calls, tape = [], []
    real = F.quad_learnt_concurrent_policy_grads

    def counted(*a, **kw):
        res = real(*a, **kw)
        calls.append((float(res[0]), kw.get("update")))
        return res
    monkeypatch.setattr(F, "quad_learnt_concurrent_policy_grads", counted)
    direct = float(step(dev, "steps", 33)["loss"])

    t = make_trainer(dev, True, data)
    with pytest.raises(ZeroDivisionError):        # a single batch: running_loss / 0
        t.run_epoch("controller")
    assert len(calls) == 2 and calls[1][0] == direct          # (calls[0]: `direct` itself)
    assert calls[1][1] is not None                             # one process: in-kernel update
    assert t.last_epoch_loop == "loader"      # (the loops that probe first stay out)

    u = make_trainer(dev, False, data)
    real_tape = u.train_controller_model
    u.train_controller_model = lambda *a, **kw: tape.append(real_tape(*a, **kw)) or tape[-1]
    with pytest.raises(ZeroDivisionError):
        u.run_epoch("controller")
    assert len(calls) == 2 and len(tape) == 1
    l_tape = float(tape[0].detach())
    print("trainer: fused %.9g tape %.9g" % (calls[1][0], l_tape))
    assert abs(calls[1][0] - l_tape) <= 1e-4 * abs(l_tape)
    before = dict(pc.policy().named_parameters())
    for (k, a), (_, b) in zip(t.net.named_parameters(), u.net.named_parameters()):
        assert rel_err(N(a), N(b)) < 1e-5, k
        if k in F._MLP_PARAMS:
            assert not np.array_equal(N(a), N(before[k])), k   # the step moved them
