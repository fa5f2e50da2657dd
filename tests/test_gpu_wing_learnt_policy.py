"""The concurrent controller step through the learnt fixed-wing simulator on the
device (functional.wing_learnt_concurrent_policy_grads ->
apg_wing_learnt_mlp_train_step): against the float64 oracle of
tests/wing_learnt_policy_cases.py (whose conditions
tests/test_wing_learnt_policy_cpu.py holds), against the existing learnt rollout
kernel on the step's own actions, and through TrainFixedWing.

B in {1, 33, 257, 515}: one lane pair, a ragged second wave, a ragged second
workgroup, three workgroups' partials.  Bars: loss 1e-5, every parameter
gradient 1e-4 (conftest.rel_err) - those of tests/test_gpu_in_sweep.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import wing_learnt_policy_cases as pc
from conftest import rel_err

pytestmark = pytest.mark.gpu
H, DT = pc.H, pc.DT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def fresh_net(dev):
    return copy.deepcopy(pc.policy()).to(dev)


def step(dev, which, B, net=None, dyn=None, **kw):
    from apg_trajectory_tracking_amd import functional as F
    net = net if net is not None else fresh_net(dev)
    dyn = dyn if dyn is not None else pc.module(pc.sim_weights(which), dev)
    _, b = pc.batch(which, B, dev)
    out = {}
    loss, gr, flat = F.wing_learnt_concurrent_policy_grads(
        net, dyn, b["normed"], b["in_ref"], b["state0"], b["ref"], DT, out=out, **kw)
    torch.cuda.synchronize()
    return dict(loss=loss, grads=gr, flat=flat, out=out, net=net, dyn=dyn, batch=b)


def check_against(got_loss, got_grads, want, what):
    e_loss = abs(float(got_loss) - want["loss"]) / abs(want["loss"])
    e = {k: rel_err(N(got_grads[k]), want["grads"][k]) for k in want["grads"]}
    print(what, "loss %.2g" % e_loss, "worst gradient %.2g" % max(e.values()))
    assert e_loss < pc.LOSS_BAR, (what, e_loss)
    assert set(e) == set(got_grads) == set(pc.NAMES)
    for k, v in e.items():
        assert v < pc.GRAD_BAR, (what, k, v)
    return e


# ------------------------------------------------------------ against float64
@pytest.mark.parametrize("B", pc.SIZES)
@pytest.mark.parametrize("which", pc.SIMS)
def test_against_the_float64_oracle(dev, which, B):
    from apg_trajectory_tracking_amd import _capi, functional as F
    r = step(dev, which, B)
    check_against(r["loss"], r["grads"], pc.oracle(which, B), f"{which} B{B}")
    # the flat buffer: the gradients in _WING_PARAMS order at the published
    # offsets, then the loss slot
    assert tuple(r["grads"]) == F._WING_PARAMS
    at = [(v.data_ptr() - r["flat"].data_ptr()) // 4 for v in r["grads"].values()]
    assert tuple(at) == _capi.WING_POLICY_G
    assert all(v.is_contiguous() for v in r["grads"].values())
    assert r["flat"].numel() == _capi.WING_POLICY_GRADS + 1


def test_the_predicate_holds_the_shapes_on_the_device(dev):
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    from apg_trajectory_tracking_amd.models.hutter_model import Net
    dyn = pc.module(pc.sim_weights("w"), dev)
    assert F.wing_learnt_policy_fusable(fresh_net(dev), dyn)
    assert not F.wing_learnt_policy_fusable(Net(9, 1, 3, 44, conv=False).to(dev), dyn)
    assert not F.wing_learnt_policy_fusable(Net(9, 1, 3, 80, conv=False).to(dev), dyn)
    assert not F.wing_learnt_policy_fusable(pc.policy(), dyn)              # host policy
    assert not F.wing_learnt_policy_fusable(fresh_net(dev).double(), dyn)
    assert not F.wing_learnt_policy_fusable(fresh_net(dev), FixedWingDynamics())


# ---------------------------------------- against the existing learnt rollout
@pytest.mark.parametrize("which", pc.SIMS)
@pytest.mark.parametrize("B", [33, 515])
def test_against_the_learnt_rollout_kernel_on_the_same_actions(dev, which, B):
    """Physics, residual and loss pinned to a kernel the goldens already pin:
    grad_actions planes, states and loss on the step's OWN actions; the
    project's parity bar, rel_err < 1e-4."""
    from apg_trajectory_tracking_amd import functional as F, synthetic
    r = step(dev, which, B)
    acts = r["out"]["acts"]
    a = acts[332:372].reshape(H, 4, B).contiguous()                     # [H][4][B]
    b = r["batch"]
    o = F.wing_learnt_rollout_fwd_bwd(
        r["dyn"], synthetic.to_soa_state(b["state0"]), a, synthetic.to_soa_seq(b["ref"]), DT,
        layout="soa", want_states=True, want_grad_state0=False)
    torch.cuda.synchronize()
    # (the actions are the policy's: sigmoid(W_out h3 + b_out) of the saved plane)
    h3 = acts[268:332].double()
    z = r["net"].fc_out.weight.detach().double() @ h3 + r["net"].fc_out.bias.detach().double()[:, None]
    assert rel_err(N(acts[332:372]), N(torch.sigmoid(z))) < 1e-5
    e_s = rel_err(N(r["out"]["states"]), N(o["states"]))
    e_g = rel_err(N(acts[372:412]).reshape(H, 4, B), N(o["grad_actions"]))
    e_l = abs(float(r["loss"]) - float(o["loss"])) / abs(float(o["loss"]))
    print(which, B, "vs the rollout kernel: states %.2g grad_actions %.2g loss %.2g"
          % (e_s, e_g, e_l))
    assert e_s < 1e-4 and e_g < 1e-4 and e_l < 1e-4


# ------------------------------------------- determinism, frozen simulator, index
def test_two_runs_give_the_same_bits_and_the_simulator_is_left_alone(dev):
    dyn = pc.module(pc.sim_weights("steps"), dev)
    before = {k: v.detach().clone() for k, v in dyn.state_dict().items()}
    net = fresh_net(dev)
    a, b = (step(dev, "steps", 515, net=net, dyn=dyn) for _ in range(2))
    assert torch.equal(a["flat"][:-1], b["flat"][:-1]) and torch.equal(a["loss"], b["loss"])
    for k in ("acts", "cot", "states"):
        assert torch.equal(a["out"][k], b["out"][k]), k
    for k, v in dyn.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in dyn.parameters())


@pytest.mark.parametrize("B", [33, 257])
def test_index_form_equals_the_gathered_batch(dev, B):
    from apg_trajectory_tracking_amd import functional as F
    r = step(dev, "w", B)
    d = pc.pool()
    rows, _ = pc.batch("w", B)
    whole = [d[k].to(dev).contiguous() for k in ("normed", "in_ref", "state0", "ref")]
    index = torch.as_tensor(rows, dtype=torch.int64, device=dev)
    loss, gr, flat = F.wing_learnt_concurrent_policy_grads(
        r["net"], r["dyn"], *whole, DT, index=index)
    torch.cuda.synchronize()
    assert torch.equal(loss, r["loss"]) and torch.equal(flat[:-1], r["flat"][:-1])


@pytest.mark.parametrize("B", [9362, 9363])
def test_both_sides_of_the_products_launch_threshold(dev, B):
    """7 B <= 65 536 columns: the weight products share one launch pair, beyond
    that each gets its own launch.  The batch is the 515-row batch eighteen
    times over plus its first rows (through `index`), so the float64 answer is
    18 x the oracle's of 515 rows + the oracle's of the rest."""
    from apg_trajectory_tracking_amd import functional as F
    reps, rest = divmod(B, 515)
    rows515 = pc.batch_rows("steps", 515)
    rows = np.concatenate([np.tile(rows515, reps), rows515[:rest]])
    full, part = pc.oracle("steps", 515), pc.oracle("steps", rest)
    want = dict(loss=reps * full["loss"] + part["loss"],
                grads={k: reps * full["grads"][k] + part["grads"][k] for k in full["grads"]})
    d = pc.pool()
    whole = [d[k].to(dev).contiguous() for k in ("normed", "in_ref", "state0", "ref")]
    index = torch.as_tensor(rows, dtype=torch.int64, device=dev)
    loss, gr, _ = F.wing_learnt_concurrent_policy_grads(
        fresh_net(dev), pc.module(pc.sim_weights("steps"), dev), *whole, DT, index=index)
    torch.cuda.synchronize()
    check_against(loss, gr, want, f"threshold B{B}")


# ----------------------------------------------------------------------- update
def momentum_buffers(net, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    named = dict(net.named_parameters())
    return {n: (0.1 * torch.randn(named[n].shape, generator=g)).to(dev) for n in pc.NAMES}


@pytest.mark.parametrize("B", [33, 515])
def test_update_is_momentum_sgd_from_the_returned_gradients(dev, B):
    """Parameters and momentum buffers against momentum SGD in float64 from the
    gradients of a call WITHOUT the update; tolerances of
    tests/test_gpu_quad_learnt_policy.py."""
    lr, m = 1e-5, 0.9
    net = fresh_net(dev)
    plain = step(dev, "steps", B, net=net)
    g0 = {n: v.clone() for n, v in plain["grads"].items()}
    bufs = momentum_buffers(net, dev)
    named = dict(net.named_parameters())
    p0 = {n: named[n].detach().clone() for n in bufs}
    b0 = {n: v.clone() for n, v in bufs.items()}
    versions = {n: named[n]._version for n in bufs}
    r = step(dev, "steps", B, net=net, update=(lr, m, bufs))
    want = pc.oracle("steps", B)
    check_against(r["loss"], r["grads"], want, f"update B{B}")
    for n in bufs:
        assert torch.equal(r["grads"][n], g0[n]), n
        buf = m * b0[n].double() + g0[n].double()
        torch.testing.assert_close(bufs[n].double(), buf, rtol=1e-6, atol=0)
        # (p -= lr buf with the buffer as it is STORED, float32, as torch.optim.SGD does)
        torch.testing.assert_close(named[n].detach().double(),
                                   p0[n].double() - lr * buf.float().double(),
                                   rtol=1e-6, atol=1e-9)
        # ... and the float64 step
        p64 = N(p0[n]).astype(np.float64) - lr * (m * N(b0[n]).astype(np.float64) + want["grads"][n])
        assert rel_err(N(named[n]), p64) < 1e-5, n
        assert named[n]._version > versions[n], n      # (note_in_kernel_update)
    for n, p in net.named_parameters():                # (conv_ref: not part of this policy)
        if n not in bufs:
            assert torch.equal(p.detach().cpu(), dict(pc.policy().named_parameters())[n]), n


# ------------------------------------------------------------------------ graph
def changed_simulator(w0):
    w1 = {k: v.copy() for k, v in w0.items()}
    w1["linear_state_2.weight"] = w1["linear_state_2.weight"] * 3
    g = torch.Generator().manual_seed(10)
    w1["I"] = (w1["I"] * 1.3 + 2e-3 * torch.randn(3, 3, generator=g).numpy()).astype(np.float32)
    return w1


def test_captured_step_follows_the_simulators_tensors(dev):
    from apg_trajectory_tracking_amd import functional as F
    which, B, lr, m = "steps", 257, 1e-6, 0.9
    w0 = pc.sim_weights(which)
    w1 = changed_simulator(w0)
    # rows off a kink under both simulators
    rows = pc.batch_rows(which, B, also=(pc.oracle_run(w1, pc.policy(), range(pc.POOL))["kink"],))
    d = pc.pool()
    r_ = torch.as_tensor(rows, dtype=torch.long)
    ins = [d[k][r_].contiguous().to(dev) for k in ("normed", "in_ref", "state0", "ref")]
    net, dyn = fresh_net(dev), pc.module(w0, dev)
    bufs = {n: torch.zeros_like(p) for n, p in net.named_parameters() if n in pc.NAMES}
    call = lambda upd: F.wing_learnt_concurrent_policy_grads(net, dyn, *ins, DT, update=upd)
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
        dyn.I.copy_(torch.from_numpy(w1["I"]))
    n1 = host_net()
    graph.replay()
    torch.cuda.synchronize()
    fresh = pc.oracle_run(w1, n1, rows)
    check_against(loss, gr, fresh, "graph, second replay")
    # ... and equals a fresh eager call on the changed module
    eager_net = copy.deepcopy(n1).to(dev)
    l2, g2, _ = F.wing_learnt_concurrent_policy_grads(eager_net, dyn, *ins, DT)
    torch.cuda.synchronize()
    assert torch.equal(l2, loss)
    for n in pc.NAMES:
        assert torch.equal(g2[n], gr[n]), n
    stale = pc.oracle_run(w0, n1, rows)
    e = pc.moved(stale["grads"], fresh["grads"])
    print("the simulator change moves the gradients by >= %.3g" % min(e.values()))
    assert min(e.values()) > 1e-2, e


# --------------------------------------------------------------------- canaries
@pytest.mark.parametrize("B", [1, 257])
def test_nothing_is_written_behind_an_output_buffer(dev, B):
    from apg_trajectory_tracking_amd import _capi, functional as F
    pad, mark = 64, -7.25
    lib = _capi.lib()
    _, b = pc.batch("steps", B, dev)
    net, dyn = fresh_net(dev), pc.module(pc.sim_weights("steps"), dev)
    shapes = F._WING_POLICY_SHAPES
    sizes = dict(acts=412 * B, cot=360 * B, loss_partials=(B + 31) // 32, loss=1,
                 flat=_capi.WING_POLICY_GRADS, states=H * 12 * B,
                 workspace=lib.apg_wing_learnt_mlp_step_workspace_floats(B))
    bufs = {k: torch.full((n + pad,), mark, dtype=torch.float32, device=dev)
            for k, n in sizes.items()}
    acts = bufs["acts"][:412 * B].view(412, B)
    _, _, s0, rf = F.to_soa_multi([(b["normed"], acts[:9]), (b["in_ref"], acts[9:12]),
                                   (b["state0"], None), (b["ref"], None)])
    params = F._net_params(net, F._WING_PARAMS)
    pol = _capi.ApgWingPolicy(*[p.data_ptr() for p in params])
    grads = _capi.ApgWingPolicyGrads(*[bufs["flat"].data_ptr() + 4 * at
                                       for at in _capi.WING_POLICY_G])
    sim = F._wing_learnt_tensors(dyn)
    model = _capi.ApgWingLearnt(*[t.data_ptr() for t in sim])
    weights = F.wing_loss_weights()
    p = lambda k: bufs[k].data_ptr()
    rc = lib.apg_wing_learnt_mlp_train_step(
        p("acts"), p("acts") + 4 * 9 * B, s0.data_ptr(), rf.data_ptr(), DT, ctypes.byref(model),
        ctypes.byref(weights), ctypes.byref(pol), B, H, p("acts"), p("cot"),
        p("loss_partials"), p("loss"), ctypes.byref(grads), p("states"), p("workspace"), None,
        torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.apg_last_error_string()
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert bool((bufs[k][n:] == mark).all()), k
    for k in ("acts", "cot", "states", "flat", "loss_partials", "loss"):   # ... and filled
        assert not bool((bufs[k][:sizes[k]] == mark).any()), k
    # (and the call did what the functional does)
    got = {n: v.view(shapes[n]) for n, v in zip(shapes, bufs["flat"][:sizes["flat"]].split(
        [int(np.prod(s)) for s in shapes.values()]))}
    check_against(bufs["loss"][0], got, pc.oracle("steps", B), "direct call")


def test_an_empty_batch_gives_zero_gradients_and_zero_loss(dev):
    from apg_trajectory_tracking_amd import _capi, functional as F
    lib = _capi.lib()
    net, dyn = fresh_net(dev), pc.module(pc.sim_weights("w"), dev)
    flat = torch.full((_capi.WING_POLICY_GRADS + 8,), 3.0, device=dev)
    loss = torch.full((1,), 3.0, device=dev)
    pol = _capi.ApgWingPolicy(*[p.data_ptr() for p in F._net_params(net, F._WING_PARAMS)])
    grads = _capi.ApgWingPolicyGrads(*[flat.data_ptr() + 4 * at for at in _capi.WING_POLICY_G])
    model = _capi.ApgWingLearnt(*[t.data_ptr() for t in F._wing_learnt_tensors(dyn)])
    weights = F.wing_loss_weights()
    rc = lib.apg_wing_learnt_mlp_train_step(
        None, None, None, None, DT, ctypes.byref(model), ctypes.byref(weights),
        ctypes.byref(pol), 0, H, None, None, None, loss.data_ptr(), ctypes.byref(grads), None,
        None, None, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.apg_last_error_string()
    torch.cuda.synchronize()
    assert float(loss) == 0 and bool((flat[:_capi.WING_POLICY_GRADS] == 0).all())
    assert bool((flat[_capi.WING_POLICY_GRADS:] == 3.0).all())


# ---------------------------------------------------------------------- trainer
def make_trainer(dev, fused, data, lr):
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    from apg_trajectory_tracking_amd.train_fixed_wing import TrainFixedWing
    cfg = dict(delta_t=DT, delta_t_train=DT, epoch_size=33, self_play=0, batch_size=33,
               state_size=12, horizon=10, train_mode="concurrent", ref_dim=3, action_dim=4,
               learning_rate_controller=lr, learning_rate_dynamics=1e-4, system="wing",
               sample_in="train_env")
    t = TrainFixedWing(pc.module(pc.sim_weights("steps"), dev), FixedWingDynamics(), cfg)

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
    lr = 1e-5
    _, data = pc.batch("steps", 33, dev)
    calls, tape = [], []
    real = F.wing_learnt_concurrent_policy_grads

    def counted(*a, **kw):
        res = real(*a, **kw)
        calls.append((float(res[0]), kw.get("update")))
        return res
    monkeypatch.setattr(F, "wing_learnt_concurrent_policy_grads", counted)
    direct = float(step(dev, "steps", 33)["loss"])

    t = make_trainer(dev, True, data, lr)
    with pytest.raises(ZeroDivisionError):        # a single batch: running_loss / 0
        t.run_epoch("controller")
    assert len(calls) == 2 and calls[1][0] == direct          # (calls[0]: `direct` itself)
    assert calls[1][1] is not None                             # one process: in-kernel update
    assert t.last_epoch_loop == "loader"      # (the loops that probe first stay out)

    u = make_trainer(dev, False, data, lr)
    real_tape = u.train_controller_model
    u.train_controller_model = lambda *a, **kw: tape.append(real_tape(*a, **kw)) or tape[-1]
    with pytest.raises(ZeroDivisionError):
        u.run_epoch("controller")
    assert len(calls) == 2 and len(tape) == 1
    l_tape = float(tape[0].detach())
    print("trainer: fused %.9g tape %.9g" % (calls[1][0], l_tape))
    assert abs(calls[1][0] - l_tape) <= pc.LOSS_BAR * abs(l_tape)
    before = dict(pc.policy().named_parameters())
    tape_grads = {k: p.grad for k, p in u.net.named_parameters()}
    for (k, a), (_, b) in zip(t.net.named_parameters(), u.net.named_parameters()):
        if k not in pc.NAMES:
            assert torch.equal(a, b), k
            continue
        # p - lr g: the gradient bar times the learning rate, plus the one float32
        # rounding of the parameter each trainer makes
        g_max, p_max = float(tape_grads[k].abs().max()), float(b.detach().abs().max())
        tol = pc.GRAD_BAR * lr * g_max + 2 ** -23 * p_max
        diff = float((a.detach() - b.detach()).abs().max())
        assert diff <= tol, (k, diff, tol)
        assert not np.array_equal(N(a), N(before[k])), k       # the step moved them
