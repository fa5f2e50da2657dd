"""The fused simulator-fit step of the learnt quadrotor on the GPU
(apg_quad_learnt_fit_fwd_bwd through functional.quad_learnt_fit_fwd_bwd and
TrainDrone.train_dynamics_model): the inputs and references of
test_quad_fit_cpu.py - the recordings of the real module (G10), float64 autograd
through the oracle, the regulariser - plus the host twin, run-to-run
determinism, parity of the trainer's fused and unfused fit steps, and a graph
capture of the whole step, optimizer included.  Bound: conftest.rel_err < 1e-4
(torch_inertia_vector against G10: 2e-3 / 5e-3, as test_quad_fit_cpu.py
explains); every test prints what it saw."""
import numpy as np
import pytest
import torch

import test_quad_fit_cpu as ref
from conftest import load_golden, rel_err
from test_quad_fit_cpu import tw  # noqa: F401  (the host twin, a fixture)

pytestmark = pytest.mark.gpu
BAR, DT = ref.BAR, ref.DT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def module(w, dev, init=ref.INIT):
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    dyn = LearntDynamics(initial_params=dict(init))
    dyn.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in w.items()})
    return dyn.to(dev)


def fit(w, dev, state, action, dt, target=None, params=None, l2=0.0, init=ref.INIT):
    """functional.quad_learnt_fit_fwd_bwd on the device, results as
    test_quad_fit_cpu.twin_fit returns them."""
    from apg_trajectory_tracking_amd import functional as F
    dyn = module(w, dev, init)
    to = lambda x: None if x is None else torch.as_tensor(np.asarray(x)).to(dev)
    res = F.quad_learnt_fit_fwd_bwd(dyn, to(state), to(action), dt, target=to(target),
                                    eval_params=params, l2_lambda=l2)
    views = F.quad_learnt_fit_grad_views(dyn, res["grad"])
    for (name, p), v in zip(dyn.named_parameters(), views):
        assert v.shape == p.shape and v.data_ptr() >= res["grad"].data_ptr(), name
    g = {name: v.cpu().numpy() for (name, _), v in zip(dyn.named_parameters(), views)}
    grad = res["grad"].cpu().numpy()
    for name, v in ref.split(grad).items():              # the views ARE the offsets
        assert np.array_equal(v, g[name]), name
    return dict(loss=float(res["loss"].item()), grad=grad, g=g)


# ---------------------------------------------------------------- 1: golden
def test_golden_loss_and_every_gradient_in_both_target_modes(dev):
    g = load_golden("learnt_dynamics.npz")
    w, dt = ref.weights("w"), float(g["dt"])
    by_params = fit(w, dev, g["state"], g["action"], dt, params=ref.eval_params())
    by_target = fit(w, dev, g["state"], g["action"], dt, target=g["target_next"])
    want = ref.golden_grads(g)
    for name, res in (("eval_params", by_params), ("target", by_target)):
        e = abs(res["loss"] - float(g["loss"])) / float(g["loss"])
        print(name, "loss error %.3g" % e)
        assert e < BAR
        ref.check_grads(res["g"], want, "gpu G10/" + name, bars={"torch_inertia_vector": 2e-3})
        assert res["g"]["mass"][0] == 0.0
    assert abs(by_params["loss"] - by_target["loss"]) < BAR * by_target["loss"]
    for k in w:
        assert rel_err(by_params["g"][k], by_target["g"][k]) < BAR, k


# ------------------------------------------------- 2: four momentum-SGD steps
def test_four_momentum_sgd_steps(dev):
    from apg_trajectory_tracking_amd import functional as F
    g = load_golden("learnt_dynamics.npz")
    dyn = module(ref.weights("w"), dev)
    state, action, tgt = (torch.from_numpy(g[k]).to(dev) for k in (
        "state", "action", "target_next"))
    opt = torch.optim.SGD(dyn.parameters(), lr=1e-4, momentum=0.9)
    losses = []
    for _ in range(4):
        res = F.quad_learnt_fit_fwd_bwd(dyn, state, action, float(g["dt"]), target=tgt)
        for p, v in zip(dyn.parameters(), F.quad_learnt_fit_grad_views(dyn, res["grad"])):
            p.grad = v
        opt.step()
        losses.append(res["loss"].item())
    errs = [abs(l - want) / want for l, want in zip(losses, g["steps.loss"])]
    print("loss errors", ["%.3g" % e for e in errs])
    assert max(errs) < BAR
    after = {k: v.cpu().numpy() for k, v in dyn.state_dict().items()}
    worst = max((rel_err(after[k], g["steps.w." + k]), k) for k in after)
    print("final weights, worst error %.3g (%s)" % worst)
    for k in after:
        tol = 5e-3 if k == "torch_inertia_vector" else BAR
        assert rel_err(after[k], g["steps.w." + k]) < tol, k


# ------------------------------------------- 3: float64 oracle, and the twin
@pytest.mark.parametrize("B", [1, 67, 321])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_against_float64_oracle(dev, which, B):
    s, a = ref.batch(B)
    w = ref.weights(which)
    want = ref.oracle(w, (which, B, 0.0), s, a, DT)
    res = fit(w, dev, s, a, DT, params=ref.eval_params())
    e = abs(res["loss"] - want["loss"]) / want["loss"]
    print(f"gpu {which}/B{B} loss error %.3g" % e)
    assert e < BAR
    ref.check_grads(res["g"], want["g"], f"gpu oracle/{which}/B{B}")


@pytest.mark.parametrize("B", [1, 64, 67, 321, 2500])
def test_against_the_host_twin(dev, tw, B):  # noqa: F811
    """The same per-lane header on both sides, so what differs is the order of
    the sums, the hardware sin / cos and fma contraction.  The flat gradient as
    one tensor and each parameter, both target modes, with and without the
    regulariser: a single lane, a full wave, a ragged wave, two workgroups, and
    (B = 2 500) ten workgroup rows - the last kernel's threads then add more
    than one row each."""
    s, a = ref.batch(B)
    w, ep = ref.weights("steps"), ref.eval_params()
    with torch.no_grad():
        from oracle import torch_port as tp
        tgt = tp.QuadOracle(dict(ref.MOD), dtype=torch.float32)(s, a, DT).numpy()
    for kw in (dict(params=ep), dict(target=tgt), dict(params=ep, l2=0.01)):
        got = fit(w, dev, s, a, DT, **kw)
        want = ref.twin_fit(tw, w, s, a, DT, **kw)
        errs = {"loss": abs(got["loss"] - want["loss"]) / want["loss"],
                "grad": rel_err(got["grad"], want["grad"])}
        for k in w:
            if k == "mass":
                assert got["g"][k][0] == 0.0 and want["g"][k][0] == 0.0
            else:
                errs[k] = rel_err(got["g"][k], want["g"][k])
        print(f"gpu vs twin B{B} {sorted(kw)}", {k: float("%.3g" % v) for k, v in errs.items()})
        for k, v in errs.items():
            assert v < BAR, (k, v)


# ------------------------------------------------------------- 4: regulariser
def test_regulariser_against_the_oracle_with_norm_terms(dev):
    B, l2 = 67, 0.01
    s, a = ref.batch(B)
    w = ref.weights("w")
    want = ref.oracle(w, ("w", B, l2), s, a, DT, l2=l2)
    res = fit(w, dev, s, a, DT, params=ref.eval_params(), l2=l2)
    e = abs(res["loss"] - want["loss"]) / want["loss"]
    print("gpu l2 loss error %.3g" % e)
    assert e < BAR
    ref.check_grads(res["g"], want["g"], "gpu oracle/l2")


def test_regulariser_on_a_fresh_zero_residual_is_finite(dev):
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    w = {k: v.detach().numpy() for k, v in LearntDynamics().state_dict().items()}
    s, a = ref.batch(67)
    data = fit(w, dev, s, a, DT, params=ref.eval_params(), init={})
    res = fit(w, dev, s, a, DT, params=ref.eval_params(), l2=0.01, init={})
    print("fresh module: loss %.6g with and %.6g without the penalty" % (
        res["loss"], data["loss"]))
    assert np.isfinite(res["loss"]) and res["loss"] == data["loss"]
    assert np.all(np.isfinite(res["grad"]))
    for k in ref.RESIDUAL:
        assert np.array_equal(res["g"][k], data["g"][k]), k
    assert np.any(data["g"]["linear_state_2.bias"])


def test_empty_batch_and_argument_errors(dev):
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    dyn = module(ref.weights("w"), dev)
    s, a = torch.zeros(0, 12, device=dev), torch.zeros(0, 4, device=dev)
    res = F.quad_learnt_fit_fwd_bwd(dyn, s, a, DT, eval_params=ref.eval_params())
    assert res["loss"].item() == 0.0 and not torch.any(res["grad"])
    assert res["grad"].shape == (1891,)
    s, a = (t.to(dev) for t in ref.batch(3))
    with pytest.raises(ValueError):
        F.quad_learnt_fit_fwd_bwd(dyn, s, a, DT)
    with pytest.raises(ValueError):
        F.quad_learnt_fit_fwd_bwd(dyn, s, a, DT, target=s, eval_params=ref.eval_params())
    with pytest.raises(ValueError):
        F.quad_learnt_fit_fwd_bwd(dyn, s, a, DT, target=s, l2_lambda=-1.0)
    with pytest.raises(ValueError):
        F.quad_learnt_fit_fwd_bwd(dyn, s, a[:, :3], DT, target=s)
    wide = LearntDynamics()
    wide.linear_state_1 = torch.nn.Linear(16, 32)
    wide.linear_state_2 = torch.nn.Linear(32, 12)
    assert not F.quad_learnt_fusable(wide.to(dev)) and F.quad_learnt_fusable(dyn)
    with pytest.raises(ValueError):
        F.quad_learnt_fit_fwd_bwd(wide, s, a, DT, target=s)


# ---------------------------------------------------------------- determinism
def test_two_calls_give_the_same_bits(dev):
    from apg_trajectory_tracking_amd import functional as F
    dyn = module(ref.weights("steps"), dev)
    s, a = (t.to(dev) for t in ref.batch(321))
    runs = [F.quad_learnt_fit_fwd_bwd(dyn, s, a, DT, eval_params=ref.eval_params(),
                                      l2_lambda=0.01) for _ in range(2)]
    assert torch.equal(runs[0]["grad"], runs[1]["grad"])
    assert torch.equal(runs[0]["loss"], runs[1]["loss"])
    assert runs[0]["grad"].data_ptr() != runs[1]["grad"].data_ptr()


# ------------------------------------------------------ the trainer's fit step
def _trainer(dev, tmp_path, l2, lr=1e-4):
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    from apg_trajectory_tracking_amd.train_base import momentum_sgd
    from apg_trajectory_tracking_amd.train_drone import TrainDrone
    cfg = dict(delta_t=DT, delta_t_train=DT, epoch_size=8, self_play=0, batch_size=8,
               state_size=12, horizon=10, ref_dim=9, action_dim=4, train_mode="concurrent",
               learning_rate_controller=1e-7, learning_rate_dynamics=lr, l2_lambda=l2,
               system="quad", save_name=str(tmp_path / "t"), sample_in="train_env")
    dyn = module(ref.weights("w"), dev)
    t = TrainDrone(dyn, FlightmareDynamics(modified_params=dict(ref.MOD)), cfg)
    t.optimizer_dynamics = momentum_sgd(dyn.parameters(), lr)
    t.grad_sync_dynamics = None
    return t


def _batch(dev, B):
    s, a = ref.batch(B)
    actions = a.unsqueeze(1).repeat(1, 10, 1).contiguous()
    return s.to(dev), actions.to(dev)


def test_fused_and_unfused_fit_steps_agree(dev, tmp_path):
    s, actions = _batch(dev, 67)
    out = {}
    for fused in (True, False):
        t = _trainer(dev, tmp_path, l2=0.01)
        t.fused_fit = fused
        assert t._fusable_fit(s, actions) == fused
        losses = [float(t.train_dynamics_model(s, actions).detach()) for _ in range(3)]
        out[fused] = (losses, {k: v.cpu().numpy()
                               for k, v in t.train_dynamics.state_dict().items()})
    errs = [abs(a - b) / abs(b) for a, b in zip(out[True][0], out[False][0])]
    print("fused vs unfused loss errors", ["%.3g" % e for e in errs])
    assert max(errs) < BAR and out[True][0][2] < out[True][0][0]
    worst = max((rel_err(out[True][1][k], v), k) for k, v in out[False][1].items())
    print("final state_dict, worst error %.3g (%s)" % worst)
    for k, v in out[False][1].items():
        assert rel_err(out[True][1][k], v) < BAR, k


def test_the_whole_fit_step_is_capturable(dev, tmp_path):
    """One warm-up step (the optimizer's momentum buffers come to life), one
    step captured, replayed twice = three eager steps, bit for bit."""
    s, actions = _batch(dev, 67)
    eager = _trainer(dev, tmp_path, l2=0.01)
    for _ in range(3):
        eager.train_dynamics_model(s, actions)
    t = _trainer(dev, tmp_path, l2=0.01)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        t.train_dynamics_model(s, actions)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = t.train_dynamics_model(s, actions)
    one = {k: v.clone() for k, v in t.train_dynamics.state_dict().items()}
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for k, v in eager.train_dynamics.state_dict().items():
        got = t.train_dynamics.state_dict()[k]
        assert torch.equal(got, v), (k, rel_err(got.cpu().numpy(), v.cpu().numpy()))
    assert not torch.equal(one["linear_at"], t.train_dynamics.linear_at.detach())
    assert float(loss) == float(eager.results_dict["loss_dyn_per_step"][-1])
    print("captured step replayed twice: final loss %.6g" % float(loss))
