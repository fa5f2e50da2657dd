"""The fused simulator-fit step of the learnt cart-pole on the GPU
(apg_cartpole_learnt_fit_fwd_bwd through functional.cartpole_learnt_fit_fwd_bwd
and TrainCartpole.train_dynamics_model): the recordings of the real module (G20:
`step.*`, `train_all.*`, `train_frozen.*`), the host twin of
test_cartpole_fit_cpu.py, run-to-run determinism, parity of the trainer's fused
and unfused fit steps, and a graph capture of the whole step, optimizer
included.  Bounds: the golden within 1e-4 of the tensor's scale
(test_cartpole_learnt_cpu.close), the twin within conftest.rel_err < 1e-4; every
test prints what it saw."""
import numpy as np
import pytest
import torch

import test_cartpole_fit_cpu as ref
from conftest import rel_err
from test_cartpole_fit_cpu import tw  # noqa: F401  (the host twin, a fixture)
from test_cartpole_learnt_cpu import DT, close, g20

pytestmark = pytest.mark.gpu
BAR = ref.BAR


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def module(w, dev, not_trainable=()):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    dyn = LearntCartpoleDynamics(not_trainable=not_trainable)
    dyn.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in w.items()})
    return dyn.to(dev)


def fit(w, dev, state, action, dt, target=None, params=None):
    """functional.cartpole_learnt_fit_fwd_bwd on the device, results as
    test_cartpole_fit_cpu.twin_fit returns them."""
    from apg_trajectory_tracking_amd import functional as F
    dyn = module(w, dev)
    assert F.cartpole_learnt_fusable(dyn)
    to = lambda x: None if x is None else torch.as_tensor(np.asarray(x)).to(dev)
    res = F.cartpole_learnt_fit_fwd_bwd(dyn, to(state), to(action), dt, target=to(target),
                                        eval_params=params)
    views = F.cartpole_learnt_fit_grad_views(dyn, res["grad"])
    g = {name: v.cpu().numpy() for (name, _), v in zip(dyn.named_parameters(), views)
         if v is not None}
    grad = res["grad"].cpu().numpy()
    assert sorted(g) == sorted(ref.split(grad))
    for name, v in ref.split(grad).items():              # the views ARE the offsets
        assert np.array_equal(v, g[name]), name
    return dict(loss=float(res["loss"].item()), grad=grad, g=g)


# ---------------------------------------------------------------- 1: golden
def test_golden_loss_and_every_gradient_in_both_target_modes(dev):
    g = g20()
    w = ref.weights("fit")
    by_target = fit(w, dev, g["step.state"], g["step.action"], DT, target=g["step.target"])
    by_params = fit(w, dev, g["step.state"], g["step.action"], DT, params=ref.eval_params())
    ref.check_golden(by_target, g, "gpu G20/target")
    ref.check_golden(by_params, g, "gpu G20/eval_params")
    assert abs(by_params["loss"] - by_target["loss"]) < BAR * by_target["loss"]
    for k in by_target["g"]:
        assert rel_err(by_params["g"][k], by_target["g"][k]) < BAR, k


# ------------------------------------------------------------ 2: the host twin
@pytest.mark.parametrize("B", [1, 64, 67, 321, 2500])
def test_against_the_host_twin(dev, tw, B):  # noqa: F811
    """The same per-lane header on both sides, so what differs is the order of
    the sums, the hardware sin / cos and fma contraction.  The flat gradient as
    one tensor and each parameter, both target modes: a single lane, a full
    wave, a ragged wave, two workgroups, and (B = 2 500) ten workgroup rows - the
    reduce kernel's threads then add more than one row each.

    One key has a bound of its own, after the precedent of torch_inertia_vector
    in the quadrotor's fit tests: cfg.polemass_length at B = 1 with a given
    target.  A single sample, so no order of summation is involved; the scalar
    is the sum of two terms (through x_dot' and through theta_dot') that cancel
    to 1 / 26 of their size, and the theta_dot' residual pred - target is 1 / 94
    of pred, so ONE float32 ulp of the predicted theta_dot' (2.4e-7: the
    hardware's sin / cos against libm's) moves the gradient by 1.8e-4 of itself.
    test_cartpole_fit_cpu.prediction_ulp_bound evaluates that in float64 from
    the same per-sample terms: 1.95e-4, which is the bound used; measured on
    the MI355X: 1.76e-4 (exactly the one ulp of theta_dot').  With the target
    stepped in-lane the ulp is shared by prediction and target: 5.9e-6."""
    s, a = ref.batch(B)
    w, ep = ref.weights("fit"), ref.eval_params()
    tgt = ref.twin_target(tw, s.numpy(), a.numpy(), DT, ep)
    for kw in (dict(params=ep), dict(target=tgt)):
        bars = {}
        if B == 1 and "target" in kw:
            one_ulp = ref.prediction_ulp_bound(w, s, a, DT, tgt, "cfg.polemass_length")
            print("cfg.polemass_length, one ulp of the prediction: %.3g" % one_ulp)
            assert BAR < one_ulp < 2.5 * BAR     # shown, and no licence beyond it
            bars["cfg.polemass_length"] = one_ulp
        got = fit(w, dev, s, a, DT, **kw)
        want = ref.twin_fit(tw, w, s, a, DT, **kw)
        errs = {"loss": abs(got["loss"] - want["loss"]) / want["loss"],
                "grad": rel_err(got["grad"], want["grad"])}
        for k in want["g"]:
            errs[k] = rel_err(got["g"][k], want["g"][k])
        print(f"gpu vs twin B{B} {sorted(kw)}", {k: float("%.3g" % v) for k, v in errs.items()})
        for k, v in errs.items():
            assert v < bars.get(k, BAR), (k, v)


# ------------------------------------------------------------- 3: determinism
def test_two_calls_give_the_same_bits(dev):
    from apg_trajectory_tracking_amd import functional as F
    dyn = module(ref.weights("fit"), dev)
    s, a = (t.to(dev) for t in ref.batch(2500))
    runs = [F.cartpole_learnt_fit_fwd_bwd(dyn, s, a, DT, eval_params=ref.eval_params())
            for _ in range(2)]
    assert torch.equal(runs[0]["grad"], runs[1]["grad"])
    assert torch.equal(runs[0]["loss"], runs[1]["loss"])
    assert runs[0]["grad"].data_ptr() != runs[1]["grad"].data_ptr()
    assert torch.any(runs[0]["grad"] != 0) and runs[0]["loss"].item() > 0


def test_empty_batch_and_argument_errors(dev):
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    dyn = module(ref.weights("fit"), dev)
    s, a = torch.zeros(0, 4, device=dev), torch.zeros(0, 1, device=dev)
    res = F.cartpole_learnt_fit_fwd_bwd(dyn, s, a, DT, eval_params=ref.eval_params())
    assert res["loss"].item() == 0.0 and not torch.any(res["grad"])
    assert res["grad"].shape == (646,)
    s, a = (t.to(dev) for t in ref.batch(3))
    with pytest.raises(ValueError):
        F.cartpole_learnt_fit_fwd_bwd(dyn, s, a, DT)
    with pytest.raises(ValueError):
        F.cartpole_learnt_fit_fwd_bwd(dyn, s, a, DT, target=s, eval_params=ref.eval_params())
    with pytest.raises(ValueError):
        F.cartpole_learnt_fit_fwd_bwd(dyn, s, a.repeat(1, 2), DT, target=s)
    with pytest.raises(ValueError):
        F.cartpole_learnt_fit_fwd_bwd(dyn, s, a, DT, target=s[:, :3])
    wide = LearntCartpoleDynamics()
    wide.linear_state_1 = torch.nn.Linear(5, 32)
    wide.linear_state_2 = torch.nn.Linear(32, 4, bias=False)
    assert not F.cartpole_learnt_fusable(wide.to(dev)) and F.cartpole_learnt_fusable(dyn)
    with pytest.raises(ValueError):
        F.cartpole_learnt_fit_fwd_bwd(wide, s, a, DT, target=s)


# ------------------------------------------------------ the trainer's fit step
class Wrapped:
    """An eval dynamics that is not the plain analytic class: called in torch,
    its output handed over as the target."""

    def __init__(self, inner):
        self.inner = inner

    def __call__(self, state, action, dt):
        return self.inner(state, action, dt)


def trainer(dyn, tmp_path, fused, lr=0.01, wrap=False):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.train_base import momentum_sgd
    from apg_trajectory_tracking_amd.train_cartpole import TrainCartpole
    cfg = {"system": "cartpole", "delta_t": DT, "state_size": 4, "batch_size": 16,
           "nr_epochs": 1, "sample_in": "train_env", "horizon": 10, "action_dim": 1,
           "l2_lambda": 0, "save_name": str(tmp_path / "fit")}
    evald = CartpoleDynamics(dict(ref.MOD))
    t = TrainCartpole(dyn, Wrapped(evald) if wrap else evald, cfg)
    t.optimizer_dynamics = momentum_sgd(dyn.parameters(), lr)
    t.grad_sync_dynamics = None
    t.fused_fit = fused
    return t


def seeded(dev, nt):
    """G20's train case: the module as torch.manual_seed(21) draws it."""
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    torch.manual_seed(21)
    return LearntCartpoleDynamics(not_trainable=nt).to(dev)


def train_batch(dev, tag):
    g = g20()
    s = torch.from_numpy(g[f"train_{tag}.state"]).to(dev)
    a = torch.from_numpy(g[f"train_{tag}.action"]).to(dev)
    return s, a[:, None, :].repeat(1, 10, 1)


@pytest.mark.parametrize("tag,nt", [("all", []), ("frozen", "all")])
def test_five_momentum_sgd_steps_of_the_trainer_vs_golden(dev, tmp_path, tag, nt):
    """TrainCartpole.train_dynamics_model with fused_fit = True (momentum 0.9,
    lr 0.01): the loss of each step and the state_dict after it; the frozen
    module keeps all 13 cfg gradients None."""
    g = g20()
    m = seeded(dev, nt)
    t = trainer(m, tmp_path, fused=True)
    s, seq = train_batch(dev, tag)
    assert t._fusable_fit(s, seq)
    stamps = (m.timestamp, t.eval_dynamics.timestamp)
    errs = []
    for k in range(5):
        loss = t.train_dynamics_model(s, seq)
        want = float(g[f"train_{tag}.losses"][k])
        errs.append(abs(loss.item() - want) / want)
        assert errs[-1] <= BAR, (k, loss.item(), want)
        for key, v in m.state_dict().items():
            close(v.cpu(), g[f"train_{tag}.after{k}.{key}"], BAR)
        none = sum(p.grad is None for p in m.cfg.values())
        assert none == (13 if nt == "all" else 7), none
        assert all(p.grad is not None for p in (
            m.linear_state_1.weight, m.linear_state_1.bias, m.linear_state_2.weight))
    print(f"train_{tag} loss errors", ["%.3g" % e for e in errs])
    assert len(t.results_dict["loss_dyn_per_step"]) == 5
    # both dynamics' timestamp side effects are kept
    assert m.timestamp == pytest.approx(stamps[0] + 5 * .05)
    assert t.eval_dynamics.timestamp == pytest.approx(stamps[1] + 5 * .05)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("nt", [[], ["length"]])
def test_fused_and_unfused_fit_steps_agree(dev, tmp_path, monkeypatch, wrap, nt):
    """Loss and every .grad, the None ones included, of one trainer step from
    the fitted module - with a plain CartpoleDynamics as eval dynamics (stepped
    inside the kernel) and a wrapped one (called, handed over as target)."""
    from apg_trajectory_tracking_amd import functional as F
    s, a = (x.to(dev) for x in ref.batch(67))
    seq = a[:, None, :].repeat(1, 10, 1)
    seq[:, 1:] += 0.25                       # only the first action may be used
    calls = []
    real = F.cartpole_learnt_fit_fwd_bwd
    monkeypatch.setattr(F, "cartpole_learnt_fit_fwd_bwd",
                        lambda *p, **kw: calls.append(kw) or real(*p, **kw))
    out = {}
    for fused in (True, False):
        m = module(ref.weights("fit"), dev, not_trainable=nt)
        t = trainer(m, tmp_path, fused, lr=1e-3, wrap=wrap)
        assert t._fusable_fit(s, seq) == fused
        del calls[:]
        loss = float(t.train_dynamics_model(s, seq).detach())
        assert len(calls) == (1 if fused else 0)
        if fused:
            assert (calls[0].get("target") is not None) == wrap
            assert (calls[0].get("eval_params") is not None) == (not wrap)
        out[fused] = (loss, {k: None if p.grad is None else p.grad.cpu().numpy()
                             for k, p in m.named_parameters()},
                      {k: v.cpu().numpy() for k, v in m.state_dict().items()},
                      (m.timestamp, t.eval_dynamics.inner.timestamp if wrap
                       else t.eval_dynamics.timestamp))
    e = abs(out[True][0] - out[False][0]) / abs(out[False][0])
    worst = ("", 0.0)
    for k, want in out[False][1].items():
        got = out[True][1][k]
        assert (got is None) == (want is None), k
        if want is not None:
            worst = max(worst, (k, rel_err(got, want)), key=lambda x: x[1])
            assert rel_err(got, want) < BAR, (k, rel_err(got, want))
    print(f"fused vs unfused (wrap {wrap}, frozen {nt}): loss error %.3g, worst gradient "
          "%.3g (%s)" % (e, worst[1], worst[0]))
    assert e < BAR
    assert sum(v is None for v in out[True][1].values()) == 7 + len(nt)
    for k, v in out[False][2].items():
        assert rel_err(out[True][2][k], v) < BAR, k
    assert out[True][3] == pytest.approx(out[False][3])


def test_the_whole_fit_step_is_capturable(dev, tmp_path):
    """One warm-up step (the optimizer's momentum buffers come to life), the
    module and the buffers put back, one step captured and replayed three times
    = three eager steps within 1e-4."""
    s, seq = train_batch(dev, "all")
    eager_m = seeded(dev, [])
    eager = trainer(eager_m, tmp_path, fused=True)
    for _ in range(3):
        eager.train_dynamics_model(s, seq)
    m = seeded(dev, [])
    start = {k: v.clone() for k, v in m.state_dict().items()}
    t = trainer(m, tmp_path, fused=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        t.train_dynamics_model(s, seq)
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(start[k])
        for st in t.optimizer_dynamics.state.values():
            st["momentum_buffer"].zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = t.train_dynamics_model(s, seq)
    for k, v in m.state_dict().items():          # capturing ran nothing
        assert torch.equal(v, start[k]), k
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    want_loss = float(eager.results_dict["loss_dyn_per_step"][-1])
    e = abs(float(loss) - want_loss) / want_loss
    worst = max((rel_err(m.state_dict()[k].cpu().numpy(), v.cpu().numpy()), k)
                for k, v in eager_m.state_dict().items())
    print("captured step replayed three times: loss %.6g (error %.3g), worst state_dict "
          "error %.3g (%s)" % (float(loss), e, worst[0], worst[1]))
    assert e < BAR and worst[0] < BAR
    assert not torch.equal(m.linear_state_1.weight.detach(), start["linear_state_1.weight"])
    assert not torch.equal(m.cfg["length"].detach(), start["cfg.length"])


def test_the_call_touches_nothing_but_its_outputs(dev):
    """functional.cartpole_learnt_fit_fwd_bwd leaves every parameter of the
    module (value, requires_grad, .grad) and its inputs as they were."""
    from apg_trajectory_tracking_amd import functional as F
    dyn = module(ref.weights("fit"), dev, not_trainable=["length"])
    s, a = (t.to(dev) for t in ref.batch(321))
    before = {k: v.clone() for k, v in dyn.state_dict().items()}
    flags = [p.requires_grad for p in dyn.parameters()]
    s0, a0, stamp = s.clone(), a.clone(), dyn.timestamp
    res = F.cartpole_learnt_fit_fwd_bwd(dyn, s, a, DT, eval_params=ref.eval_params())
    torch.cuda.synchronize()
    assert torch.any(res["grad"] != 0)
    for k, v in dyn.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert [p.requires_grad for p in dyn.parameters()] == flags
    assert all(p.grad is None for p in dyn.parameters())
    assert torch.equal(s, s0) and torch.equal(a, a0) and dyn.timestamp == stamp
