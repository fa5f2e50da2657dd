"""The fused simulator-fit step of the learnt quadrotor without a GPU: the host
twin of apg_quad_learnt_fit_fwd_bwd (include/apg_cpu_quad_fit.h - the per-lane
header of the kernel, csrc/quad_fit_math.h, looped over the batch) against the
recordings of the REAL module (G10, learnt_dynamics.npz: the loss, every
parameter's gradient, four momentum-SGD steps), against float64 autograd through
the oracle, the regulariser, its reduction to the physics step's own reverse,
the argument checks, the kernels' resources as the build reports them, and the
trainer's routing with the twin standing behind the functional.

Bound: the project's parity bar, conftest.rel_err < 1e-4 (for a scalar: the
relative error).  torch_inertia_vector against G10 alone is granted what
tests/test_gpu_trainers.py grants it - 2e-3 on the gradient, 5e-3 on the stepped
weights: the reference's autograd differentiates J and inverse(J) separately
there, the closed form keeps what does not cancel.  Against the float64 oracle
kinv and inertia are checked with the closed forms evaluated in float64 from the
oracle's own lam, at the parity bar.  Every test prints what it saw."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

BAR = 1e-4
DT = 0.1
SETS = {"w": "w.", "steps": "steps.w."}
RESIDUAL = ("linear_state_1.weight", "linear_state_1.bias",
            "linear_state_2.weight", "linear_state_2.bias")
# G10's recipe (tests/golden/make_golden.py): what the module is built with and
# the mismatched simulator it is fitted to
INIT = {"rotational_drag": [.01, .02, .03]}
MOD = dict(translational_drag=[.1, .2, .3], rotational_drag=[.01, .02, .03], mass=1.0)
# (name, offset attribute of _capi, shape) in LearntDynamics.parameters() order
LAYOUT = (("linear_at", "QUAD_FIT_G_LINEAR_AT", (4, 4)), ("mass", "QUAD_FIT_G_MASS", (1,)),
          ("torch_inertia_vector", "QUAD_FIT_G_INERTIA", (3,)),
          ("torch_kinv_vector", "QUAD_FIT_G_KINV", (3,)),
          ("linear_state_1.weight", "QUAD_FIT_G_W1", (64, 16)),
          ("linear_state_1.bias", "QUAD_FIT_G_B1", (64,)),
          ("linear_state_2.weight", "QUAD_FIT_G_W2", (12, 64)),
          ("linear_state_2.bias", "QUAD_FIT_G_B2", (12,)))


def weights(which):
    """{reference state_dict name: float32 array} of a recorded weight set."""
    g = load_golden("learnt_dynamics.npz")
    p = SETS[which]
    return {k[len(p):]: np.array(g[k]) for k in g.files if k.startswith(p)}


def sim_params():
    """The struct the module simulates with: its construction-time constants."""
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    return LearntDynamics(initial_params=dict(INIT)).params


def eval_params():
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    return FlightmareDynamics(modified_params=dict(MOD)).params


@pytest.fixture(scope="module")
def tw():
    from apg_trajectory_tracking_amd import build as b
    return ctypes.CDLL(b.build_cpu())


def fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class HostModel:
    """ApgLearntResidual over HOST arrays: `w` a {state_dict name: array}."""

    def __init__(self, w):
        from apg_trajectory_tracking_amd import _capi
        self.arrays = [np.ascontiguousarray(w[k], np.float32)
                       for k in ("linear_at",) + RESIDUAL]
        self.struct = _capi.ApgLearntResidual(*[a.ctypes.data for a in self.arrays])


def split(grad):
    """{parameter name: its part of the flat gradient}, by the published offsets."""
    from apg_trajectory_tracking_amd import _capi
    out = {}
    for name, off, shape in LAYOUT:
        o = getattr(_capi, off)
        out[name] = grad[o:o + int(np.prod(shape))].reshape(shape)
    return out


def twin_fit(tw, w, state, action, dt, target=None, params=None, l2=0.0, sim=None):
    """The twin behind the conventions of functional.quad_learnt_fit_fwd_bwd:
    dict(loss, grad (flat), g ({name: array}))."""
    from apg_trajectory_tracking_amd import _capi
    s = np.ascontiguousarray(np.asarray(state, np.float32))
    a = np.ascontiguousarray(np.asarray(action, np.float32))
    t = None if target is None else np.ascontiguousarray(np.asarray(target, np.float32))
    B = s.shape[0]
    parts = np.zeros(_capi.loss_partials_count(B), np.float32)
    loss = np.full(1, np.nan, np.float32)
    grad = np.full(_capi.QUAD_FIT_GRADS, np.nan, np.float32)
    m = HostModel(w)
    sim = sim or sim_params()
    rc = tw.apg_quad_learnt_fit_fwd_bwd_cpu(
        fp(s), fp(a), ctypes.c_float(dt), ctypes.byref(sim), ctypes.byref(m.struct), fp(t),
        None if params is None else ctypes.byref(params), ctypes.c_float(l2), B,
        fp(parts), fp(loss), fp(grad), None)
    assert rc == 0, rc
    return dict(loss=float(loss[0]), grad=grad, g=split(grad), parts=parts)


def batch(B):
    """G10's recipe at another size: positions, rates and velocities all live."""
    gen = torch.Generator().manual_seed(62 + B)
    state = torch.randn(B, 12, generator=gen)
    state[:, 3:6] *= 0.4
    action = torch.rand(B, 4, generator=gen)
    return state, action


_ORACLE = {}


def oracle(w, key, state, action, dt, l2=0.0):
    """loss and {name: gradient} of the fit loss in float64: autograd through
    LearntQuadOracle for its five tensors, the closed forms of kinv / inertia
    from the oracle's own lam, mass 0; target = the oracle's analytic step on
    the modified parameters (computed once per `key`, shared, never written
    to)."""
    if key not in _ORACLE:
        from oracle import torch_port as tp
        f64 = torch.float64
        ora = tp.LearntQuadOracle(w, initial_params=dict(INIT), dtype=f64)
        leaves = {"linear_at": "A", "linear_state_1.weight": "w1", "linear_state_1.bias": "b1",
                  "linear_state_2.weight": "w2", "linear_state_2.bias": "b2"}
        for attr in leaves.values():
            getattr(ora, attr).requires_grad_()
        with torch.no_grad():
            tgt = tp.QuadOracle(dict(MOD), dtype=f64)(state, action, dt)
        pred = ora(state, action, dt)
        loss = torch.sum((pred - tgt)**2)
        if l2 > 0:
            loss = loss + l2 * sum(torch.norm(t) for t in (ora.w2, ora.b2, ora.w1, ora.b1))
        loss.backward()
        g = {k: getattr(ora, attr).grad.numpy() for k, attr in leaves.items()}
        with torch.no_grad():
            lam_w = (2 * (pred - tgt))[:, 9:12]
            at = (ora.A @ action.to(f64).unsqueeze(2))[:, :, 0]
            omega = state.to(f64)[:, 9:12]
            g["torch_kinv_vector"] = (lam_w * (dt * ((at[:, 1:] - 0.5) - omega))).sum(0).numpy()
            J = torch.diagonal(ora.base.J)
            g["torch_inertia_vector"] = (-(lam_w.sum(0)) * dt * ora.base.r_drag / J**2).numpy()
        g["mass"] = None
        _ORACLE[key] = dict(loss=float(loss.detach()), g=g, target=tgt.numpy())
    return _ORACLE[key]


def check_grads(got, want, what, bar=BAR, bars=None):
    """Every parameter's gradient against `want` ({name: array or None = exactly
    zero}); prints the largest error."""
    worst = ("", 0.0)
    for k, v in want.items():
        if v is None:
            assert not np.any(got[k]), (what, k)
            continue
        e = rel_err(got[k], np.asarray(v).reshape(got[k].shape))
        if e > worst[1]:
            worst = (k, e)
        assert e < (bars or {}).get(k, bar), (what, k, e)
    print(what, "worst gradient error %.3g (%s)" % (worst[1], worst[0]))


def golden_grads(g):
    want = {name: g["g." + name] for name, _, _ in LAYOUT}
    assert not np.any(want["mass"])
    want["mass"] = None
    return want


# ------------------------------------------------------------ 1: golden G10
def test_golden_loss_and_every_gradient_in_both_target_modes(tw):
    g = load_golden("learnt_dynamics.npz")
    w, dt = weights("w"), float(g["dt"])
    by_params = twin_fit(tw, w, g["state"], g["action"], dt, params=eval_params())
    by_target = twin_fit(tw, w, g["state"], g["action"], dt, target=g["target_next"])
    want = golden_grads(g)
    for name, res in (("eval_params", by_params), ("target", by_target)):
        e = abs(res["loss"] - float(g["loss"])) / float(g["loss"])
        print(name, "loss error %.3g" % e)
        assert e < BAR
        check_grads(res["g"], want, "G10/" + name, bars={"torch_inertia_vector": 2e-3})
        assert res["g"]["mass"][0] == 0.0
        assert np.all(np.isfinite(res["grad"]))
    assert abs(by_params["loss"] - by_target["loss"]) < BAR * by_target["loss"]
    e = rel_err(by_params["grad"], by_target["grad"])
    print("eval_params vs target, whole gradient: %.3g" % e)
    assert e < BAR
    for k in w:
        assert rel_err(by_params["g"][k], by_target["g"][k]) < BAR, k


# ------------------------------------------------- 2: four momentum-SGD steps
def test_four_momentum_sgd_steps_on_the_twins_gradients(tw):
    """lr 1e-4, momentum 0.9, as torch.optim.SGD: buf = 0.9 buf + g (the first
    buf = g), p -= lr buf.  kinv / inertia drift while the step keeps the
    constants of construction time - the recorded losses pin that."""
    g = load_golden("learnt_dynamics.npz")
    w = {k: v.copy() for k, v in weights("w").items()}
    lr, dt = np.float32(1e-4), float(g["dt"])
    sim = sim_params()
    buf, losses = {}, []
    for step in range(4):
        res = twin_fit(tw, w, g["state"], g["action"], dt, target=g["target_next"], sim=sim)
        losses.append(res["loss"])
        for k in w:
            gk = res["g"][k].reshape(w[k].shape)
            buf[k] = gk.copy() if step == 0 else np.float32(0.9) * buf[k] + gk
            w[k] = (w[k] - lr * buf[k]).astype(np.float32)
    errs = [abs(l - want) / want for l, want in zip(losses, g["steps.loss"])]
    print("loss errors", ["%.3g" % e for e in errs])
    assert max(errs) < BAR
    worst = max((rel_err(w[k], g["steps.w." + k]), k) for k in w)
    print("final weights, worst error %.3g (%s)" % worst)
    for k in w:
        tol = 5e-3 if k == "torch_inertia_vector" else BAR
        assert rel_err(w[k], g["steps.w." + k]) < tol, k
    assert not np.array_equal(w["torch_kinv_vector"], weights("w")["torch_kinv_vector"])


# ---------------------------------------------------------- 3: float64 oracle
@pytest.mark.parametrize("B", [1, 67, 321])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_twin_against_float64_oracle(tw, which, B):
    """One live lane, a ragged second wave, more than one workgroup with a
    ragged tail."""
    s, a = batch(B)
    w = weights(which)
    want = oracle(w, (which, B, 0.0), s, a, DT)
    res = twin_fit(tw, w, s, a, DT, params=eval_params())
    e = abs(res["loss"] - want["loss"]) / want["loss"]
    print(f"{which}/B{B} loss error %.3g" % e)
    assert e < BAR
    check_grads(res["g"], want["g"], f"oracle/{which}/B{B}")
    assert res["parts"].shape == ((B + 63) // 64,)


# ------------------------------------------------------------- 4: regulariser
def test_regulariser_against_the_oracle_with_norm_terms(tw):
    B, l2 = 67, 0.01
    s, a = batch(B)
    w = weights("w")
    want = oracle(w, ("w", B, l2), s, a, DT, l2=l2)
    plain = oracle(w, ("w", B, 0.0), s, a, DT)
    assert want["loss"] > plain["loss"]
    assert rel_err(want["g"]["linear_state_2.bias"], plain["g"]["linear_state_2.bias"]) > BAR
    res = twin_fit(tw, w, s, a, DT, params=eval_params(), l2=l2)
    e = abs(res["loss"] - want["loss"]) / want["loss"]
    print("l2 loss error %.3g" % e)
    assert e < BAR
    check_grads(res["g"], want["g"], "oracle/l2")


def test_regulariser_on_a_fresh_zero_residual_is_finite(tw):
    """|t| = 0 for all four tensors - the state every fresh module starts in:
    gradient 0 from the penalty (torch's norm backward), nothing non-finite."""
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    w = {k: v.detach().numpy() for k, v in LearntDynamics().state_dict().items()}
    assert not any(np.any(w[k]) for k in RESIDUAL)
    s, a = batch(67)
    sim = LearntDynamics().params
    data = twin_fit(tw, w, s, a, DT, params=eval_params(), sim=sim)
    res = twin_fit(tw, w, s, a, DT, params=eval_params(), l2=0.01, sim=sim)
    assert np.isfinite(res["loss"]) and res["loss"] == data["loss"]
    assert np.all(np.isfinite(res["grad"]))
    for k in RESIDUAL:
        assert np.array_equal(res["g"][k], data["g"][k]), k
    assert np.any(data["g"]["linear_state_2.bias"])     # the data term is there


# ------------------------------------------------- 5: reduction to known code
def test_zero_residual_identity_transform_is_the_step_reverse(tw):
    """All residual weights zero, linear_at the identity, l2_lambda = 0: pred is
    the physics step, so with grad_next = lam = 2 (pred - target) the cotangents
    of apg_quad_step_bwd_cpu give the three non-residual gradients in closed
    form: dlinear_at = sum_b grad_action (x) a, dkinv = sum_b lam_w dt ((a - 1/2)
    - w), dinertia = -(sum_b lam_w) dt d_r / J^2; and db2 = sum_b lam."""
    from apg_trajectory_tracking_amd import _capi
    B = 67
    s, a = batch(B)
    w = weights("steps")
    for k in RESIDUAL:
        w[k] = np.zeros_like(w[k])
    w["linear_at"] = np.eye(4, dtype=np.float32)
    sim, ep = sim_params(), eval_params()
    sn, an = s.numpy().copy(), a.numpy().copy()
    pred, tgt = np.zeros_like(sn), np.zeros_like(sn)
    for p, out in ((sim, pred), (ep, tgt)):
        assert tw.apg_quad_step_fwd_cpu(fp(sn), fp(an), ctypes.c_float(DT), ctypes.byref(p), B,
                                        _capi.LAYOUT_AOS, fp(out)) == 0
    lam = (2 * (pred - tgt)).astype(np.float32)
    gs, ga = np.zeros_like(sn), np.zeros_like(an)
    assert tw.apg_quad_step_bwd_cpu(fp(sn), fp(an), ctypes.c_float(DT), ctypes.byref(sim), B,
                                    _capi.LAYOUT_AOS, fp(lam), fp(gs), fp(ga)) == 0
    lam64, a64, s64 = lam.astype(np.float64), an.astype(np.float64), sn.astype(np.float64)
    J = np.array(list(sim.inertia), np.float64)
    rd = np.array(list(sim.rot_drag), np.float64)
    want = {"linear_at": ga.astype(np.float64).T @ a64,
            "torch_kinv_vector": (lam64[:, 9:] * (DT * ((a64[:, 1:] - 0.5) - s64[:, 9:]))).sum(0),
            "torch_inertia_vector": -lam64[:, 9:].sum(0) * DT * rd / J**2,
            "mass": None,
            "linear_state_2.bias": lam64.sum(0)}
    assert np.any(want["torch_inertia_vector"])
    res = twin_fit(tw, w, s, a, DT, params=ep, sim=sim)
    check_grads(res["g"], want, "zero residual")
    assert not np.any(res["g"]["linear_state_1.weight"])    # W2 = 0: nothing reaches W1
    e = abs(res["loss"] - float(np.sum((pred - tgt).astype(np.float64)**2)))
    assert e < BAR * res["loss"]


# ---------------------------------------------------------- 6: argument checks
def test_argument_checks(tw):
    from apg_trajectory_tracking_amd import _capi
    g = load_golden("learnt_dynamics.npz")
    m = HostModel(weights("w"))
    s, a, t = (np.ascontiguousarray(g[k], np.float32) for k in (
        "state", "action", "target_next"))
    ep, sim = eval_params(), sim_params()
    parts, loss = np.zeros(1, np.float32), np.full(1, 7.0, np.float32)
    grad = np.full(_capi.QUAD_FIT_GRADS, 7.0, np.float32)

    def call(model, target, params, B=64, l2=0.0):
        return tw.apg_quad_learnt_fit_fwd_bwd_cpu(
            fp(s), fp(a), ctypes.c_float(DT), ctypes.byref(sim), model, fp(target),
            None if params is None else ctypes.byref(params), ctypes.c_float(l2), B,
            fp(parts), fp(loss), fp(grad), None)
    ok = ctypes.byref(m.struct)
    assert call(ok, t, ep) == -1            # both
    assert call(ok, None, None) == -1       # neither
    assert call(None, t, None) == -1        # no model
    for missing in range(5):                # each of its pointers
        ptrs = [x.ctypes.data for x in m.arrays]
        ptrs[missing] = None
        assert call(ctypes.byref(_capi.ApgLearntResidual(*ptrs)), t, None) == -1, missing
    assert call(ok, t, None, B=-1) == -1
    assert call(ok, t, None, l2=-0.5) == -1
    assert np.all(grad == 7.0) and loss[0] == 7.0       # nothing ran
    assert call(ok, t, None, B=0) == 0
    assert loss[0] == 0.0 and not np.any(grad)


def test_the_twin_repeats_the_device_signature(tw):
    import os
    import re
    from conftest import REPO
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    cpu = open(os.path.join(REPO, "include", "apg_cpu_quad_fit.h")).read()
    gpu = open(os.path.join(REPO, "include", "apg.h")).read()
    decls = re.findall(r"\bint\s+(apg_\w+_cpu)\s*\(([^;]*?)\)\s*;", cpu, re.S)
    assert [d[0] for d in decls] == ["apg_quad_learnt_fit_fwd_bwd_cpu"]
    name, args = decls[0]
    m = re.search(r"\bint\s+" + name[:-4] + r"\s*\(([^;]*?)\)\s*;", gpu, re.S)
    dev_args = norm(m.group(1))
    assert dev_args.endswith(", apg_stream_t stream")
    assert norm(args) == dev_args[:-len(", apg_stream_t stream")]
    # the offsets of apg.h, mirrored in _capi
    from apg_trajectory_tracking_amd import _capi
    defines = re.findall(r"#define APG_QUAD_FIT_(\w+) (\d+)", gpu)
    assert len(defines) == 9
    for n, v in defines:
        assert getattr(_capi, "QUAD_FIT_" + n) == int(v), n
    assert _capi.lib().apg_quad_learnt_fit_grad_count() == _capi.QUAD_FIT_GRADS == 1891
    # ... and they are LearntDynamics.parameters() order
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    off = 0
    for (name, p), (want, attr, shape) in zip(LearntDynamics().named_parameters(), LAYOUT):
        assert name == want and tuple(p.shape) == shape and getattr(_capi, attr) == off, name
        off += p.numel()
    assert off == _capi.QUAD_FIT_GRADS


# ------------------------------------------------------------ 7: build report
def test_fit_kernels_have_no_scratch_and_no_spills():
    from apg_trajectory_tracking_amd import build
    build.build()
    with open(build.RESOURCES) as f:
        res = json.load(f)
    mine = {k: v for k, v in res.items() if "quad_learnt_fit" in k}
    assert len([k for k in mine if "quad_learnt_fit_kernelILb" in k]) == 2, sorted(mine)
    assert any("fit_pack_kernel" in k for k in mine)
    assert any("fit_reduce_kernel" in k for k in mine)
    for k, v in mine.items():
        print(k, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)


# ------------------------------------------------ 8: trainer routing, no GPU
def _trainer(train_dynamics, eval_dynamics, tmp_path, l2=0.0):
    from apg_trajectory_tracking_amd.train_base import momentum_sgd
    from apg_trajectory_tracking_amd.train_drone import TrainDrone
    cfg = dict(delta_t=DT, delta_t_train=DT, epoch_size=8, self_play=0, batch_size=8,
               state_size=12, horizon=10, ref_dim=9, action_dim=4, train_mode="concurrent",
               learning_rate_controller=1e-7, learning_rate_dynamics=1e-4, l2_lambda=l2,
               system="quad", save_name=str(tmp_path / "t"), sample_in="train_env")
    t = TrainDrone(train_dynamics, eval_dynamics, cfg)
    t.optimizer_dynamics = momentum_sgd(train_dynamics.parameters(), 1e-4)
    t.grad_sync_dynamics = None
    return t


def _learnt(which="steps"):
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    learnt = LearntDynamics(initial_params=dict(INIT))
    learnt.load_state_dict({k: torch.from_numpy(v) for k, v in weights(which).items()})
    return learnt


def _patch(monkeypatch, tw, calls):
    """The twin behind functional.quad_learnt_fit_fwd_bwd; the base method
    replaced by a marker."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd import train_base

    def fused(dyn, state, action, dt, target=None, eval_params=None, l2_lambda=0.0):
        calls.append(dict(dyn=dyn, action=action, dt=dt, target=target,
                          eval_params=eval_params, l2=l2_lambda))
        w = {k: v.detach().numpy() for k, v in dyn.state_dict().items()}
        res = twin_fit(tw, w, state.numpy(), action.numpy(), dt,
                       target=None if target is None else target.numpy(),
                       params=eval_params, l2=l2_lambda, sim=dyn.params)
        return dict(loss=torch.tensor([res["loss"]]), grad=torch.from_numpy(res["grad"]))
    monkeypatch.setattr(F, "quad_learnt_fit_fwd_bwd", fused)

    def base(self, current_state, action_seq):
        calls.append("base")
        return torch.zeros(())
    monkeypatch.setattr(train_base.TrainBase, "train_dynamics_model", base)


def test_trainer_routes_the_fit_to_the_fused_step(tw, tmp_path, monkeypatch):
    """train_dynamics_model of a TrainDrone whose train dynamics is the stock
    module calls functional.quad_learnt_fit_fwd_bwd (here: the twin behind it)
    with the first action, delta_t, the eval dynamics' parameters and l2_lambda,
    sets every .grad and steps the optimizer; an eval dynamics that is not the
    plain analytic one is called in torch and handed over as `target`."""
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    B, H = 8, 10
    s0, a0 = batch(B)
    actions = a0.unsqueeze(1).repeat(1, H, 1).contiguous()
    actions[:, 1:] += 0.25                   # only the first action may be used
    learnt = _learnt()
    calls = []
    _patch(monkeypatch, tw, calls)
    evald = FlightmareDynamics(modified_params=dict(MOD))
    t = _trainer(learnt, evald, tmp_path, l2=0.01)
    assert t.fused_fit is True and t._fusable_fit(s0, actions)
    before = {k: v.clone() for k, v in learnt.state_dict().items()}
    loss = t.train_dynamics_model(s0, actions)
    assert len(calls) == 1 and calls[0]["eval_params"] is evald.params
    assert calls[0]["dyn"] is learnt and torch.equal(calls[0]["action"], a0)
    assert calls[0]["target"] is None and calls[0]["dt"] == DT
    assert calls[0]["l2"] == pytest.approx(0.01)
    want = oracle(weights("steps"), ("steps", "routing"), s0, a0, DT, l2=0.01)
    print("routed loss %.6g, oracle %.6g" % (float(loss), want["loss"]))
    assert abs(float(loss) - want["loss"]) < BAR * want["loss"]
    for k, p in learnt.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        if want["g"][k] is None:
            assert not torch.any(p.grad), k
        else:
            assert rel_err(p.grad.numpy(), want["g"][k]) < BAR, k
        # the optimizer stepped: p = before - lr grad (first momentum step)
        assert torch.allclose(p.detach(), before[k] - 1e-4 * p.grad, rtol=0, atol=1e-7), k
    assert not torch.equal(learnt.linear_at.detach(), before["linear_at"])
    assert len(t.results_dict["loss_dyn_per_step"]) == 1

    # an eval dynamics that is not the plain analytic one: called in torch
    class Other:
        def __call__(self, state, action, dt):
            return state + action.sum(1, keepdim=True) * dt
    del calls[:]
    t2 = _trainer(learnt, Other(), tmp_path)
    t2.train_dynamics_model(s0, actions)
    assert len(calls) == 1 and calls[0]["eval_params"] is None and calls[0]["l2"] == 0.0
    assert torch.equal(calls[0]["target"], s0 + a0.sum(1, keepdim=True) * DT)


def test_trainer_falls_back_to_the_base_method(tw, tmp_path, monkeypatch):
    """fused_fit = False, and a residual of another shape: the base method."""
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    s0, a0 = batch(8)
    actions = a0.unsqueeze(1).repeat(1, 10, 1).contiguous()
    calls = []
    _patch(monkeypatch, tw, calls)
    evald = FlightmareDynamics(modified_params=dict(MOD))
    wide = LearntDynamics()
    wide.linear_state_1 = torch.nn.Linear(16, 32)
    wide.linear_state_2 = torch.nn.Linear(32, 12)
    off = _trainer(_learnt(), evald, tmp_path)
    off.fused_fit = False
    for tr in (off, _trainer(wide, evald, tmp_path)):
        assert not tr._fusable_fit(s0, actions)
        del calls[:]
        tr.train_dynamics_model(s0, actions)
        assert calls == ["base"]
