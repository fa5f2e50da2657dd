"""LearntCartpoleDynamics without a GPU: construction against the REAL class
(G20, tests/golden/make_golden_cartpole_learnt.py), the host twins of the
learnt step and rollout (include/apg_cpu_learnt.h: the per-lane header of the
kernels, csrc/cartpole_learnt_math.h) against G20's recorded forward and
autograd, the run_dynamics schedule of TrainCartpole, and the kernels'
resources as the build reports them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.05
PHYS = ("max_force_mag", "masspole", "length", "friction", "total_mass",
        "polemass_length")


def g20():
    return load_golden("cartpole_learnt.npz")


def golden_sd(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(g[k]))
            for k in g.files if k.startswith(prefix) and k[len(prefix):] not in ("seed", "keys")}


def fitted(g):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    m = LearntCartpoleDynamics()
    m.load_state_dict(golden_sd(g, "fit."), strict=True)
    return m


def close(got, want, rel):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(np.abs(want).max(), 1e-30)
    assert got.shape == want.shape
    err = np.abs(got - want).max()
    assert err <= rel * scale, (err, scale)


# ------------------------------------------------------------ construction
def test_init_state_dict_keys_order_and_strict_load():
    """Same parameter names, order and init draws as the reference: after
    torch.manual_seed the state_dict equals G20's exactly (the residual's
    four draws in the reference's order, cfg last - in torch's ParameterDict
    order, which the reference's state_dicts carry)."""
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    g = g20()
    torch.manual_seed(int(g["init.seed"]))
    m = LearntCartpoleDynamics()
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["init.keys"]]
    assert len([k for k in sd if k.startswith("cfg.")]) == 13
    for k, v in sd.items():
        want = g["init." + k]
        assert v.dtype == torch.float32 and tuple(v.shape) == want.shape, k
        assert np.array_equal(v.numpy(), want), k
    m2 = LearntCartpoleDynamics()
    m2.load_state_dict(golden_sd(g, "init."), strict=True)
    assert all(p.requires_grad for p in m2.parameters())
    frozen = LearntCartpoleDynamics(not_trainable="all")
    assert not any(p.requires_grad for p in frozen.cfg.values())
    assert frozen.linear_state_1.weight.requires_grad
    some = LearntCartpoleDynamics(not_trainable=["length", "wind"])
    assert [k for k, p in some.cfg.items() if not p.requires_grad] == ["length", "wind"]
    # modified_params; friction forced to 0.5 after them; derived keys once
    mod = LearntCartpoleDynamics({"masspole": .2, "friction": 3.0})
    assert float(mod.cfg["friction"].detach()) == .5
    assert float(mod.cfg["total_mass"].detach()) == np.float32(1.2)
    assert float(mod.cfg["polemass_length"].detach()) == np.float32(.2 * .5)


def test_no_analytic_params_and_rejects_host_tensors():
    """Nothing inherited may fly the construction-time analytic parameters:
    the module has no `params`; forward wants fp32 device tensors."""
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        CartpoleDynamics, LearntCartpoleDynamics)
    m = LearntCartpoleDynamics()
    assert isinstance(m, CartpoleDynamics) and isinstance(m, torch.nn.Module)
    assert not hasattr(m, "params")
    with pytest.raises(ValueError):
        m(torch.zeros(2, 4), torch.zeros(2, 1), DT)


# -------------------------------------------------------------- host twins
@pytest.fixture(scope="module")
def tw():
    from apg_trajectory_tracking_amd import build as b
    lib = ctypes.CDLL(b.build_cpu())
    return lib


class _Model:
    """ApgCartpoleLearnt over HOST copies of a module's tensors."""

    def __init__(self, m, residual=True):
        from apg_trajectory_tracking_amd import _capi
        self.arrays = [np.ascontiguousarray(m.cfg[k].detach().numpy(), np.float32)
                       for k in PHYS]
        if residual:
            self.arrays += [np.ascontiguousarray(t.detach().numpy(), np.float32) for t in (
                m.linear_state_1.weight, m.linear_state_1.bias, m.linear_state_2.weight)]
        ptrs = [a.ctypes.data for a in self.arrays] + [None] * (9 - len(self.arrays))
        self.struct = _capi.ApgCartpoleLearnt(*ptrs)


def fp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_twin_step_forward_and_cotangents_vs_golden(tw):
    g = g20()
    m = fitted(g)
    s = np.ascontiguousarray(g["step.state"], np.float32)
    a = np.ascontiguousarray(g["step.action"], np.float32)
    B = s.shape[0]
    out = np.zeros_like(s)
    for residual, key in ((True, "step.forward"), (False, "step.simulate")):
        mod = _Model(m, residual)
        assert tw.apg_cartpole_learnt_step_fwd_cpu(
            fp(s), fp(a), ctypes.c_float(DT), ctypes.byref(mod.struct), B, fp(out)) == 0
        close(out, g[key], 1e-5)
    mod = _Model(m)
    tw.apg_cartpole_learnt_step_fwd_cpu(fp(s), fp(a), ctypes.c_float(DT),
                                        ctypes.byref(mod.struct), B, fp(out))
    lam = np.ascontiguousarray(2 * (out - g["step.target"]), np.float32)
    gs, ga = np.zeros_like(s), np.zeros_like(a)
    gp = np.zeros(646, np.float32)
    assert tw.apg_cartpole_learnt_step_bwd_cpu(
        fp(s), fp(a), ctypes.c_float(DT), ctypes.byref(mod.struct), B, fp(lam), fp(gs),
        fp(ga), fp(gp), None) == 0
    close(gs, g["step.grad_state"], 1e-4)
    close(ga, g["step.grad_action"], 1e-4)
    for i, k in enumerate(PHYS):
        close(gp[i:i + 1], g["step.grad.cfg." + k], 1e-4)
    close(gp[6:326].reshape(64, 5), g["step.grad.linear_state_1.weight"], 1e-4)
    close(gp[326:390], g["step.grad.linear_state_1.bias"], 1e-4)
    close(gp[390:646].reshape(4, 64), g["step.grad.linear_state_2.weight"], 1e-4)
    # the seven keys that do not enter the physics get no gradient
    unused = [k for k in g["init.keys"] if k.startswith("cfg.") and k[4:] not in PHYS]
    assert len(unused) == 7
    assert all(int(g["step.has_grad." + k]) == 0 for k in unused)


@pytest.mark.parametrize("B", [8, 64])
def test_twin_rollout_vs_golden_controller_branch(tw, B):
    """The fused controller phase's per-lane composition: loss, and the
    policy gradients that its dL/dactions give through the shipped net."""
    from apg_trajectory_tracking_amd import _capi
    from test_cartpole_eval_cpu import golden_net
    g = g20()
    m = fitted(g)
    net = golden_net(load_golden("cartpole_closed_loop.npz"), "shipped")
    s = torch.from_numpy(g[f"ctrl{B}.state"])
    acts = net(s.clone()).reshape(B, 10, 1)
    a = np.ascontiguousarray(acts.detach().numpy(), np.float32)
    s0 = np.ascontiguousarray(s.numpy(), np.float32)
    parts = np.zeros(_capi.loss_partials_count(B), np.float32)
    loss = np.zeros(1, np.float32)
    ga, gs = np.zeros_like(a), np.zeros_like(s0)
    mod = _Model(m)
    assert tw.apg_cartpole_learnt_rollout_fwd_bwd_cpu(
        fp(s0), fp(a), ctypes.c_float(DT), ctypes.byref(mod.struct), B, 10, _capi.LAYOUT_AOS,
        fp(parts), fp(loss), fp(ga), fp(gs), None) == 0
    assert abs(loss[0] - float(g[f"ctrl{B}.loss"])) <= 1e-4 * float(g[f"ctrl{B}.loss"])
    acts.backward(torch.from_numpy(ga))
    for k, p in net.named_parameters():
        close(p.grad.numpy(), g[f"ctrl{B}.grad.{k}"], 1e-4)


def test_learnt_twins_repeat_the_device_signatures(tw):
    """include/apg_cpu_learnt.h: each twin resolves and repeats its apg.h
    entry point's parameter list minus the trailing stream."""
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    cpu = open(os.path.join(REPO, "include", "apg_cpu_learnt.h")).read()
    gpu = open(os.path.join(REPO, "include", "apg.h")).read()
    decls = re.findall(r"\bint\s+(apg_\w+_cpu)\s*\(([^;]*?)\)\s*;", cpu, re.S)
    assert len(decls) == 3
    for name, args in decls:
        assert hasattr(tw, name), name
        m = re.search(r"\bint\s+" + name[:-4] + r"\s*\(([^;]*?)\)\s*;", gpu, re.S)
        assert m, name
        dev_args = norm(m.group(1))
        assert dev_args.endswith(", apg_stream_t stream"), name
        assert norm(args) == dev_args[:-len(", apg_stream_t stream")], name


# ------------------------------------------------------- trainer schedule
def test_run_dynamics_schedule_with_stubbed_epochs(tmp_path, monkeypatch):
    """TrainBase.run_dynamics drives TrainCartpole.run_epoch(train=...,
    epoch=...) (the reference's TypeError there is the deviation): dynamics
    epochs for epoch <= train_dyn_for_epochs, then controller epochs;
    count_finetune_data grows by the batch per dynamics batch."""
    monkeypatch.chdir(tmp_path)
    from apg_trajectory_tracking_amd import train_cartpole as tc
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        CartpoleDynamics, LearntCartpoleDynamics)
    cfg = {"system": "cartpole", "delta_t": DT, "state_size": 4, "batch_size": 4,
           "nr_epochs": 5, "sample_in": "train_env", "horizon": 10, "action_dim": 1,
           "l2_lambda": 0, "train_dyn_for_epochs": 2, "train_dyn_every": 1,
           "save_name": str(tmp_path / "cp")}
    tr = tc.TrainCartpole(LearntCartpoleDynamics(), CartpoleDynamics(), cfg)
    batches = [(torch.rand(4, 4), torch.rand(4, 4)) for _ in range(3)]
    tr.trainloader = batches
    tr.net = lambda x: torch.zeros(x.shape[0], 10)
    calls = []

    def fit(state, action_seq):
        calls.append(("dyn", tuple(action_seq.shape)))
        return torch.tensor(1.0)

    def ctrl(state, action_seq):
        calls.append(("ctrl", tuple(action_seq.shape)))
        return torch.tensor(2.0)
    monkeypatch.setattr(tr, "train_dynamics_model", fit)
    monkeypatch.setattr(tr, "_controller_loss", ctrl)
    monkeypatch.setattr(tr, "_step", lambda loss: loss)
    tr.optimizer_controller = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0)
    monkeypatch.setattr(tr, "evaluate_model", lambda epoch: None)
    monkeypatch.setattr(tr, "sample_new_data", lambda epoch: None)
    monkeypatch.setattr(tr, "finalize", lambda: None)
    tr.run_dynamics(cfg)
    assert tr.results_dict["trained"] == ["dynamics"] * 3 + ["controller"] * 2
    assert [c[0] for c in calls] == ["dyn"] * 9 + ["ctrl"] * 6
    assert all(c[1] == (4, 10, 1) for c in calls)
    assert tr.results_dict["samples_in_d2"] == [12, 24, 36, 36, 36]
    assert tr.results_dict["loss_dynamics"] == [1.5] * 3
    assert tr.results_dict["loss_controller"] == [3.0] * 2
    # an analytic simulator still cannot be fitted; the regulariser is refused
    tr2 = tc.TrainCartpole(CartpoleDynamics(), CartpoleDynamics(), cfg)
    tr2.trainloader = batches
    with pytest.raises(NotImplementedError):
        tr2.run_epoch(train="dynamics", epoch=0)
    tr3 = tc.TrainCartpole(LearntCartpoleDynamics(), CartpoleDynamics(),
                           dict(cfg, l2_lambda=0.1))
    with pytest.raises(ValueError):
        tr3.train_dynamics_model(torch.zeros(2, 4), torch.zeros(2, 10, 1))


# -------------------------------------------------------------- resources
def test_new_kernels_no_scratch_and_analytic_closed_loop_unchanged():
    """Zero scratch and spills in every learnt cart-pole kernel; the analytic
    closed loop keeps the registers and occupancy of the parent build."""
    import kernel_names
    res = kernel_names.resources()
    loop = kernel_names.instances(res, "cart_closed_loop_kernel")
    assert sorted(loop) == ["ILb0E", "ILb1E"], sorted(loop)
    learnt = {("cart_closed_loop_kernel", "ILb1E"): loop["ILb1E"]}
    # the kernels of cartpole_learnt.hip, by name and number of instantiations
    for name, count in (("cart_learnt_rollout_kernel", 2), ("cart_learnt_reduce_kernel", 1),
                        ("cart_learnt_step_fwd_kernel", 1), ("cart_learnt_step_bwd_kernel", 1)):
        found = kernel_names.instances(res, name)
        assert len(found) == count, (name, sorted(found))
        learnt.update({(name, args): v for args, v in found.items()})
    assert len(learnt) == 6, sorted(learnt)
    for k, v in learnt.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
    ana = loop["ILb0E"]
    assert {k: ana[k] for k in ("vgprs", "agprs", "sgprs", "occupancy", "scratch")} == \
        {"vgprs": 71, "agprs": 64, "sgprs": 84, "occupancy": 3, "scratch": 0}
