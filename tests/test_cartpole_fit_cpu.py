"""The fused simulator-fit step of the learnt cart-pole without a GPU: the host
twin of apg_cartpole_learnt_fit_fwd_bwd (include/apg_cpu_cartpole_fit.h - the
per-lane header of the kernel, csrc/cartpole_fit_math.h, looped over the batch)
against the recordings of the REAL module (G20, cartpole_learnt.npz: `step.*`),
against a float64 restatement under autograd written here, the argument checks,
the per-parameter views of the flat gradient, the ABI mirror and the kernels'
resources as the build reports them.

Bounds: the project's own - the golden within 1e-4 relative to the tensor's
scale (test_cartpole_learnt_cpu.close), the oracle within conftest.rel_err <
1e-4 (for a scalar: the relative error).  Every test prints what it saw."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_err
from test_cartpole_learnt_cpu import DT, PHYS, close, g20, golden_sd

BAR = 1e-4
MOD = {"masspole": .2, "length": .7}        # G20's eval dynamics
RESIDUAL = ("linear_state_1.weight", "linear_state_1.bias", "linear_state_2.weight")
# (state_dict name, offset attribute of _capi or index, shape): the ONE layout
LAYOUT = tuple(("cfg." + k, i, (1,)) for i, k in enumerate(PHYS)) + (
    ("linear_state_1.weight", "CARTPOLE_LEARNT_G_W1", (64, 5)),
    ("linear_state_1.bias", "CARTPOLE_LEARNT_G_B1", (64,)),
    ("linear_state_2.weight", "CARTPOLE_LEARNT_G_W2", (4, 64)))


@pytest.fixture(scope="module")
def tw():
    from apg_trajectory_tracking_amd import build as b
    return ctypes.CDLL(b.build_cpu())


def fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def weights(which):
    """{state_dict name: float32 array} of G20's `fit.` or `init.` module."""
    return {k: v.numpy() for k, v in golden_sd(g20(), which + ".").items()}


def eval_params():
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    return CartpoleDynamics(dict(MOD)).params


class HostModel:
    """ApgCartpoleLearnt over HOST arrays: `w` a {state_dict name: array}."""

    def __init__(self, w):
        from apg_trajectory_tracking_amd import _capi
        self.arrays = [np.ascontiguousarray(w["cfg." + k], np.float32) for k in PHYS]
        self.arrays += [np.ascontiguousarray(w[k], np.float32) for k in RESIDUAL]
        self.struct = _capi.ApgCartpoleLearnt(*[a.ctypes.data for a in self.arrays])


def split(grad):
    """{parameter name: its part of the flat gradient}, by the published offsets."""
    from apg_trajectory_tracking_amd import _capi
    out = {}
    for name, off, shape in LAYOUT:
        o = off if isinstance(off, int) else getattr(_capi, off)
        out[name] = grad[o:o + int(np.prod(shape))].reshape(shape)
    return out


def twin_fit(tw, w, state, action, dt, target=None, params=None):
    """The twin behind the conventions of functional.cartpole_learnt_fit_fwd_bwd:
    dict(loss, grad (flat), g ({name: array}), parts)."""
    from apg_trajectory_tracking_amd import _capi
    s = np.ascontiguousarray(np.asarray(state, np.float32))
    a = np.ascontiguousarray(np.asarray(action, np.float32))
    t = None if target is None else np.ascontiguousarray(np.asarray(target, np.float32))
    B = s.shape[0]
    parts = np.zeros(_capi.loss_partials_count(B), np.float32)
    loss = np.full(1, np.nan, np.float32)
    grad = np.full(_capi.CARTPOLE_LEARNT_GRADS, np.nan, np.float32)
    m = HostModel(w)
    rc = tw.apg_cartpole_learnt_fit_fwd_bwd_cpu(
        fp(s), fp(a), ctypes.c_float(dt), ctypes.byref(m.struct), fp(t),
        None if params is None else ctypes.byref(params), B, fp(parts), fp(loss), fp(grad),
        None)
    assert rc == 0, (rc, tw.apg_cpu_last_error_string())
    return dict(loss=float(loss[0]), grad=grad, g=split(grad), parts=parts)


def twin_target(tw, state, action, dt, params):
    """apg_cartpole_step_fwd_cpu: the target the eval dynamics produces."""
    from apg_trajectory_tracking_amd import _capi
    s = np.ascontiguousarray(np.asarray(state, np.float32))
    a = np.ascontiguousarray(np.asarray(action, np.float32))
    out = np.zeros_like(s)
    assert tw.apg_cartpole_step_fwd_cpu(fp(s), fp(a), ctypes.c_float(dt), ctypes.byref(params),
                                        s.shape[0], _capi.LAYOUT_AOS, fp(out)) == 0
    return out


def batch(B):
    """G20's recipe for states and actions at another size: the whole range of
    every component, a quarter of the lanes with a large theta_dot.  theta stays
    inside (-3, 3): the step's wrap of theta + dt theta_dot is the same function
    of the inputs in prediction and target, so a sample an ulp from +-pi would
    only test whether float32 and float64 round it to the same side."""
    gen = torch.Generator().manual_seed(70 + B)
    s = (torch.rand(B, 4, generator=gen) * 2 - 1) * torch.tensor([2.4, 7.5, 3.0, 7.5])
    q = B // 4
    s[:q, 3] = (torch.rand(q, generator=gen) * 2 - 1) * 25
    a = torch.rand(B, 1, generator=gen) * 2 - 1
    return s.float(), a.float()


# ------------------------------------------------- float64 restatement (oracle)
def physics64(s, a, dt, F, mp, l, mu, tm, pml):
    """simulate_cartpole (neural_control/dynamics/cartpole_dynamics.py:53-119) in
    the tensors' dtype on SIX independent parameters, gravity 9.81."""
    grav = 9.81
    x, xd, th, thd = s.unbind(-1)
    force = a[..., 0] * F * 0.5
    sn, cs = torch.sin(th), torch.cos(th)
    xacc = (-2 * pml * thd**2 * sn + 3 * mp * grav * sn * cs + 4 * force - 4 * mu * xd) / (
        4 * tm - 3 * mp * cs**2)
    thacc = (-3 * pml * thd**2 * sn * cs + 6 * tm * grav * sn + 6 * (force - mu * xd) * cs) / (
        4 * l * tm - 3 * pml * cs**2)
    sd, cd = torch.sin(thd * dt), torch.cos(thd * dt)
    new_th = torch.atan2(sn * cd + cs * sd, cs * cd - sn * sd)
    return torch.stack([x + xd * dt, xd + xacc * dt, new_th, thd + thacc * dt], -1)


def oracle_target(state, action, dt):
    """CartpoleDynamics(MOD)'s step in float64 (friction .5, total_mass and
    polemass_length derived)."""
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import _config
    cfg = _config(dict(MOD))
    f64 = torch.float64
    return physics64(state.to(f64), action.to(f64), dt,
                     *[torch.tensor(float(cfg[k]), dtype=f64) for k in PHYS])


def forward64(w, state, action, dt):
    """(leaves, prediction) of the module in float64: physics on the six
    parameters plus the 5 -> 64 -> 4 relu residual on the pre-step state and the
    raw action; the leaves require a gradient."""
    f64 = torch.float64
    leaf = {k: torch.tensor(np.asarray(w[k], np.float64), dtype=f64, requires_grad=True)
            for k in ["cfg." + p for p in PHYS] + list(RESIDUAL)}
    s, a = torch.as_tensor(state).to(f64), torch.as_tensor(action).to(f64)
    pred = physics64(s, a, dt, *[leaf["cfg." + k][0] for k in PHYS])
    z = torch.cat([s, a], 1)
    hidden = torch.relu(z @ leaf["linear_state_1.weight"].t() + leaf["linear_state_1.bias"])
    return leaf, pred + hidden @ leaf["linear_state_2.weight"].t()


def oracle(w, state, action, dt, target):
    """loss and {name: gradient} of the fit loss in float64 under autograd."""
    leaf, pred = forward64(w, state, action, dt)
    loss = ((pred - torch.as_tensor(target).to(torch.float64))**2).sum()
    loss.backward()
    return dict(loss=float(loss.detach()), g={k: v.grad.numpy() for k, v in leaf.items()})


def prediction_ulp_bound(w, state, action, dt, target, key):
    """How far ONE float32 ulp of every predicted component moves the scalar
    gradient `key`, relative to that gradient, all in float64:
        sum_{b,i} |d g_key / d pred_bi| ulp32(pred_bi) / |g_key|
    (g_key = sum lam_bi dpred_bi/dkey is linear in lam = 2 (pred - target), so
    d g_key / d pred_bi = -d g_key / d target_bi, which autograd gives).  No
    float32 evaluation of the step - the twin's, the kernel's, torch's - can be
    held closer to another one than this."""
    leaf, pred = forward64(w, state, action, dt)
    tgt = torch.as_tensor(np.asarray(target, np.float64)).requires_grad_()
    loss = ((pred - tgt)**2).sum()
    (g,) = torch.autograd.grad(loss, leaf[key], create_graph=True)
    (sens,) = torch.autograd.grad(g[0], tgt)
    ulp = np.spacing(np.abs(pred.detach().numpy()).astype(np.float32)).astype(np.float64)
    return float((sens.abs().numpy() * ulp).sum() / abs(float(g[0].detach())))


def check_grads(got, want, what, bar=BAR):
    """Every parameter's gradient against `want`; prints the largest error."""
    worst = ("", 0.0)
    for k, v in want.items():
        e = rel_err(got[k], np.asarray(v).reshape(got[k].shape))
        if e > worst[1]:
            worst = (k, e)
        assert e < bar, (what, k, e)
    print(what, "worst gradient error %.3g (%s)" % (worst[1], worst[0]))


def golden_grads(g, tag="step"):
    return {name: g[f"{tag}.grad.{name}"] for name, _, _ in LAYOUT}


def check_golden(res, g, what):
    e = abs(res["loss"] - float(g["step.loss"])) / float(g["step.loss"])
    print(what, "loss %.6g, golden %.6g, error %.3g" % (res["loss"], float(g["step.loss"]), e))
    assert e < BAR
    for name, want in golden_grads(g).items():
        close(res["g"][name], np.asarray(want).reshape(res["g"][name].shape), BAR)
    assert np.all(np.isfinite(res["grad"]))


# ----------------------------------------------------------- 1: golden G20
def test_golden_loss_and_every_gradient_with_the_given_target(tw):
    g = g20()
    assert g["step.state"].shape == (256, 4)
    res = twin_fit(tw, weights("fit"), g["step.state"], g["step.action"], DT,
                   target=g["step.target"])
    check_golden(res, g, "G20/target")
    assert res["parts"].shape == (4,) and abs(res["parts"].sum() - res["loss"]) < BAR * res["loss"]


def test_golden_with_the_eval_params_target_and_both_modes_agree(tw):
    """The eval dynamics stepped inside the call; the batch's target as the
    twin's own apg_cartpole_step_fwd_cpu produces it is G20's recorded one, and
    handing that over gives what the in-lane step gives."""
    g = g20()
    w, ep = weights("fit"), eval_params()
    tgt = twin_target(tw, g["step.state"], g["step.action"], DT, ep)
    close(tgt, g["step.target"], 1e-5)
    by_params = twin_fit(tw, w, g["step.state"], g["step.action"], DT, params=ep)
    by_target = twin_fit(tw, w, g["step.state"], g["step.action"], DT, target=tgt)
    check_golden(by_params, g, "G20/eval_params")
    assert abs(by_params["loss"] - by_target["loss"]) < BAR * by_target["loss"]
    e = rel_err(by_params["grad"], by_target["grad"])
    print("eval_params vs target, whole gradient: %.3g" % e)
    assert e < BAR
    for name, _, _ in LAYOUT:
        assert rel_err(by_params["g"][name], by_target["g"][name]) < BAR, name


# ---------------------------------------------------------- 2: float64 oracle
def test_float64_oracle_reproduces_the_golden():
    """The restatement itself against the recordings of the real module."""
    g = g20()
    want = oracle(weights("fit"), g["step.state"], g["step.action"], DT, g["step.target"])
    e = abs(want["loss"] - float(g["step.loss"])) / float(g["step.loss"])
    print("oracle loss error against G20 %.3g" % e)
    assert e < BAR
    for name, gold in golden_grads(g).items():
        close(want["g"][name].reshape(np.asarray(gold).shape), gold, BAR)
    tgt = oracle_target(torch.from_numpy(g["step.state"]), torch.from_numpy(g["step.action"]), DT)
    # (G20's batch has lanes an ulp from +-pi: compare the angle on the circle)
    d = tgt.numpy() - g["step.target"].astype(np.float64)
    d[:, 2] = (d[:, 2] + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(d).max() < 1e-5 * np.abs(g["step.target"]).max()


_ORACLE = {}


def oracle_case(which, B):
    """(state, action, float64 target, oracle result) - computed once per case,
    shared with tests/test_gpu_cartpole_fit.py, never written to."""
    if (which, B) not in _ORACLE:
        s, a = batch(B)
        tgt = oracle_target(s, a, DT).numpy()
        _ORACLE[which, B] = (s, a, tgt, oracle(weights(which), s, a, DT, tgt))
    return _ORACLE[which, B]


@pytest.mark.parametrize("B", [1, 67, 321])
@pytest.mark.parametrize("which", ["fit", "init"])
def test_twin_against_float64_oracle(tw, which, B):
    """One live lane, a ragged second wave, more than one workgroup with a
    ragged tail; the fitted module (a residual that matters) and a fresh one
    (weights of 1e-4: the physics gradients dominate)."""
    s, a, _, want = oracle_case(which, B)
    res = twin_fit(tw, weights(which), s, a, DT, params=eval_params())
    e = abs(res["loss"] - want["loss"]) / want["loss"]
    print(f"{which}/B{B} loss %.6g, error %.3g" % (res["loss"], e))
    assert e < BAR
    check_grads(res["g"], want["g"], f"oracle/{which}/B{B}")
    assert res["parts"].shape == ((B + 63) // 64,)


# ---------------------------------------------------------- 3: argument checks
def test_empty_batch_and_argument_errors(tw):
    from apg_trajectory_tracking_amd import _capi
    g = g20()
    m = HostModel(weights("fit"))
    s, a, t = (np.ascontiguousarray(g[k], np.float32) for k in (
        "step.state", "step.action", "step.target"))
    ep = eval_params()
    parts, loss = np.zeros(1, np.float32), np.full(1, 7.0, np.float32)
    grad = np.full(_capi.CARTPOLE_LEARNT_GRADS, 7.0, np.float32)

    def call(model, target, params, B=64, state=s, action=a, parts=parts, grad=grad):
        return tw.apg_cartpole_learnt_fit_fwd_bwd_cpu(
            fp(state), fp(action), ctypes.c_float(DT), model, fp(target),
            None if params is None else ctypes.byref(params), B, fp(parts), fp(loss),
            fp(grad), None)
    ok = ctypes.byref(m.struct)
    assert call(ok, t, ep) == -1            # both
    assert call(ok, None, None) == -1       # neither
    assert call(None, t, None) == -1        # no model
    for missing in range(9):                # each of its pointers, the residual's too
        ptrs = [x.ctypes.data for x in m.arrays]
        ptrs[missing] = None
        assert call(ctypes.byref(_capi.ApgCartpoleLearnt(*ptrs)), t, None) == -1, missing
    ptrs = [x.ctypes.data for x in m.arrays[:6]] + [None] * 3     # physics only
    assert call(ctypes.byref(_capi.ApgCartpoleLearnt(*ptrs)), t, None) == -1
    assert call(ok, t, None, B=-1) == -1
    assert call(ok, t, None, grad=None) == -1
    assert np.all(grad == 7.0) and loss[0] == 7.0       # nothing ran
    assert call(ok, t, None, state=None) == -1
    assert call(ok, t, None, action=None) == -1
    assert call(ok, t, None, parts=None) == -1
    assert loss[0] == 7.0
    assert call(ok, t, None, B=0) == 0
    assert loss[0] == 0.0 and not np.any(grad)
    # the device entry point reports the same errors before any HIP call
    lib = _capi.lib()

    def dev(model, target, params, B=64, grad=1):
        return lib.apg_cartpole_learnt_fit_fwd_bwd(
            1, 1, DT, model, target, None if params is None else ctypes.byref(params), B, 1,
            1, grad, 1, None)
    assert dev(ok, 1, ep) == -1 and b"exactly one" in lib.apg_last_error_string()
    assert dev(ok, None, None) == -1
    assert dev(None, 1, None) == -1
    assert dev(ctypes.byref(_capi.ApgCartpoleLearnt(*ptrs)), 1, None) == -1
    assert b"w1 / b1 / w2" in lib.apg_last_error_string()
    assert dev(ok, 1, None, B=-1) == -1 and b"B must be" in lib.apg_last_error_string()
    assert dev(ok, 1, None, grad=None) == -1
    assert lib.apg_cartpole_learnt_fit_workspace_floats(0) == 0
    assert lib.apg_cartpole_learnt_fit_workspace_floats(256) == 672
    assert lib.apg_cartpole_learnt_fit_workspace_floats(257) == 2 * 672


# --------------------------------------------------------------- 4: grad views
@pytest.mark.parametrize("nt", [[], "all", ["length"]])
def test_grad_views_shapes_offsets_and_none_pattern(nt):
    from apg_trajectory_tracking_amd import _capi, functional as F
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    g = g20()
    dyn = LearntCartpoleDynamics(not_trainable=nt)
    grad = torch.arange(_capi.CARTPOLE_LEARNT_GRADS, dtype=torch.float32)
    views = F.cartpole_learnt_fit_grad_views(dyn, grad)
    names = [k for k, _ in dyn.named_parameters()]
    assert len(views) == len(names) == 16
    want_at = {name: (off if isinstance(off, int) else getattr(_capi, off))
               for name, off, _ in LAYOUT}
    for name, p, v in zip(names, dyn.parameters(), views):
        frozen = name.startswith("cfg.") and (nt == "all" or name[4:] in nt)
        if name not in want_at or frozen:
            assert v is None, name
            continue
        assert v.shape == p.shape and v.dtype == torch.float32, name
        assert v.data_ptr() == grad.data_ptr() + 4 * want_at[name], name     # a view
        assert float(v.reshape(-1)[0]) == want_at[name], name
    # ... which is the pattern autograd leaves in the real module
    if nt != ["length"]:
        tag = "step_frozen" if nt == "all" else "step"
        for name, v in zip(names, views):
            assert int(v is not None) == int(g[f"{tag}.has_grad.{name}"]), name
    assert sum(v is None for v in views) == (13 if nt == "all" else 7 + len(nt))
    # a host module is not what the fused step serves
    assert not F.cartpole_learnt_fusable(dyn)
    with pytest.raises(ValueError):
        F.cartpole_learnt_fit_fwd_bwd(dyn, torch.zeros(2, 4), torch.zeros(2, 1), DT,
                                      eval_params=eval_params())


# ------------------------------------------------------------------ 5: the ABI
def test_the_twin_and_capi_repeat_the_device_signature(tw):
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    cpu = open(os.path.join(REPO, "include", "apg_cpu_cartpole_fit.h")).read()
    gpu = open(os.path.join(REPO, "include", "apg.h")).read()
    decls = re.findall(r"\bint\s+(apg_\w+_cpu)\s*\(([^;]*?)\)\s*;", cpu, re.S)
    assert [d[0] for d in decls] == ["apg_cartpole_learnt_fit_fwd_bwd_cpu"]
    name, args = decls[0]
    assert hasattr(tw, name)
    m = re.search(r"\bint\s+" + name[:-4] + r"\s*\(([^;]*?)\)\s*;", gpu, re.S)
    dev_args = norm(m.group(1))
    assert dev_args.endswith(", apg_stream_t stream")
    assert norm(args) == dev_args[:-len(", apg_stream_t stream")]
    # the ctypes prototype, argument by argument
    from apg_trajectory_tracking_amd import _capi
    kinds = {"const float *": ctypes.c_void_p, "float *": ctypes.c_void_p,
             "float": ctypes.c_float, "int": ctypes.c_int, "apg_stream_t": ctypes.c_void_p,
             "const ApgCartpoleLearnt *": ctypes.POINTER(_capi.ApgCartpoleLearnt),
             "const ApgCartpoleParams *": ctypes.POINTER(_capi.ApgCartpoleParams)}
    want = [kinds[norm(re.match(r"(.*?)(\w+)$", norm(a)).group(1))] for a in dev_args.split(",")]
    assert _capi.SIGNATURES["apg_cartpole_learnt_fit_fwd_bwd"] == want
    assert _capi.SIGNATURES["apg_cartpole_learnt_fit_workspace_floats"] == [ctypes.c_int]
    # the offsets of apg.h, mirrored in _capi: ONE layout, the step reverse's
    defines = re.findall(r"#define APG_CARTPOLE_LEARNT_(\w+) (\d+)", gpu)
    assert len(defines) == 4
    for n, v in defines:
        assert getattr(_capi, "CARTPOLE_LEARNT_" + n) == int(v), n
    assert _capi.lib().apg_cartpole_learnt_param_count() == _capi.CARTPOLE_LEARNT_GRADS == 646
    assert _capi.CARTPOLE_LEARNT_FIELDS == PHYS
    off = 0
    for name, at, shape in LAYOUT:
        assert (at if isinstance(at, int) else getattr(_capi, at)) == off, name
        off += int(np.prod(shape))
    assert off == 646


# ------------------------------------------------------------ 6: build report
def test_fit_kernels_have_no_scratch_and_no_spills():
    import kernel_names
    from apg_trajectory_tracking_amd import build
    build.build()
    with open(build.RESOURCES) as f:
        res = json.load(f)
    mine = {k: v for k, v in res.items() if "cartpole_fit" in k}
    assert len([k for k in mine if "cartpole_fit_kernelILb" in k]) == 2, sorted(mine)
    assert len([k for k in mine if "cartpole_fit_reduce_kernel" in k]) == 1, sorted(mine)
    assert len(mine) == 3
    for k, v in mine.items():
        print(k, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        # the names the other resource tests count by substring stay theirs
        # (tests/test_cartpole_learnt_cpu.py finds its kernels by whole name)
        assert not any(s in k for s in ("wing_learnt_fit", "quad_learnt_fit")), k
    assert set(kernel_names.instances(mine, "cartpole_fit_kernel")) == {"ILb0E", "ILb1E"}
    assert set(kernel_names.instances(mine, "cartpole_fit_reduce_kernel")) == {""}
