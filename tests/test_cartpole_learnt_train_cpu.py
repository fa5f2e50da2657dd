"""The fused controller step of the cart-pole through LearntCartpoleDynamics
without a GPU: the host twin of apg_cartpole_learnt_mlp_train_step
(include/apg_cpu_cartpole_learnt_train.h - the per-sample headers of the kernel,
csrc/cartpole_train_math.h and csrc/cartpole_learnt_math.h, looped over the
batch) against the recording of the REAL reference step (G20,
cartpole_learnt.npz: ctrl8.*, ctrl64.*), against a float64 restatement of the
whole step under autograd written here, against the analytic twin where the
simulator IS the analytic one, the argument checks, the ABI mirror, the new
kernel's resources as the build reports them and what the functional refuses.

Two simulators throughout: G20's fitted module, and a seeded module built by
the same recipe with other numbers - the six physical parameters moved
independently by a few percent (total_mass != masspole + masscart: the step
constants must come from all six) and the residual drawn large enough to matter
(at the init's std of 1e-4 it moves a state by 1e-8).

Bounds: the project's own - conftest.rel_err < 1e-4 on every gradient tensor,
the actions and the relative error of the loss.  Two conditions, not
tolerances, guard the float64 cases, both asserted in float64: no sample's
theta + dt theta_dot comes within 1e-4 rad of an odd multiple of pi at any step
(test_cartpole_train_cpu.py), and no pre-activation of the residual's hidden
layer lies within 1e-5 of zero - a relu that falls on different sides in
float32 and float64 moves one unit's whole contribution.  Every test prints
what it saw."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import test_cartpole_learnt_cpu as lref
import test_cartpole_train_cpu as ref
from conftest import REPO, load_golden, rel_err
from test_cartpole_train_cpu import tw  # noqa: F401  (the host twins, a fixture)

BAR, WRAP_MARGIN, RELU_MARGIN = ref.BAR, ref.WRAP_MARGIN, 1e-5
KERNEL = "cartpole_learnt_policy_kernel"
SIMULATORS = ("fitted", "seeded")
SHAPES = [(1, 5, .05), (8, 10, .05), (64, 5, .05), (67, 10, .05), (67, 1, .05),
          (67, 2, .05), (5, 33, .01), (3, 48, .01)]
# synthetic.cartpole_batch(B, H, seed = 100 + B) everywhere but where that batch
# misses one of the two conditions (tried on the CPU, in steps of 1000, until
# both margins were met twice over; the assertions stay in the test)
SEEDS = {("fitted", 64, 5, .05): 1164, ("fitted", 5, 33, .01): 1105,
         ("seeded", 64, 5, .05): 1164}


def simulator(kind):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    if kind == "fitted":
        return lref.fitted(lref.g20())
    torch.manual_seed(77)
    m = LearntCartpoleDynamics()
    with torch.no_grad():
        for k, f in zip(lref.PHYS, (1.04, .93, 1.06, .95, 1.03, .97)):
            m.cfg[k].mul_(f)
        m.linear_state_1.weight.normal_(0, .3)
        m.linear_state_1.bias.normal_(0, .2)
        m.linear_state_2.weight.normal_(0, .01)
    return m


def case(kind, B, H, dt):
    from apg_trajectory_tracking_amd import synthetic
    seed = SEEDS.get((kind, B, H, dt), 100 + B)
    return synthetic.cartpole_batch(B, H, seed=seed)["state0"].float().numpy()


def twin_step(tw, m, w, in_state, state0, dt, update=None):  # noqa: F811
    """ref.twin_step through the learnt twin: the module `m` as HOST arrays."""
    from apg_trajectory_tracking_amd import _capi
    x = np.ascontiguousarray(in_state, np.float32)
    s0 = np.ascontiguousarray(state0, np.float32)
    x_before = x.copy()
    B, H = x.shape[0], w["fc_out.bias"].shape[0]
    at, n = _capi.cartpole_policy_offsets(H)
    live = [w[k].copy() for k in ref.names()]
    pol = _capi.ApgCartpolePolicy(*[a.ctypes.data for a in live])
    flat = np.full(n + 1, np.nan, np.float32)
    g = {k: flat[o:o + int(np.prod(sh))].reshape(sh) for k, (o, sh) in at.items()}
    gs = ref.grads_struct([g[k] for k in ref.names()])
    parts = np.zeros(_capi.loss_partials_count(B), np.float32)
    loss = np.full(1, np.nan, np.float32)
    actions = np.full((B, H, 1), np.nan, np.float32)
    bufs = [np.zeros_like(a) for a in live]
    upd = None
    if update is not None:
        upd = ctypes.byref(_capi.ApgCartpoleSgdUpdate(
            update[0], update[1], ref.grads_struct(live), ref.grads_struct(bufs)))
    model = lref._Model(m)
    before = [a.copy() for a in model.arrays]
    rc = tw.apg_cartpole_learnt_mlp_train_step_cpu(
        ref.fp(x), ref.fp(s0), ctypes.c_float(dt), ctypes.byref(model.struct),
        ctypes.byref(pol), B, H, ref.fp(parts), ref.fp(loss), ctypes.byref(gs),
        ref.fp(actions), None, upd)
    assert rc == 0, (rc, tw.apg_cpu_last_error_string())
    assert np.array_equal(x, x_before)          # in_state is never written
    assert all(np.array_equal(a, b) for a, b in zip(model.arrays, before))   # nor the simulator
    assert np.isnan(flat[-1])                   # the loss slot is the caller's
    return dict(loss=float(loss[0]), flat=flat, g=g, actions=actions, parts=parts,
                w=dict(zip(ref.names(), live)), bufs=dict(zip(ref.names(), bufs)))


# ------------------------------------------------ the step, restated in float64
def module64(m):
    """(the six physical parameters as floats, W1, b1, W2 as float64 tensors)"""
    phys = [float(m.cfg[k].detach()) for k in lref.PHYS]
    return phys, [t.detach().double() for t in (
        m.linear_state_1.weight, m.linear_state_1.bias, m.linear_state_2.weight)]


def learnt_step64(phys, res, state, action, dt):
    """LearntCartpoleDynamics.forward written out: simulate_cartpole on the six
    live parameters (gravity 9.81) and the residual W2 relu(W1 [s; a] + b1).
    Returns (next state, the physics alone, the hidden pre-activations)."""
    F, mp, l, mu, tm, pml = phys
    W1, b1, W2 = res
    g = 9.81
    force = action[..., 0] * F * 0.5
    x_dot, theta, th_dot = state[..., 1], state[..., 2], state[..., 3]
    s, co = torch.sin(theta), torch.cos(theta)
    xacc = (-2 * pml * th_dot**2 * s + 3 * mp * g * s * co + 4 * force - 4 * mu * x_dot) / (
        4 * tm - 3 * mp * co**2)
    thacc = (-3 * pml * th_dot**2 * s * co + 6 * tm * g * s + 6 * (force - mu * x_dot) * co) / (
        4 * l * tm - 3 * pml * co**2)
    sd, cd = torch.sin(th_dot * dt), torch.cos(th_dot * dt)
    physics = torch.stack([state[..., 0] + x_dot * dt, x_dot + xacc * dt,
                           torch.atan2(s * cd + co * sd, co * cd - s * sd),
                           th_dot + thacc * dt], dim=-1)
    pre = torch.cat([state, action], dim=-1) @ W1.T + b1
    return physics + torch.relu(pre) @ W2.T, physics, pre


def oracle64(m, w, in_state, state0, dt):
    """The whole step in float64 under autograd: simple_model.Net (column 0
    zeroed), H learnt steps, oracle.torch_port's cartpole_reference and
    cartpole_loss_mpc.  Returns (loss, {name: gradient}, actions, the smallest
    distance of theta + dt theta_dot to an odd multiple of pi, the smallest
    |pre-activation| of the residual - both over all samples and steps)."""
    from oracle import torch_port as tp
    phys, res = module64(m)
    W = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    H = w["fc_out.bias"].shape[0]
    x = torch.tensor(in_state, dtype=torch.float64).clone()
    x[:, 0] = 0
    for l in ref.LAYERS:
        x = torch.tanh(x @ W[l + ".weight"].T + W[l + ".bias"])
    a = x.reshape(-1, H, 1)
    s0 = torch.tensor(state0, dtype=torch.float64)
    cur, states, wrap, kink = s0, [], math.inf, math.inf
    for k in range(H):
        with torch.no_grad():
            v = cur[:, 2] + dt * cur[:, 3]
            wrap = min(wrap, float(torch.abs(torch.remainder(v, 2 * math.pi) - math.pi).min()))
        cur, _, pre = learnt_step64(phys, res, cur, a[:, k], dt)
        kink = min(kink, float(pre.detach().abs().min()))
        states.append(cur)
    loss = tp.cartpole_loss_mpc(torch.stack(states, 1), tp.cartpole_reference(s0, H), a)
    loss.backward()
    return (float(loss.detach()), {k: W[k].grad.numpy() for k in W}, a.detach().numpy(),
            wrap, kink)


# ------------------------------------------------------------------ 1: golden
@pytest.mark.parametrize("B", [8, 64])
def test_golden_loss_and_every_gradient(tw, B):  # noqa: F811
    from test_cartpole_eval_cpu import golden_net
    g = lref.g20()
    net = golden_net(load_golden("cartpole_closed_loop.npz"), "shipped")
    w = {k: np.ascontiguousarray(v.detach().numpy(), np.float32)
         for k, v in net.named_parameters()}
    s = np.ascontiguousarray(g[f"ctrl{B}.state"], np.float32)
    got = twin_step(tw, lref.fitted(g), w, s, s, lref.DT)
    want = float(g[f"ctrl{B}.loss"])
    e_l = abs(got["loss"] - want) / abs(want)
    errs = {k: rel_err(got["g"][k], g[f"ctrl{B}.grad.{k}"]) for k in ref.names()}
    print(f"G20 ctrl{B} loss {got['loss']:.6g} rel {e_l:.2e} worst gradient "
          f"{max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert got["actions"].shape == (B, 10, 1)
    assert e_l < BAR
    for k, e in errs.items():
        assert e < BAR, (k, e)


# ----------------------------------------------------------------- 2: float64
def test_the_restated_step_against_the_recorded_forward():
    g = lref.g20()
    phys, res = module64(lref.fitted(g))
    s = torch.tensor(g["step.state"], dtype=torch.float64)
    a = torch.tensor(g["step.action"], dtype=torch.float64)
    full, physics, _ = learnt_step64(phys, res, s, a, lref.DT)
    lref.close(full.numpy(), g["step.forward"], 1e-6)
    lref.close(physics.numpy(), g["step.simulate"], 1e-6)


@pytest.mark.parametrize("kind", SIMULATORS)
@pytest.mark.parametrize("B,H,dt", SHAPES)
def test_twin_against_float64_oracle(tw, kind, B, H, dt):  # noqa: F811
    m, w, s0 = simulator(kind), ref.seeded_weights(H), case(kind, B, H, dt)
    loss64, want, acts64, wrap, kink = oracle64(m, w, s0, s0, dt)
    got = twin_step(tw, m, w, s0, s0, dt)
    errs = {k: rel_err(got["g"][k], want[k]) for k in ref.names()}
    e_loss = abs(got["loss"] - loss64) / abs(loss64)
    e_acts = rel_err(got["actions"], acts64)
    print(f"{kind} B={B} H={H} dt={dt} wrap margin {wrap:.3g} relu margin {kink:.3g} loss "
          f"{got['loss']:.6g} rel {e_loss:.2e} actions {e_acts:.2e} worst gradient "
          f"{max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert wrap >= WRAP_MARGIN, wrap
    assert kink >= RELU_MARGIN, kink
    assert e_acts < BAR and e_loss < BAR, (e_acts, e_loss)
    for k, e in errs.items():
        assert e < BAR, (k, e)
    assert got["parts"].shape[0] == (B + 63) // 64      # one partial per 64 samples
    assert abs(float(got["parts"].astype(np.float64).sum()) - got["loss"]) <= 1e-6 * abs(
        got["loss"])


# ------------------------------------------- 3: where the simulator is analytic
def test_zero_residual_and_default_parameters_give_the_analytic_twin_bit_for_bit(tw):  # noqa: F811
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    p = ref.default_params()
    f32 = np.float32
    values = dict(max_force_mag=p.max_force_mag, masspole=p.masspole, length=p.length,
                  friction=p.friction, total_mass=f32(p.masspole) + f32(p.masscart),
                  polemass_length=f32(p.masspole) * f32(p.length))
    assert f32(p.gravity) == f32(9.81)
    m = LearntCartpoleDynamics()
    with torch.no_grad():
        for k, v in values.items():
            m.cfg[k].fill_(float(v))
        for t in (m.linear_state_1.weight, m.linear_state_1.bias, m.linear_state_2.weight):
            t.zero_()
    for B, H, dt in [(67, 10, .05), (3, 48, .01)]:
        s0 = ref.case(B, H, dt)
        x = s0 * np.float32(.5)
        w = ref.seeded_weights(H)
        want = ref.twin_step(tw, w, x, s0, dt, update=(1e-4, .9))
        got = twin_step(tw, m, w, x, s0, dt, update=(1e-4, .9))
        assert got["loss"] == want["loss"] and got["loss"] > 0
        assert np.array_equal(got["flat"][:-1], want["flat"][:-1])
        assert np.array_equal(got["actions"], want["actions"])
        assert np.array_equal(got["parts"], want["parts"])
        for k in ref.names():
            assert np.array_equal(got["w"][k], want["w"][k]), k
            assert np.array_equal(got["bufs"][k], want["bufs"][k]), k
    # ... and a simulator that is not: the result moves
    assert twin_step(tw, simulator("seeded"), w, x, s0, dt)["loss"] != want["loss"]


def test_the_update_is_momentum_sgd_on_the_policy_alone(tw):  # noqa: F811
    B, H, dt = 8, 10, .05
    m, w, s0 = simulator("fitted"), ref.seeded_weights(H), case("fitted", B, H, dt)
    plain = twin_step(tw, m, w, s0, s0, dt)
    got = twin_step(tw, m, w, s0, s0, dt, update=(1e-4, .9))
    assert np.array_equal(got["flat"][:-1], plain["flat"][:-1]) and got["loss"] == plain["loss"]
    for k in ref.names():
        assert np.array_equal(got["bufs"][k], got["g"][k]), k
        want = (w[k].astype(np.float64) - 1e-4 * got["g"][k].astype(np.float64)).astype(
            np.float32)
        assert np.array_equal(got["w"][k], want) and not np.array_equal(want, w[k]), k


# ----------------------------------------------------------- 4: argument errors
def test_argument_errors_before_anything_runs(tw):  # noqa: F811
    from apg_trajectory_tracking_amd import _capi
    H, B = 5, 8
    w = ref.seeded_weights(H)
    live = [w[k].copy() for k in ref.names()]
    s = ref.case(B, H, .05)
    at, n = _capi.cartpole_policy_offsets(H)
    flat = np.full(n, 7.0, np.float32)
    gl = [flat[o:o + int(np.prod(sh))] for o, sh in at.values()]
    bufs = [np.zeros_like(a) for a in live]
    parts, loss = np.zeros(1, np.float32), np.full(1, 7.0, np.float32)
    model = lref._Model(simulator("fitted"))
    pol = _capi.ApgCartpolePolicy(*[a.ctypes.data for a in live])
    lib = _capi.lib()

    def call(fn, stream, B=B, H=H, x=s, s0=s, model=model.struct, pol=pol, parts=parts,
             gs=ref.grads_struct(gl), upd=None):
        # (host addresses on the device side too: every bad call must fail before
        # it touches them)
        return fn(ref.fp(x), ref.fp(s0), ctypes.c_float(.05),
                  None if model is None else ctypes.byref(model),
                  None if pol is None else ctypes.byref(pol), B, H, ref.fp(parts),
                  ref.fp(loss), None if gs is None else ctypes.byref(gs), None,
                  None if parts is None else ref.fp(flat),
                  None if upd is None else ctypes.byref(upd), *stream)

    host = lambda **kw: call(tw.apg_cartpole_learnt_mlp_train_step_cpu, (), **kw)
    dev = lambda **kw: call(lib.apg_cartpole_learnt_mlp_train_step, (None,), **kw)

    def without(field):
        ptrs = {f: getattr(model.struct, f) for f, _ in _capi.ApgCartpoleLearnt._fields_}
        ptrs[field] = None
        return dict(model=_capi.ApgCartpoleLearnt(**ptrs))

    def update(lr=1e-4, param=live, buf=bufs, drop=None):
        ptrs = [[a.ctypes.data for a in param], [a.ctypes.data for a in buf]]
        if drop is not None:
            ptrs[drop[0]][drop[1]] = None
        return dict(upd=_capi.ApgCartpoleSgdUpdate(
            lr, .9, _capi.ApgCartpolePolicyGrads(*ptrs[0]),
            _capi.ApgCartpolePolicyGrads(*ptrs[1])))
    bad = [dict(model=None), without("w1"), without("b1"), without("w2"), without("length"),
           dict(H=0), dict(H=49), dict(B=0), dict(B=-3), dict(x=None), dict(s0=None),
           dict(pol=None), dict(parts=None), dict(gs=None), update(lr=float("nan")),
           update(drop=(0, 3)), update(drop=(1, 9))]
    for fn in (host, dev):
        for kw in bad:
            assert fn(**kw) == -1, sorted(kw)
    assert dev(H=49) == -1 and b"H must be" in lib.apg_last_error_string()
    assert dev(B=0) == -1 and b"B must be" in lib.apg_last_error_string()
    assert dev(**without("b1")) == -1 and b"w1 / b1 / w2" in lib.apg_last_error_string()
    assert dev(**update(drop=(1, 7))) == -1 and b"update" in lib.apg_last_error_string()
    assert np.all(flat == 7.0) and loss[0] == 7.0          # nothing ran
    assert all(np.array_equal(a, w[k]) for a, k in zip(live, ref.names()))
    assert host() == 0 and loss[0] != 7.0 and not np.any(flat == 7.0)


# --------------------------------------------------------------- 5: signatures
def test_the_twin_and_capi_repeat_the_device_signature(tw):  # noqa: F811
    from apg_trajectory_tracking_amd import _capi
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    cpu = open(os.path.join(REPO, "include", "apg_cpu_cartpole_learnt_train.h")).read()
    gpu = open(os.path.join(REPO, "include", "apg.h")).read()
    decls = re.findall(r"\bint\s+(apg_\w+_cpu)\s*\(([^;]*?)\)\s*;", cpu, re.S)
    assert [d[0] for d in decls] == ["apg_cartpole_learnt_mlp_train_step_cpu"]
    name, args = decls[0]
    assert hasattr(tw, name)
    m = re.search(r"\bint\s+" + name[:-4] + r"\s*\(([^;]*?)\)\s*;", gpu, re.S)
    dev_args = norm(m.group(1))
    assert dev_args.endswith(", apg_stream_t stream")
    assert norm(args) == dev_args[:-len(", apg_stream_t stream")]
    # the analytic entry point's list with the simulator swapped
    ana = norm(re.search(r"\bint\s+apg_cartpole_mlp_train_step\s*\(([^;]*?)\)\s*;", gpu,
                         re.S).group(1))
    assert dev_args == ana.replace("const ApgCartpoleParams *params",
                                   "const ApgCartpoleLearnt *model")
    kinds = {"const float *": ctypes.c_void_p, "float *": ctypes.c_void_p,
             "float": ctypes.c_float, "int": ctypes.c_int, "apg_stream_t": ctypes.c_void_p,
             "const ApgCartpoleLearnt *": ctypes.POINTER(_capi.ApgCartpoleLearnt),
             "const ApgCartpolePolicy *": ctypes.POINTER(_capi.ApgCartpolePolicy),
             "const ApgCartpolePolicyGrads *": ctypes.POINTER(_capi.ApgCartpolePolicyGrads),
             "const ApgCartpoleSgdUpdate *": ctypes.POINTER(_capi.ApgCartpoleSgdUpdate)}
    want = [kinds[norm(re.match(r"(.*?)(\w+)$", norm(a)).group(1))] for a in dev_args.split(",")]
    assert _capi.SIGNATURES["apg_cartpole_learnt_mlp_train_step"] == want


# ---------------------------------------------------------------- 6: resources
def test_the_kernel_has_no_scratch_and_the_resources_design_md_states():
    from apg_trajectory_tracking_amd import build
    build.build()
    with open(build.RESOURCES) as f:
        res = json.load(f)
    mine = [v for k, v in res.items() if KERNEL in k]
    assert len(mine) == 1, [k for k in res if KERNEL in k]
    r = mine[0]
    print(KERNEL, r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    sec = design[design.index("cart-pole controller step through the learnt simulator"):]
    stated = re.search(KERNEL + r":\s+(\d+)\s+VGPRs,\s+(\d+)\s+AGPRs,\s+(\d+)\s+SGPRs,\s+"
                       r"occupancy\s+(\d+)", sec)
    assert stated, "DESIGN.md states the kernel's resources"
    assert (r["vgprs"], r["agprs"], r["sgprs"], r["occupancy"]) == tuple(
        map(int, stated.groups()))
    # a workgroup's dynamic LDS: the analytic step's and the residual's 640 floats
    lds = lambda H: 4 * ((196 + H) * 65 + 4 * H * 64) + 2560
    assert (lds(10), lds(48)) == (66360, 115152)
    for H in (10, 48):
        assert f"{lds(H):,}".replace(",", " ") + " B" in sec, H
    assert lds(48) <= 160 * 1024


# ---------------------------------------------------------------- 7: refusals
def test_functional_refuses_what_the_step_does_not_serve():
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    from apg_trajectory_tracking_amd.models.simple_model import Net

    class Other(Net):
        pass

    class WithBias(LearntCartpoleDynamics):
        pass
    x = torch.zeros(2, 4)
    biased = LearntCartpoleDynamics()
    biased.linear_state_2 = torch.nn.Linear(64, 4, bias=True)
    assert not F.cartpole_learnt_fusable(biased)
    for net, dyn in [(Other(4, 5), LearntCartpoleDynamics()),      # a non-stock policy
                     (Net(4, 5), biased),                          # a residual output bias
                     (Net(4, 5), WithBias()),                      # a non-stock simulator
                     (Net(4, 5), LearntCartpoleDynamics())]:       # host tensors
        with pytest.raises(ValueError):
            F.cartpole_learnt_policy_train_step(net, dyn, x, x, .05)
    # the analytic step's functional is a function of its own
    assert F.cartpole_learnt_policy_train_step is not F.cartpole_policy_train_step


def test_the_trainer_keeps_the_tape_unless_told_otherwise():
    from apg_trajectory_tracking_amd import train_cartpole as tc
    import inspect
    assert tc.TrainCartpole.fused_learnt_policy is False
    sig = inspect.signature(tc.train_norm_dynamics)
    assert sig.parameters["fused_learnt_policy"].default is False
