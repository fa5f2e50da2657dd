"""Float64 / float32 restatement of the shooting MPC that plans through the
LEARNT simulator (include/apg.h: apg_quad_learnt_mpc_solve,
apg_quad_learnt_mpc_closed_loop) - the arbiter of
tests/test_quad_learnt_mpc_cpu.py and tests/test_gpu_quad_learnt_mpc.py.  It is
the rule of quad_mpc_restatement.solve_snapshots / closed_loop with the model a
`torch_port.LearntQuadOracle` in the requested dtype: cost
`torch_port.quad_mpc_loss` on the policy's action u, gradient torch autograd.

Every float64 run also yields a per-trajectory `kink` flag, as
tests/quad_loss_cases.learnt_oracle_run defines it: at some model step of some
iteration a hidden pre-activation has |z_j| < KINK (|b1_j| + sum_i |W1_ji|
|x_i|) - a float32 evaluation may take the other ReLU branch there, after which
its gradient is another one; such trajectories are set aside from the
comparisons, and their share is capped by the tests.

Not a test module (no test_ prefix); runs are cached, the CPU and the GPU tests
of one session share them."""
import ast
import ctypes
import functools

import numpy as np
import torch

import quad_mpc_restatement as R
from conftest import load_golden
from oracle import torch_port as tp
from quad_loss_cases import KINK, LEARNT_INIT, learnt_weights

H, DT = R.H, 0.1
F64, F32 = torch.float64, torch.float32
ITERS = (0, 1, 10, 20)
# kink share above which a run does not test what it is meant to (measured:
# 0.086 at 10 iterations, 0.199 at 20 on `golden`; 0.074 / 0.184 on `steps`)
MAX_KINK_SHARE = {0: 0.12, 1: 0.12, 10: 0.12, 20: 0.25}


class Traced:
    """A LearntQuadOracle that marks the trajectories on which a hidden
    pre-activation of ANY of its steps comes within KINK of zero."""

    def __init__(self, ora, B):
        self.ora, self.dtype = ora, ora.dtype
        self.kink = torch.zeros(B, dtype=torch.bool)

    def __call__(self, state, action, dt):
        ora = self.ora
        with torch.no_grad():
            s, a = state.detach().to(ora.dtype), action.detach().to(ora.dtype)
            x = torch.cat((s, (ora.A @ a.unsqueeze(2))[:, :, 0]), 1)
            z = x @ ora.w1.t() + ora.b1
            scale = ora.b1.abs() + x.abs() @ ora.w1.abs().t()
            self.kink.logical_or_((z.abs() < KINK * scale).any(1))
        return ora(state, action, dt)


@functools.lru_cache(maxsize=None)
def module_weights(which):
    """(weights, initial_params) of the weight set `which`: golden / steps -
    tests/golden/learnt_dynamics.npz (quad_loss_cases.learnt_weights, constructed
    with LEARNT_INIT); loop - the fitted simulator of closed_loop_learnt.npz with
    the `init` of the file; zero - a freshly constructed module."""
    if which == "loop":
        g = load_golden("closed_loop_learnt.npz")
        init = {kv.split("=")[0]: ast.literal_eval(kv.split("=")[1]) for kv in g["init"]}
        return {k[len("dyn."):]: g[k] for k in g.files if k.startswith("dyn.")}, init
    if which == "zero":
        z = lambda *s: np.zeros(s, dtype=np.float32)
        return {"linear_at": np.eye(4, dtype=np.float32),
                "linear_state_1.weight": z(64, 16), "linear_state_1.bias": z(64),
                "linear_state_2.weight": z(12, 64), "linear_state_2.bias": z(12)}, {}
    return learnt_weights(which), dict(LEARNT_INIT)


def oracle(which, dtype):
    weights, init = module_weights(which)
    return tp.LearntQuadOracle(weights, initial_params=init, dtype=dtype)


def solve_snapshots(dtype, model, state0, ref, u0, dt, snaps, beta=R.BETA,
                    alpha_thrust=R.ALPHA_THRUST, alpha_rate=R.ALPHA_RATE):
    """quad_mpc_restatement.solve_snapshots with the model a callable ->
    {iters: dict(u, cost, trace, kink)}: `kink` = the flags raised up to and
    including the cost evaluation of that snapshot."""
    traced = Traced(model, state0.shape[0])
    s0, r, u = state0.to(dtype), ref.to(dtype), u0.to(dtype).clone()
    alpha = torch.tensor([alpha_thrust, alpha_rate, alpha_rate, alpha_rate], dtype=dtype)
    m = torch.zeros_like(u)
    trace, out = [], {}
    for it in range(max(snaps) + 1):
        if it in snaps:
            J = R.cost(traced, s0, r, u, dt)
            out[it] = dict(u=u.clone(), cost=J, trace=torch.stack(trace + [J]),
                           kink=traced.kink.numpy().copy())
        if it == max(snaps):
            break
        J, g = R.cost_and_grad(traced, s0, r, u, dt)
        trace.append(J)
        m = beta * m + alpha * g
        u = (u - m).clamp(0.0, 1.0)
    return out


@functools.lru_cache(maxsize=None)
def windows(B=256):
    s0, ref = R.experiment_windows(B=B)
    return s0, ref, torch.full((B, H, 4), 0.5)


@functools.lru_cache(maxsize=None)
def solve_case(which, dtype, horizon=H, B=256):
    """Cases S1 (`golden`) and S2 (`steps`): experiment_windows(B), u0 = 0.5,
    dt 0.1 -> {iters: ...} for ITERS (one run of 20 iterations serves all)."""
    s0, ref, u0 = windows(B)
    return solve_snapshots(dtype, oracle(which, dtype), s0, ref[:, :horizon],
                           u0[:, :horizon], DT, ITERS)


def closed_loop(dtype, traj, dt, iters, max_steps, thresh_div, thresh_stable, test_time,
                plant, model):
    """quad_mpc_restatement.closed_loop with the solver's model a callable
    (LearntQuadOracle); plant: a dynamics callable.  -> its dict, without the
    probe."""
    B, L, _ = traj.shape
    ref = traj.to(dtype)
    T = min(max_steps, L + 1)
    state = torch.zeros(B, 12, dtype=dtype)
    state[:, :3] = ref[:, 0, :3]
    cur = 0
    alive = torch.ones(B, dtype=torch.bool)
    out = dict(drone=torch.zeros(B, T + 1, 12, dtype=dtype), div=torch.zeros(B, T, dtype=dtype),
               actions=torch.zeros(B, T, 4, dtype=dtype), cost=torch.zeros(B, T, dtype=dtype),
               steps=torch.zeros(B, dtype=torch.long), resets=0)
    out["drone"][:, 0] = state
    last = ref[:, -1, :3]
    u = torch.full((B, H, 4), 0.5, dtype=dtype)
    for i in range(T):
        if cur >= L - H:
            left = ref[:, cur:]
            pad = torch.zeros(B, H - (L - cur), 9, dtype=dtype)
            pad[:, :, :3] = last[:, None]
            window = torch.cat((left, pad), 1)
        else:
            window = ref[:, cur + 1:cur + H + 1]
            cur += 1
        if i > 0:
            u = R.shift(u)
        res = solve_snapshots(dtype, model, state, window, u, dt, (iters,))[iters]
        u = res["u"]
        action = u[:, 0]
        with torch.no_grad():
            new = plant(state.to(plant.dtype), action, dt).to(dtype)
        on_line = ref[:, cur, :3]
        div = torch.linalg.norm(on_line - new[:, :3], dim=1)
        stable = (new[:, 3:5].abs() < thresh_stable).all(1)
        rec = alive.clone()
        out["drone"][rec, i + 1] = new[rec]
        out["div"][rec, i] = div[rec]
        out["actions"][rec, i] = action[rec]
        out["cost"][rec, i] = res["cost"][rec]
        out["steps"][rec] = i + 1
        failed = (div > thresh_div) | ~stable
        out["resets"] += int((failed & rec).sum())
        if test_time:
            alive = alive & ~failed
            if not alive.any():
                break
        reset = torch.cat((ref[:, cur], torch.zeros(B, 3, dtype=dtype)), 1)
        state = torch.where((failed & (not test_time))[:, None], reset, new)
        if i >= L:
            break
    return out


def loop_trajectories(B, L=40):
    """quad_eval_trajectories(B, L, 0.1, seed=9) lifted 3 m."""
    from apg_trajectory_tracking_amd import synthetic
    traj = synthetic.quad_eval_trajectories(B, L, DT, seed=9)
    traj[:, :, 2] += 3
    return traj


@functools.lru_cache(maxsize=None)
def loop_case(plant, test_time, dtype=F64):
    """The closed-loop cases: B = 300, 30 steps, thresh_div 0.6, thresh_stable
    1, 10 iterations, the model the `loop` module; plant: "learnt" (the same
    module) or "drags" (analytic, quad_mpc_restatement.DRAGS)."""
    env = oracle("loop", dtype) if plant == "learnt" else tp.QuadOracle(R.DRAGS, dtype=dtype)
    return closed_loop(dtype, loop_trajectories(300), DT, 10, 30, 0.6, 1.0, test_time,
                       env, oracle("loop", dtype))


def same_flights(got_steps, got_div, ref, B, what):
    """The acceptance rule of the learnt-plant flights: same `steps` on > 97 %
    of the flights, `div` within 2e-3 on all but 3 % of those.  got_div [B,T]."""
    N = R.to_numpy
    same = [i for i in range(B) if int(got_steps[i]) == int(ref["steps"][i])]
    bad = [i for i in same
           if np.abs(N(got_div[i, :int(ref["steps"][i])])
                     - N(ref["div"][i, :int(ref["steps"][i])])).max() > 2e-3]
    print(what, "same steps: %d of %d, beyond 2e-3: %d, failed (flight, step) pairs of the "
          "restatement: %d" % (len(same), B, len(bad), ref["resets"]))
    assert len(same) > 0.97 * B, what
    assert len(bad) <= 0.03 * B, (what, len(bad))


# ---- the host twins (libapg_cpu.so) behind the restatement's tensors --------
def twins():
    from apg_trajectory_tracking_amd import _capi
    lib = R.twins()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    ptr = ctypes.POINTER
    lib.apg_quad_learnt_mpc_solve_cpu.argtypes = [
        P, P, I, F, ptr(_capi.ApgQuadParams), ptr(_capi.ApgLearntResidual),
        ptr(_capi.ApgQuadLossWeights), ptr(_capi.ApgQuadMpcOptions), I, I, P, P, P, P]
    lib.apg_quad_learnt_mpc_closed_loop_cpu.argtypes = [
        ptr(_capi.ApgQuadFlight), F, ptr(_capi.ApgQuadParams), ptr(_capi.ApgLearntResidual),
        ptr(_capi.ApgQuadParams), ptr(_capi.ApgLearntResidual), ptr(_capi.ApgQuadLossWeights),
        ptr(_capi.ApgQuadMpcOptions), I, I, P, P]
    return lib


def module(which, dev="cpu"):
    """The package's LearntDynamics carrying the weight set `which`."""
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    weights, init = module_weights(which)
    dyn = LearntDynamics(initial_params=dict(init))
    if which != "zero":
        dyn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    return dyn.to(dev)


def host_residual(dyn):
    """(ApgLearntResidual over the HOST tensors of `dyn`, what keeps them alive)."""
    from apg_trajectory_tracking_amd import _capi
    keep = [t.detach().float().contiguous() for t in (
        dyn.linear_at, dyn.linear_state_1.weight, dyn.linear_state_1.bias,
        dyn.linear_state_2.weight, dyn.linear_state_2.bias)]
    return _capi.ApgLearntResidual(*[t.data_ptr() for t in keep]), keep


def twin_solve(tw, dyn, state0, ref, u0, dt, iters):
    """apg_quad_learnt_mpc_solve_cpu on [B,12] / [B,H,C] / [B,H,4] float32
    tensors, the model the module `dyn` -> dict(u, cost, trace)."""
    from apg_trajectory_tracking_amd import functional as F
    B, Hh, C = ref.shape
    s = state0.float().t().contiguous()
    r = ref.float().permute(1, 2, 0).contiguous()
    u = u0.float().permute(1, 2, 0).contiguous()
    cost_out, trace = torch.zeros(B), torch.zeros(iters + 1, B)
    res, _keep = host_residual(dyn)
    rc = tw.apg_quad_learnt_mpc_solve_cpu(
        s.data_ptr(), r.data_ptr(), C, dt, ctypes.byref(dyn.params), ctypes.byref(res),
        ctypes.byref(F.quad_loss_weights()), ctypes.byref(R._options(iters)), B, Hh,
        u.data_ptr(), cost_out.data_ptr(), trace.data_ptr(), None)
    assert rc == 0, tw.apg_cpu_last_error_string()
    return dict(u=u.permute(2, 0, 1).contiguous(), cost=cost_out, trace=trace)


def twin_closed_loop(tw, traj, dt, iters, max_steps, thresh_div, thresh_stable, test_time,
                     plant_params, plant_dyn, model_dyn):
    """apg_quad_learnt_mpc_closed_loop_cpu -> the dict `closed_loop` returns.
    plant_dyn: a LearntDynamics module or None (the analytic plant on
    plant_params)."""
    from apg_trajectory_tracking_amd import _capi, functional as F
    B, L, _ = traj.shape
    T = min(max_steps, L + 1)
    tr = traj.float().permute(1, 2, 0).contiguous()
    div, cost_ = torch.zeros(T, B), torch.zeros(T, B)
    steps = torch.zeros(B, dtype=torch.int32)
    drone, actions, start = torch.zeros(T + 1, 12, B), torch.zeros(T, 4, B), torch.zeros(T, 12, B)
    flight = _capi.ApgQuadFlight(
        tr.data_ptr(), L, max_steps, thresh_div, thresh_stable, test_time, div.data_ptr(),
        steps.data_ptr(), drone.data_ptr(), actions.data_ptr(), start.data_ptr())
    model, _keep = host_residual(model_dyn)
    plant, _keep2 = host_residual(plant_dyn) if plant_dyn is not None else (None, None)
    rc = tw.apg_quad_learnt_mpc_closed_loop_cpu(
        ctypes.byref(flight), dt, ctypes.byref(plant_params),
        ctypes.byref(plant) if plant is not None else None, ctypes.byref(model_dyn.params),
        ctypes.byref(model), ctypes.byref(F.quad_loss_weights()),
        ctypes.byref(R._options(iters)), B, H, cost_.data_ptr(), None)
    assert rc == 0, tw.apg_cpu_last_error_string()
    return dict(div=div.t(), cost=cost_.t(), steps=steps.long(), drone=drone.permute(2, 0, 1),
                actions=actions.permute(2, 0, 1), start=start.permute(2, 0, 1))
