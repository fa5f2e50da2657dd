"""Float64 / float32 restatement of the batched cart-pole shooting MPC
(include/apg.h: apg_cartpole_mpc_solve, apg_cartpole_mpc_closed_loop) - the
arbiter of tests/test_cartpole_mpc_cpu.py and tests/test_gpu_cartpole_mpc.py.
Written from the ALGORITHM, not from the package: the model is
`oracle.torch_port.CartpoleOracle` with the angle advanced as theta + dt
theta_dot (no atan2 wrap inside the horizon), the cost
`torch_port.cartpole_loss_mpc` on `torch_port.cartpole_reference`, the gradient
torch autograd.

    for it in range(iters):
        J = cartpole_loss_mpc(unroll(model, state0, u), reference(state0), u)
        g = dJ/du
        m = beta * m + alpha * g          # beta 0.5, alpha 5e-4
        u = clamp(u - m, -1, 1)
    J = cost of the returned u

The closed loop steps the WRAPPED oracle as plant, then CartPoleEnv._step's
theta wrap, with the bookkeeping of scripts/evaluate_cartpole.py:79-318.

Not a test module (no test_ prefix); shared by the CPU and the GPU tests and by
tools/time_cartpole_mpc.py's sanity check."""
import ctypes
import functools
import math

import numpy as np
import torch

from oracle import torch_port as tp

BETA, ALPHA = 0.5, 5e-4
H = 10
MISMATCH = {"masspole": 0.2, "length": 0.7}
LIMITS = torch.tensor([2.4, 7.5, math.pi, 7.5])
W = (0.0, 3.0, 10.0, 1.0)


# ---- the model -----------------------------------------------------------------
def model_step(oracle, state, action, dt, wrapped=False):
    """The oracle's step; wrapped False: its theta replaced by theta + dt theta_dot."""
    nxt = oracle(state, action, dt)
    if wrapped:
        return nxt
    st = state.to(nxt.dtype)
    return torch.stack([nxt[..., 0], nxt[..., 1], st[..., 2] + dt * st[..., 3], nxt[..., 3]], -1)


def unroll(oracle, state0, u, dt, wrapped=False):
    cur, out = state0, []
    for k in range(u.shape[1]):
        cur = model_step(oracle, cur, u[:, k], dt, wrapped)
        out.append(cur)
    return torch.stack(out, 1)


def per_trajectory_cost(states, ref, u):
    """cartpole_loss_mpc with the batch axis kept: [B]."""
    w = torch.tensor(W, dtype=states.dtype)
    return (((states - ref)**2) * w).sum((1, 2)) + 0.01 * (u**2).sum((1, 2))


def cost_and_grad(oracle, state0, u, dt, wrapped=False):
    """(J [B], dJ/du [B,H,1]); the scalar differentiated is torch_port's own
    cartpole_loss_mpc over the batch (trajectories are independent)."""
    a = u.detach().clone().requires_grad_(True)
    ref = tp.cartpole_reference(state0, u.shape[1])
    states = unroll(oracle, state0, a, dt, wrapped)
    total = tp.cartpole_loss_mpc(states, ref, a)
    total.backward()
    J = per_trajectory_cost(states.detach(), ref, a.detach())
    total = float(total.detach())
    assert abs(float(J.sum()) - total) <= 1e-4 * abs(total) + 1e-12
    return J, a.grad


def cost(oracle, state0, u, dt, wrapped=False):
    with torch.no_grad():
        return per_trajectory_cost(unroll(oracle, state0, u, dt, wrapped),
                                   tp.cartpole_reference(state0, u.shape[1]), u)


# ---- the solver ----------------------------------------------------------------
def solve_snapshots(dtype, state0, u0, dt, snaps, modified_params=None, beta=BETA,
                    alpha=ALPHA, wrapped=False):
    """One run of max(snaps) iterations -> {iters: what `solve` returns for that
    many iterations} (the iterates of a shorter solve are a prefix of a longer
    one's)."""
    oracle = tp.CartpoleOracle(modified_params, dtype=dtype)
    s0, u = state0.to(dtype), u0.to(dtype).clone()
    m = torch.zeros_like(u)
    trace, out = [], {}
    for it in range(max(snaps) + 1):
        if it in snaps:
            J = cost(oracle, s0, u, dt, wrapped)
            out[it] = dict(u=u.clone(), cost=J, trace=torch.stack(trace + [J]))
        if it == max(snaps):
            break
        J, g = cost_and_grad(oracle, s0, u, dt, wrapped)
        trace.append(J)
        m = beta * m + alpha * g
        u = (u - m).clamp(-1.0, 1.0)
    return out


def solve(dtype, state0, u0, dt, iters, modified_params=None, **rule):
    """-> dict(u [B,H,1], cost [B], trace [iters+1,B]) in `dtype`."""
    return solve_snapshots(dtype, state0, u0, dt, (iters,), modified_params, **rule)[iters]


def shift(u):
    return torch.cat((u[:, 1:], u[:, -1:]), 1)


def projected_gradient_norm(state0, u, dt, modified_params=None):
    """Norm over the batch of the float64 gradient at `u` with the components
    that point out of the box at an active bound removed."""
    oracle = tp.CartpoleOracle(modified_params, dtype=torch.float64)
    u = u.to(torch.float64)
    _, g = cost_and_grad(oracle, state0.to(torch.float64), u, dt)
    out = ((u <= -1.0) & (g > 0)) | ((u >= 1.0) & (g < 0))
    return float(torch.where(out, torch.zeros_like(g), g).norm())


# ---- the draws -----------------------------------------------------------------
def near_upright(B, gen):
    return (torch.rand(B, 4, generator=gen) - .5) * torch.tensor([.6, .6, .4, .6])


def full_range(B, gen):
    return (torch.rand(B, 4, generator=gen) * 2 - 1) * LIMITS


def swingup(B, gen):
    """CartPoleEnv._reset_swingup's distribution."""
    s = (torch.rand(B, 4, generator=gen) * 2 - 1) * LIMITS
    s[:, 0] = 0
    s[:, 1] *= 0.1
    sign = torch.where(torch.rand(B, generator=gen) > .5, -1.0, 1.0)
    s[:, 2] = sign * (2.8 + torch.rand(B, generator=gen) * .3)
    s[:, 3] *= 0.1
    return s


def thirds(B, seed=11):
    """near-upright | full range | swing-up starts, a third each: [B,4] float32
    and the three slices."""
    gen = torch.Generator().manual_seed(seed)
    n = B // 3
    parts = [near_upright(n, gen), full_range(n, gen), swingup(B - 2 * n, gen)]
    return torch.cat(parts).float(), (slice(0, n), slice(n, 2 * n), slice(2 * n, B))


def balance_starts(B=64, seed=5):
    """Near-upright starts (theta within +-0.1) plus a quarter that leaves
    (-0.21, 0.21) within a few steps whatever the controller does: theta =
    +-0.19 with theta_dot = +-3 outwards."""
    gen = torch.Generator().manual_seed(seed)
    s = (torch.rand(B, 4, generator=gen) - .5) * torch.tensor([.6, .6, .2, .6])
    n = B // 4
    sign = torch.where(torch.rand(n, generator=gen) > .5, -1.0, 1.0)
    s[:n, 2] = sign * 0.19
    s[:n, 3] = sign * 3.0
    return s.float()


# ---- the closed loop -----------------------------------------------------------
def env_wrap(theta):
    """CartPoleEnv._step: both comparisons with the original theta."""
    out = torch.where(theta > math.pi, theta - 2 * math.pi, theta)
    return torch.where(theta <= -math.pi, 2 * math.pi + theta, out)


def closed_loop(dtype, state0, dt, iters, max_steps, mode, thresh_div=0.21, burn_in=50,
                plant=None, model_params=None, horizon=H, probe=False):
    """scripts/evaluate_cartpole.py's loops with the policy replaced by "shift the
    warm start, solve, apply u[0]" (first step from u = 0; the cart position is
    not zeroed).  plant: callable (state, action, dt) -> next state (default the
    nominal wrapped CartpoleOracle in `dtype`).  -> dict(states [B,T,4], actions
    [B,T], cost [B,T] (rows of steps not taken: 0), steps [B], upright [B],
    vel_sum / vel_sq [B] float64, wraps [B]: the plant's angle wrapped at least
    once, margin: the smallest distance of a recorded |theta| to thresh_div)."""
    B, T = state0.shape[0], max_steps
    plant = plant if plant is not None else tp.CartpoleOracle(dtype=dtype)
    s = state0.to(dtype)
    u = torch.zeros(B, horizon, 1, dtype=dtype)
    alive = torch.ones(B, dtype=torch.bool)
    out = dict(states=torch.zeros(B, T, 4, dtype=dtype), actions=torch.zeros(B, T, dtype=dtype),
               cost=torch.zeros(B, T, dtype=dtype), steps=torch.zeros(B, dtype=torch.long),
               upright=torch.ones(B, dtype=torch.bool),
               vel_sum=torch.zeros(B, dtype=torch.float64),
               vel_sq=torch.zeros(B, dtype=torch.float64),
               wraps=torch.zeros(B, dtype=torch.bool), margin=float("inf"), start=[], plans=[])
    for i in range(T):
        if i > 0:
            u = shift(u)
        if probe and i < 2:
            out["start"].append(s.clone())
        res = solve(dtype, s, u, dt, iters, model_params)
        u = res["u"]
        if probe and i < 2:
            out["plans"].append(u.clone())
        action = u[:, 0]
        with torch.no_grad():
            new = plant(s, action, dt).to(dtype)
        out["wraps"] |= (new[:, 2] - s[:, 2]).abs() > 3.0
        new = torch.stack([new[:, 0], new[:, 1], env_wrap(new[:, 2]), new[:, 3]], 1)
        rec = alive.clone()
        out["states"][rec, i] = new[rec]
        out["actions"][rec, i] = action[rec, 0]
        out["cost"][rec, i] = res["cost"][rec]
        out["steps"][rec] = i + 1
        v = new[:, 1].abs().double()
        if mode == "swingup":
            if i > burn_in:
                out["vel_sum"] += v
                out["vel_sq"] += v * v
                out["upright"] &= ~(new[:, 2] > 1.0)
        else:
            out["vel_sum"] += torch.where(rec, v, torch.zeros_like(v))
            out["vel_sq"] += torch.where(rec, v * v, torch.zeros_like(v))
            inside = (new[:, 2] > -thresh_div) & (new[:, 2] < thresh_div)
            if rec.any():
                out["margin"] = min(out["margin"],
                                    float((new[rec, 2].abs() - thresh_div).abs().min()))
            out["upright"] &= ~(rec & ~inside)
            alive = alive & inside
            if not alive.any():
                break
        s = new
    return out


@functools.lru_cache(maxsize=None)
def balance_case(dtype, mismatch, B=64, steps=60, iters=10):
    """The balance cases of the tests (nominal / plant mismatch), cached: the
    CPU and the GPU tests of one session share the restatement's runs."""
    s0 = balance_starts(B)
    plant = tp.CartpoleOracle(MISMATCH if mismatch else None, dtype=dtype)
    return s0, closed_loop(dtype, s0, 0.05, iters, steps, "balance", 0.21, 0, plant=plant)


@functools.lru_cache(maxsize=None)
def swingup_case(dtype, B=256, steps=30, burn_in=10, iters=10):
    gen = torch.Generator().manual_seed(17)
    s0 = swingup(B, gen).float()
    return s0, closed_loop(dtype, s0, 0.05, iters, steps, "swingup", 0.21, burn_in)


@functools.lru_cache(maxsize=None)
def solve_case(dtype, B=256):
    """Test 1's starts and ONE restated run of 20 iterations serving the three
    iteration counts."""
    s0, parts = thirds(B)
    return s0, parts, solve_snapshots(dtype, s0, torch.zeros(B, H, 1), 0.05, (1, 10, 20))


class LearntPlant:
    """LearntCartpoleDynamics.forward restated on the oracle: the physics on
    the module's six live parameters plus W2 relu(W1 [s; a] + b1)."""

    def __init__(self, module, dtype):
        self.dtype = dtype
        self.oracle = tp.CartpoleOracle(dtype=dtype)
        for k in ("max_force_mag", "masspole", "length", "friction", "total_mass",
                  "polemass_length"):
            self.oracle.cfg[k] = float(module.cfg[k].detach().double())
        self.w1 = module.linear_state_1.weight.detach().cpu().to(dtype)
        self.b1 = module.linear_state_1.bias.detach().cpu().to(dtype)
        self.w2 = module.linear_state_2.weight.detach().cpu().to(dtype)

    def __call__(self, state, action, dt):
        z = torch.cat((state.to(self.dtype), action.to(self.dtype)), 1)
        return self.oracle(state, action, dt) + torch.relu(z @ self.w1.t() + self.b1) @ self.w2.t()


# ---- the host twins (libapg_cpu.so) behind the restatement's tensors -----------
def twins():
    from apg_trajectory_tracking_amd import _capi, build as b
    lib = ctypes.CDLL(b.build_cpu())
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    PP = ctypes.POINTER(_capi.ApgCartpoleParams)
    PO = ctypes.POINTER(_capi.ApgCartpoleMpcOptions)
    lib.apg_cartpole_mpc_solve_cpu.argtypes = [P, P, F, PP, PO, I, I, P, P, P]
    lib.apg_cartpole_mpc_closed_loop_cpu.argtypes = [
        ctypes.POINTER(_capi.ApgCartpoleFlight), F, PP, ctypes.POINTER(_capi.ApgCartpoleLearnt),
        PP, PO, I, I, P]
    lib.apg_cpu_last_error_string.restype = ctypes.c_char_p
    return lib


def params(modified=None):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    return CartpoleDynamics(modified or {}).params


def options(iters, beta=BETA, alpha=ALPHA):
    from apg_trajectory_tracking_amd import _capi
    return _capi.ApgCartpoleMpcOptions(int(iters), beta, alpha)


def twin_solve(tw, state0, u0, dt, iters, modified_params=None, horizon=H, opt=None):
    """apg_cartpole_mpc_solve_cpu on [B,4] / [B,H,1] (or None) float32 tensors ->
    dict(u, cost, trace) as `solve` returns them."""
    B = state0.shape[0]
    s = state0.float().t().contiguous()
    start = None if u0 is None else u0.float()[:, :, 0].t().contiguous()
    u, cost_out, trace = torch.zeros(horizon, B), torch.zeros(B), torch.zeros(iters + 1, B)
    rc = tw.apg_cartpole_mpc_solve_cpu(
        s.data_ptr(), None if start is None else start.data_ptr(), dt,
        ctypes.byref(params(modified_params)), ctypes.byref(opt or options(iters)), B, horizon,
        u.data_ptr(), cost_out.data_ptr(), trace.data_ptr())
    assert rc == 0, tw.apg_cpu_last_error_string()
    return dict(u=u.t().contiguous()[:, :, None], cost=cost_out, trace=trace)


def twin_closed_loop(tw, state0, dt, iters, max_steps, mode, thresh_div=0.21, burn_in=50,
                     plant_params=None, model_params=None, horizon=H, want_trajectory=True):
    """apg_cartpole_mpc_closed_loop_cpu -> the dict `closed_loop` returns ([B, ...]).
    want_trajectory False: states / actions are passed as NULL (and come back zero)."""
    B, T = state0.shape[0], max_steps
    s = state0.float().t().contiguous()
    steps, upright = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    vs, vq = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    states, actions, cost_ = torch.zeros(T, 4, B), torch.zeros(T, B), torch.zeros(T, B)
    from apg_trajectory_tracking_amd import _capi
    flight = _capi.ApgCartpoleFlight(
        state0=s.data_ptr(), max_steps=T, mode={"balance": 0, "swingup": 1}[mode],
        thresh_div=thresh_div, burn_in=burn_in, steps=steps.data_ptr(),
        upright=upright.data_ptr(), vel_sum=vs.data_ptr(), vel_sq=vq.data_ptr(),
        states=states.data_ptr() if want_trajectory else None,
        actions=actions.data_ptr() if want_trajectory else None)
    rc = tw.apg_cartpole_mpc_closed_loop_cpu(
        ctypes.byref(flight), dt, ctypes.byref(params(plant_params)), None,
        ctypes.byref(params(model_params)), ctypes.byref(options(iters)), B, horizon,
        cost_.data_ptr())
    assert rc == 0, tw.apg_cpu_last_error_string()
    return from_device_layout(dict(steps=steps, upright=upright, vel_sum=vs, vel_sq=vq,
                                   states=states, actions=actions, cost=cost_))


def from_device_layout(o):
    """The kernel's / twin's outputs ([T,4,B], [T,B]) -> the restatement's
    ([B,T,4], [B,T])."""
    return dict(steps=o["steps"].cpu().long(), upright=o["upright"].cpu().bool(),
                vel_sum=o["vel_sum"].cpu(), vel_sq=o["vel_sq"].cpu(),
                states=o["states"].cpu().permute(2, 0, 1), actions=o["actions"].cpu().t(),
                cost=o["cost"].cpu().t())


def to_numpy(x):
    return np.asarray(x.detach().cpu(), dtype=np.float64)
