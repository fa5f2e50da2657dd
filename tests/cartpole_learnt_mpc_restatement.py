"""Float64 / float32 restatement of the cart-pole shooting MPC that plans
through the learnt simulator (include/apg.h: apg_cartpole_learnt_mpc_solve,
apg_cartpole_learnt_mpc_closed_loop) - the arbiter of
tests/test_cartpole_learnt_mpc_cpu.py and tests/test_gpu_cartpole_learnt_mpc.py.
Written from the ALGORITHM, not from the package.  The model inside the horizon:

    s' = step(s, a) + W2 relu(W1 [s; a] + b1)

`step` is cartpole_mpc_restatement.LearntPlant's oracle (CartpoleOracle on the
module's six live parameters) with its theta replaced by theta + dt theta_dot;
the residual is evaluated on the pre-step state and the raw action and added to
all four components, theta included (so this does NOT route through
R.model_step, which overwrites theta' after the fact and would drop the
residual's theta row).  Cost, reference, update rule, box and warm start are
cartpole_mpc_restatement's; the gradient is torch autograd.

A closed loop takes two callables (state, action, dt) -> next state: `model`,
what the solver differentiates through, and `plant`, what the environment steps
with (R.LearntPlant: the wrapped step plus the residual).

Not a test module (no test_ prefix); shared by the CPU and the GPU tests."""
import ctypes
import functools

import numpy as np
import torch

import cartpole_mpc_restatement as R
from oracle import torch_port as tp

BETA, ALPHA = R.BETA, R.ALPHA
H = R.H
DT = 0.05
# A hidden pre-activation with |z_j| < KINK (|b1_j| + sum_i |W1_ji| |x_i|) - about
# a hundred float32 roundings of the sum's terms - may fall on the other ReLU
# branch in a float32 evaluation; the gradient is another one from there on (the
# rule of tests/quad_loss_cases.py for the quadrotor's learnt model).
KINK = 1e-5
PHYS = ("max_force_mag", "masspole", "length", "friction", "total_mass", "polemass_length")


# ---- the modules -----------------------------------------------------------------
def module(which="fitted"):
    """The ONE instance of a module per name (see _module)."""
    return _module(which)


@functools.lru_cache(maxsize=None)
def _module(which):
    """fitted: the fitted module of tests/golden/cartpole_learnt.npz.  second:
    the same with length 0.7 and the residual's output layer halved.  zero: a
    freshly constructed module with its three residual tensors zeroed (the
    nominal physics)."""
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import LearntCartpoleDynamics
    from test_cartpole_learnt_cpu import fitted, g20
    if which == "zero":
        m = LearntCartpoleDynamics()
        with torch.no_grad():
            m.linear_state_1.weight.zero_()
            m.linear_state_1.bias.zero_()
            m.linear_state_2.weight.zero_()
        return m
    m = fitted(g20())
    if which == "second":
        with torch.no_grad():
            m.cfg["length"].fill_(0.7)
            m.linear_state_2.weight.mul_(0.5)
    return m


# ---- the model -------------------------------------------------------------------
class LearntModel:
    """The planning model over R.LearntPlant's oracle and weights.  wrapped: the
    oracle's own (atan2) theta; theta_row False: the residual's theta component
    dropped - both only to show that the code under test does neither."""

    def __init__(self, mod, dtype, wrapped=False, theta_row=True):
        self.p = R.LearntPlant(mod, dtype)
        self.dtype, self.wrapped = dtype, wrapped
        self.keep = torch.tensor([1.0, 1.0, 1.0 if theta_row else 0.0, 1.0], dtype=dtype)
        self.kink = None       # [B] bool once watch(B) was called

    def watch(self, B):
        """From now on mark the trajectories on which a hidden pre-activation of
        ANY step comes within KINK of zero."""
        self.kink = torch.zeros(B, dtype=torch.bool)
        return self

    def __call__(self, state, action, dt):
        p = self.p
        st, a = state.to(self.dtype), action.to(self.dtype)
        nxt = p.oracle(st, a, dt)
        if not self.wrapped:
            nxt = torch.stack([nxt[..., 0], nxt[..., 1], st[..., 2] + dt * st[..., 3],
                               nxt[..., 3]], -1)
        z = torch.cat((st, a), 1)
        pre = z @ p.w1.t() + p.b1
        if self.kink is not None:
            with torch.no_grad():
                scale = p.b1.abs() + z.abs() @ p.w1.abs().t()
                self.kink.logical_or_((pre.abs() < KINK * scale).any(1))
        return nxt + (torch.relu(pre) @ p.w2.t()) * self.keep


class NominalModel:
    """The analytic solver's model (R.model_step on the nominal oracle)."""

    def __init__(self, dtype, modified_params=None):
        self.oracle = tp.CartpoleOracle(modified_params, dtype=dtype)

    def __call__(self, state, action, dt):
        return R.model_step(self.oracle, state, action, dt)


def unroll(model, state0, u, dt):
    cur, out = state0, []
    for k in range(u.shape[1]):
        cur = model(cur, u[:, k], dt)
        out.append(cur)
    return torch.stack(out, 1)


def cost_and_grad(model, state0, u, dt):
    """(J [B], dJ/du [B,H,1]): torch_port's cartpole_loss_mpc over the batch."""
    a = u.detach().clone().requires_grad_(True)
    ref = tp.cartpole_reference(state0, u.shape[1])
    states = unroll(model, state0, a, dt)
    tp.cartpole_loss_mpc(states, ref, a).backward()
    return R.per_trajectory_cost(states.detach(), ref, a.detach()), a.grad


def cost(model, state0, u, dt):
    with torch.no_grad():
        return R.per_trajectory_cost(unroll(model, state0, u, dt),
                                     tp.cartpole_reference(state0, u.shape[1]), u)


# ---- the solver ------------------------------------------------------------------
def solve_snapshots(model, dtype, state0, u0, dt, snaps, beta=BETA, alpha=ALPHA):
    """R.solve_snapshots on the callable `model`."""
    s0, u = state0.to(dtype), u0.to(dtype).clone()
    m = torch.zeros_like(u)
    trace, out = [], {}
    for it in range(max(snaps) + 1):
        if it in snaps:
            J = cost(model, s0, u, dt)
            out[it] = dict(u=u.clone(), cost=J, trace=torch.stack(trace + [J]))
        if it == max(snaps):
            break
        J, g = cost_and_grad(model, s0, u, dt)
        trace.append(J)
        m = beta * m + alpha * g
        u = (u - m).clamp(-1.0, 1.0)
    return out


def solve(model, dtype, state0, u0, dt, iters):
    return solve_snapshots(model, dtype, state0, u0, dt, (iters,))[iters]


# ---- the closed loop -------------------------------------------------------------
def closed_loop(dtype, state0, dt, iters, max_steps, model, plant, thresh_div=0.21,
                horizon=H):
    """R.closed_loop's balance mode with the solver on `model` and the
    environment on `plant` -> dict(states [B,T,4], actions [B,T], cost [B,T],
    steps [B], upright [B], margin)."""
    B, T = state0.shape[0], max_steps
    s = state0.to(dtype)
    u = torch.zeros(B, horizon, 1, dtype=dtype)
    alive = torch.ones(B, dtype=torch.bool)
    out = dict(states=torch.zeros(B, T, 4, dtype=dtype), actions=torch.zeros(B, T, dtype=dtype),
               cost=torch.zeros(B, T, dtype=dtype), steps=torch.zeros(B, dtype=torch.long),
               upright=torch.ones(B, dtype=torch.bool), margin=float("inf"))
    for i in range(T):
        if i > 0:
            u = R.shift(u)
        res = solve(model, dtype, s, u, dt, iters)
        u = res["u"]
        action = u[:, 0]
        with torch.no_grad():
            new = plant(s, action, dt).to(dtype)
        new = torch.stack([new[:, 0], new[:, 1], R.env_wrap(new[:, 2]), new[:, 3]], 1)
        rec = alive.clone()
        out["states"][rec, i] = new[rec]
        out["actions"][rec, i] = action[rec, 0]
        out["cost"][rec, i] = res["cost"][rec]
        out["steps"][rec] = i + 1
        inside = (new[:, 2] > -thresh_div) & (new[:, 2] < thresh_div)
        out["margin"] = min(out["margin"], float((new[rec, 2].abs() - thresh_div).abs().min()))
        out["upright"] &= ~(rec & ~inside)
        alive = alive & inside
        if not alive.any():
            break
        s = new
    return out


# ---- cached cases ----------------------------------------------------------------
def loop_starts():
    """The starts of the existing learnt-plant test."""
    return R.balance_starts(64, seed=41)


LOOP_STEPS = 40


@functools.lru_cache(maxsize=None)
def loop_case(dtype):
    """Plant and model both the fitted module: 64 flights, 40 steps, thresh_div
    0.21, 10 iterations."""
    m = module()
    return closed_loop(dtype, loop_starts(), DT, 10, LOOP_STEPS, LearntModel(m, dtype),
                       R.LearntPlant(m, dtype))


@functools.lru_cache(maxsize=None)
def solve_case(dtype, B=256, horizon=H, seed=11):
    """R.thirds(B) from u = 0 on the fitted module: ONE restated run of 20
    iterations serving the three iteration counts."""
    s0, parts = R.thirds(B, seed=seed)
    return s0, parts, solve_snapshots(LearntModel(module(), dtype), dtype, s0,
                                      torch.zeros(B, horizon, 1), DT, (1, 10, 20))


# ---- the host twins (libapg_cpu.so) ----------------------------------------------
def twins():
    from apg_trajectory_tracking_amd import _capi
    lib = R.twins()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    PP = ctypes.POINTER(_capi.ApgCartpoleParams)
    PL = ctypes.POINTER(_capi.ApgCartpoleLearnt)
    PO = ctypes.POINTER(_capi.ApgCartpoleMpcOptions)
    lib.apg_cartpole_learnt_mpc_solve_cpu.argtypes = [P, P, F, PL, PO, I, I, P, P, P]
    lib.apg_cartpole_learnt_mpc_closed_loop_cpu.argtypes = [
        ctypes.POINTER(_capi.ApgCartpoleFlight), F, PP, PL, PL, PO, I, I, P]
    return lib


class HostModel:
    """ApgCartpoleLearnt over HOST copies of a module's tensors (kept alive here)."""

    def __init__(self, mod):
        from apg_trajectory_tracking_amd import _capi
        self.arrays = [np.ascontiguousarray(mod.cfg[k].detach().cpu().numpy(), np.float32)
                       for k in PHYS]
        self.arrays += [np.ascontiguousarray(t.detach().cpu().numpy(), np.float32) for t in (
            mod.linear_state_1.weight, mod.linear_state_1.bias, mod.linear_state_2.weight)]
        self.struct = _capi.ApgCartpoleLearnt(*[a.ctypes.data for a in self.arrays])


def twin_solve(tw, mod, state0, u0, dt, iters, horizon=H, opt=None):
    """apg_cartpole_learnt_mpc_solve_cpu -> dict(u, cost, trace) as `solve`."""
    B = state0.shape[0]
    s = state0.float().t().contiguous()
    start = None if u0 is None else u0.float()[:, :, 0].t().contiguous()
    u, cost_out, trace = torch.zeros(horizon, B), torch.zeros(B), torch.zeros(iters + 1, B)
    hm = HostModel(mod)
    rc = tw.apg_cartpole_learnt_mpc_solve_cpu(
        s.data_ptr(), None if start is None else start.data_ptr(), dt, ctypes.byref(hm.struct),
        ctypes.byref(opt or R.options(iters)), B, horizon, u.data_ptr(), cost_out.data_ptr(),
        trace.data_ptr())
    assert rc == 0, tw.apg_cpu_last_error_string()
    return dict(u=u.t().contiguous()[:, :, None], cost=cost_out, trace=trace)


def twin_closed_loop(tw, state0, dt, iters, max_steps, model, plant=None, plant_params=None,
                     model_params=None, thresh_div=0.21, mode="balance", burn_in=0,
                     horizon=H):
    """The closed-loop twins -> the restatement's layout.  model: a module
    (apg_cartpole_learnt_mpc_closed_loop_cpu) or None: the analytic solver on
    `model_params` (apg_cartpole_mpc_closed_loop_cpu).  plant: a module, or None:
    the analytic plant on `plant_params`."""
    B, T = state0.shape[0], max_steps
    s = state0.float().t().contiguous()
    steps, upright = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    vs, vq = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    states, actions, cost_ = torch.zeros(T, 4, B), torch.zeros(T, B), torch.zeros(T, B)
    hp = None if plant is None else HostModel(plant)
    hm = None if model is None else HostModel(model)
    fn = (tw.apg_cartpole_mpc_closed_loop_cpu if model is None
          else tw.apg_cartpole_learnt_mpc_closed_loop_cpu)
    from apg_trajectory_tracking_amd import _capi
    flight = _capi.ApgCartpoleFlight(
        state0=s.data_ptr(), max_steps=T, mode={"balance": 0, "swingup": 1}[mode],
        thresh_div=thresh_div, burn_in=burn_in, steps=steps.data_ptr(),
        upright=upright.data_ptr(), vel_sum=vs.data_ptr(), vel_sq=vq.data_ptr(),
        states=states.data_ptr(), actions=actions.data_ptr())
    rc = fn(ctypes.byref(flight), dt, None if hp else ctypes.byref(R.params(plant_params)),
            ctypes.byref(hp.struct) if hp else None,
            ctypes.byref(hm.struct) if hm else ctypes.byref(R.params(model_params)),
            ctypes.byref(R.options(iters)), B, horizon, cost_.data_ptr())
    assert rc == 0, tw.apg_cpu_last_error_string()
    return R.from_device_layout(dict(steps=steps, upright=upright, vel_sum=vs, vel_sq=vq,
                                     states=states, actions=actions, cost=cost_))


# ---- shared acceptance -----------------------------------------------------------
def same_flights(got, want, what):
    """The acceptance of the existing learnt-plant test: `steps` equal on >= 97 %
    of the flights, states within 2e-3 on all but 3 % of those."""
    B = want["steps"].shape[0]
    same = got["steps"] == want["steps"]
    print("%s: steps equal on %d of %d flights" % (what, int(same.sum()), B))
    assert int(same.sum()) >= 0.97 * B
    d = (got["states"].double() - want["states"].double()).abs().amax((1, 2))
    bad = int((d[same] > 2e-3).sum())
    print("%s: beyond 2e-3: %d, largest difference %.3e" % (what, bad, float(d[same].max())))
    assert bad <= 0.03 * int(same.sum())


def pays(learnt, nominal, what):
    """Planning with the adapted model pays (`learnt`, `nominal`: the two arms'
    flights on the 64 loop starts, the first 16 of which leave whatever the
    controller does): every one of the 48 near-upright starts runs all 40 steps
    with the learnt model; the nominal arm's mean steps over those 48 is below
    35 (float64 and float32 restatements: 28.35); mean |theta| over the flights
    finished in both arms is below 0.6 x the nominal arm's (0.40)."""
    T = LOOP_STEPS
    near = slice(16, 64)
    ls, ns = learnt["steps"][near], nominal["steps"][near]
    both = (learnt["steps"] == T) & (nominal["steps"] == T)
    th_l = float(learnt["states"][both][:, :, 2].abs().mean())
    th_n = float(nominal["states"][both][:, :, 2].abs().mean())
    print("%s: learnt model finishes %d of 64 (mean steps near upright %.2f), nominal %d "
          "(%.2f); mean |theta| on the %d finished in both: %.4f against %.4f, ratio %.3f"
          % (what, int((learnt["steps"] == T).sum()), float(ls.float().mean()),
             int((nominal["steps"] == T).sum()), float(ns.float().mean()), int(both.sum()),
             th_l, th_n, th_l / th_n))
    assert bool((ls == T).all())
    assert float(ns.float().mean()) < 35
    assert int(both.sum()) > 0 and th_l < 0.6 * th_n


to_numpy = R.to_numpy
