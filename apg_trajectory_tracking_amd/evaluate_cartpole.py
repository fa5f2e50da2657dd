"""Batched closed-loop evaluation of a cart-pole controller - the role of
scripts/evaluate_cartpole.py:37-318 (`Evaluator.evaluate_in_environment`,
`evaluate_swingup`) with every test flight flown in parallel by one kernel
launch (apg_cartpole_mlp_closed_loop) instead of a Python loop of batch-1
policy / dynamics calls per time step.

Same names, arguments and statistics as the reference:
  * `CartpoleWrapper` (neural_control/controllers/network_wrapper.py:101-149)
    and `CartPoleEnv` (neural_control/environments/cartpole_env.py:32-115)
    with its resets, which draw from numpy's global stream in the reference's
    order - so `np.random.seed` makes both evaluators fly the same flights and
    leaves the stream where the reference leaves it;
  * `Evaluator.evaluate_in_environment` / `evaluate_swingup` return the same
    dict (or, with return_success, the same per-flight values).
There is no renderer, no image / sequence controller and no dynamics
comparison (`eval_dyn`) here.

With a `controllers.MPC(dynamics="cartpole")` controller - the comparator of
scripts/evaluate_cartpole.py:399-407 - the same Evaluator flies the batch with
the solver inside the kernel (apg_cartpole_mpc_closed_loop): the plant is the
environment's dynamics, the model the MPC object's parameters - or, with
`MPC(dynamics="cartpole", learnt_model=m)`, the module `m`
(apg_cartpole_learnt_mpc_closed_loop)."""
import numpy as np
import torch

from . import functional as F


def _is_learnt(dynamics):
    """A LearntCartpoleDynamics environment (the adapt flow flies the trained
    simulator, scripts/train_cartpole.py:50-55)?"""
    from .dynamics.cartpole_dynamics import LearntCartpoleDynamics
    return isinstance(dynamics, LearntCartpoleDynamics)


class CartpoleWrapper:
    """network_wrapper.py:101-149: the raw state (no normalisation) in, the
    action plan [1, horizon, action_dim] out."""

    def __init__(self, model, horizon=10, action_dim=1, **kwargs):
        self.horizon = horizon
        self.action_dim = action_dim
        self.net = model

    def raw_states_to_torch(self, states):
        if len(states.shape) == 1:
            states = np.expand_dims(states, 0)
        return torch.from_numpy(np.asarray(states)).float()

    def predict_actions(self, state, ref_state=None):
        dev = next(self.net.parameters()).device
        with torch.no_grad():
            action_seq = self.net(self.raw_states_to_torch(state).to(dev))
        if action_seq.size()[-1] > self.action_dim:
            action_seq = torch.reshape(action_seq, (-1, self.horizon, self.action_dim))
        return action_seq


class CartPoleEnv:
    """cartpole_env.py:32-115 without the renderer: `state` is a numpy array,
    `_step` goes through the step kernel (apg_cartpole_step_fwd), or through
    the module's forward when `dynamics` is a LearntCartpoleDynamics."""

    def __init__(self, dynamics, dt, thresh_div=.21):
        self.dynamics = dynamics
        self.dt = dt
        self.thresh_div = thresh_div
        self.x_threshold = 2.4
        self.state_limits = np.array([2.4, 7.5, np.pi, 7.5])
        self.state = self._reset()
        self.steps_beyond_done = None

    def is_upright(self):
        theta = self.state[2]
        return theta > -self.thresh_div and theta < self.thresh_div

    def _step(self, action, image=None, state_action_buffer=None, is_torch=True,
              device="cuda"):
        state = torch.tensor([list(self.state)], dtype=torch.float32, device=device)
        action = torch.as_tensor(action if is_torch else [action],
                                 dtype=torch.float32).reshape(1, 1).to(device)
        if _is_learnt(self.dynamics):     # the module's forward, no grad
            with torch.no_grad():
                nxt = self.dynamics(state, action, self.dt)
        else:
            nxt = F.cartpole_step(state, action, self.dt, self.dynamics.params)
        self.state = nxt[0].cpu().numpy()
        # stay in bounds with theta (the reference's numpy scalar arithmetic)
        theta = self.state[2]
        if theta > np.pi:
            self.state[2] = theta - 2 * np.pi
        if theta <= -np.pi:
            self.state[2] = 2 * np.pi + theta
        return self.state

    def _reset(self):
        self.state = (np.random.rand(4) * 2 - 1) * self.state_limits
        self.steps_beyond_done = None
        return np.array(self.state)

    def _reset_swingup(self):
        self.state = (np.random.rand(4) * 2 - 1) * self.state_limits
        self.state[0] = 0
        self.state[1] *= 0.1
        rand_sign = (-1) if np.random.rand() > .5 else 1
        self.state[2] = rand_sign * (2.8 + np.random.rand() * .3)
        self.state[3] *= 0.1
        return self.state

    def _reset_upright(self):
        self.state = (np.random.rand(4) - .5) * .3
        self.state[2] = ((np.random.rand(1) - .5) * .1)[0]
        return self.state


class Evaluator:

    def __init__(self, controller, eval_env, eval_dyn=None, **kwargs):
        if eval_dyn is not None:
            raise NotImplementedError(
                "sequence dynamics (eval_dyn) are outside the batched evaluator")
        self.controller = controller
        self.eval_env = eval_env
        self.eval_dyn = eval_dyn
        self.initialize_straight = 1
        self.last_flights = None    # the kernel's output of the last call

    # ------------------------------------------------------------ the draws
    def balance_starts(self, nr_iters):
        """The start states of evaluate_in_environment's flights, drawn as the
        reference's loop draws them: per flight _reset_upright, then (after
        the flight) _reset."""
        env, starts = self.eval_env, []
        for _ in range(nr_iters):
            env._reset_upright()
            if self.initialize_straight:
                env.state[0] = env.state[1] = env.state[2] = env.state[3] = 0
            starts.append(np.array(env.state, dtype=np.float32))
            env._reset()
        return np.stack(starts)

    def swingup_starts(self, nr_iters):
        """evaluate_swingup's start states: _reset_swingup per flight."""
        env = self.eval_env
        return np.stack([np.array(env._reset_swingup(), dtype=np.float32)
                         for _ in range(nr_iters)])

    # ------------------------------------------------------------ one launch
    def _fly_mpc(self, starts, max_steps, mode, burn_in):
        mpc, env = self.controller, self.eval_env
        if mpc.dynamics_model != "cartpole":
            raise ValueError("the cart-pole evaluator needs MPC(dynamics='cartpole')")
        if float(mpc.dt) != float(env.dt):
            raise ValueError(f"MPC dt {mpc.dt} and environment dt {env.dt} differ: "
                             "the closed loop has one step length")
        learnt = _is_learnt(env.dynamics)
        dev = torch.device(mpc.device or (
            next(env.dynamics.parameters()).device if learnt else "cuda"))
        # MPC(learnt_model=m): the solver plans through the module
        planner = {} if mpc.learnt_model is None else dict(model_learnt=mpc.learnt_model)
        out = F.cartpole_mpc_closed_loop(
            torch.from_numpy(starts).to(dev), env.dt,
            None if learnt else env.dynamics.params, model_params=mpc.params,
            learnt=env.dynamics if learnt else None, max_steps=max_steps, mode=mode,
            thresh_div=env.thresh_div, burn_in=burn_in, want_trajectory=True,
            horizon=mpc.horizon, **mpc.options, **planner)
        self.last_flights = out
        return out

    def _fly(self, starts, max_steps, mode, burn_in):
        from .controllers.mpc import MPC
        if isinstance(self.controller, MPC):
            return self._fly_mpc(starts, max_steps, mode, burn_in)
        net = self.controller.net
        dev = next(net.parameters()).device
        dyn = self.eval_env.dynamics
        learnt = _is_learnt(dyn)
        out = F.cartpole_mlp_closed_loop(
            net, torch.from_numpy(starts).to(dev), self.eval_env.dt,
            None if learnt else dyn.params, max_steps=max_steps, mode=mode,
            thresh_div=self.eval_env.thresh_div, burn_in=burn_in,
            want_trajectory=True, learnt=dyn if learnt else None)
        self.last_flights = out
        return out

    def evaluate_in_environment(self, nr_iters=1, max_steps=250, render=False,
                                burn_in_steps=50, return_success=0):
        """scripts/evaluate_cartpole.py:79-264: how long the pole stays inside
        (-thresh_div, thresh_div), all flights in one launch."""
        self.dyn_eval_test = []
        if nr_iters == 0:
            return 0, 0, []
        if render:
            raise ValueError("there is no renderer on the GPU path")
        out = self._fly(self.balance_starts(nr_iters), max_steps, "balance",
                        burn_in_steps)
        steps = out["steps"].cpu().numpy().astype(np.int64)
        n = float(steps.sum())
        mean_vel = float(out["vel_sum"].sum()) / n
        var = float(out["vel_sq"].sum()) / n - mean_vel**2
        success = (steps - 1).astype(np.float64)
        res = {"mean_vel": mean_vel, "std_vel": float(np.sqrt(max(var, 0.0))),
               "mean_stable": float(np.mean(success)),
               "std_stable": float(np.std(success))}
        print("Average velocity: %3.2f (%3.2f)" % (res["mean_vel"], res["std_vel"]))
        print("Average success: %3.2f (%3.2f)" % (res["mean_stable"], res["std_stable"]))
        if return_success:
            vel = out["states"][:, 1].abs().t().cpu().numpy()
            velocities = [float(v) for i, k in enumerate(steps) for v in vel[i, :k]]
            return success, velocities
        return res

    def evaluate_swingup(self, nr_iters=1, max_steps=250, render=False,
                         burn_in_steps=100, return_success=0):
        """scripts/evaluate_cartpole.py:266-318: swing up from a hanging start;
        a flight stays `upright` unless theta > 1 after burn_in_steps."""
        if render:
            raise ValueError("there is no renderer on the GPU path")
        if nr_iters == 0:   # (the reference: means of empty lists)
            return np.zeros(0) if return_success else {
                "mean_vel": float("nan"), "std_vel": float("nan")}
        out = self._fly(self.swingup_starts(nr_iters), max_steps, "swingup",
                        burn_in_steps)
        # the environment is left in the last flight's state
        self.eval_env.state = out["states"][-1, :, -1].cpu().numpy()
        success = out["upright"].cpu().numpy().astype(np.float64)
        if return_success:
            return success
        n = nr_iters * max(max_steps - burn_in_steps - 1, 0)
        mean_vel = float(out["vel_sum"].sum()) / n if n else float("nan")
        # (quirk kept: std_vel is the mean as well)
        return {"mean_vel": mean_vel, "std_vel": mean_vel}
