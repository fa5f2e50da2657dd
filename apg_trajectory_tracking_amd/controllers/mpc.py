"""Drop-in for `neural_control.controllers.mpc.MPC` on the quadrotor, the
cart-pole and the fixed wing: the comparator the reference judges its learnt controllers against,
batched.

    mpc = MPC(horizon=10, dt=0.1, dynamics="flightmare")
    action = mpc.predict_actions(current_state, ref_states)    # [1, 4]

Kept from the reference (neural_control/controllers/mpc.py): the stage cost
(_initParamsSimpleQuad: Q_pen = diag(100,100,100, 0,0,0, 10,10,10, 1,1,1), Q_u
= diag(50,1,1,1) around u = 0.5 - quad_mpc_loss is that cost divided by ten),
the action box [0, 1], the Flightmare model with `modified_params`, the warm
start by shifting the previous solution, and this call surface.

Two deliberate differences:
  * ALL H stages carry state cost (the reference's NLP drops the last
    stage's): the MPC optimum and a policy's training loss are then the same
    quantity on the same window (functional.quad_policy_optimality_gap);
  * the solver is first-order single shooting - projected heavy-ball descent
    with a fixed number of iterations, one trajectory per GPU lane
    (apg_quad_mpc_solve) - instead of IPOPT on a multiple-shooting NLP: every
    trajectory of a batch does the same work and the result is a deterministic
    function of the inputs.

`MPC(learnt_model=module)` plans through a LearntDynamics module instead - the
role of the reference's LearntDynamicsMPC (neural_control/dynamics/
learnt_dynamics.py:5-55): MPC with the ADAPTED model; `params` are then the
module's, `modified_params` cannot be given together with it.

`QuadEvaluator(MPC(...), environment)` flies whole batches of reference
trajectories with the solver inside the closed-loop kernel
(functional.quad_mpc_closed_loop): plant = the evaluator's environment, model =
this object's parameters.

The cart-pole (scripts/evaluate_cartpole.py:399-407):

    mpc = MPC(horizon=10, dt=0.05, dynamics="cartpole")
    action = mpc.predict_actions(current_state)                # [1, 1]

Kept from the reference (_initParamsCartpole, mpc.py:87-100): the action box
[-1, 1], the start u = 0, the warm start by shifting, `modified_params`, and
the model of its CasADi twin (CartpoleDynamicsMPC.simulate_cartpole,
neural_control/dynamics/cartpole_dynamics.py:239-278): the angle is advanced as
theta + dt theta_dot, without the atan2 wrap of the torch step, inside the
horizon.  The cost is the TRAINING loss on the training reference
(cartpole_loss_mpc against make_reference), so that the MPC optimum and a
policy's loss are the same quantity (functional.cartpole_policy_optimality_gap).
Two deliberate differences from the reference's NLP follow from that:
  * the reference's NLP has no action cost (here 0.01 sum u^2);
  * the reference's NLP uses a `linspace` reference over H + 2 points and drops
    the last stage's state cost (here: the state fading to zero over H rows,
    every row with its cost).
The solver is the same first-order single shooting (apg_cartpole_mpc_solve).
`MPC(dynamics="cartpole", learnt_model=m)` plans through a
LearntCartpoleDynamics module (apg_cartpole_learnt_mpc_solve: the same unwrapped
step on the module's six live parameters plus its residual); `params` is then
None - the module has no parameter struct.
`evaluate_cartpole.Evaluator(MPC(...), env)` flies whole batches of episodes
with the solver inside the closed-loop kernel
(functional.cartpole_mpc_closed_loop).

The fixed wing (scripts/evaluate_fixed_wing.py:232-243):

    mpc = MPC(horizon=10, dt=0.05, dynamics="fixed_wing_3D")
    action = mpc.predict_actions(current_state, target)        # [1, 4]

Kept from the reference (_initParamsFixedWing_3D, mpc.py:135-150): the action
box [0, 1], an action cost on the three control surfaces only, around 0.5 (its
_Q_u = diag(0, 10, 10, 10): the thrust is free), the FixedWingDynamics model
with `modified_params`, the warm start by shifting, and the call surface
(state, target point).  What differs:
  * the cost is the TRAINING loss on the training reference (fixed_wing_mpc_loss
    against WingDataset._compute_target_pos: rows p0 + n (12 dt) (k + 1) towards
    the target, every row with its cost), so that the MPC optimum and a policy's
    loss are the same quantity (functional.wing_policy_optimality_gap); the
    reference's NLP (preprocess_fixed_wing, mpc.py:383-414) spaces its points
    by the current speed, |v| dt per step, weights the position with 1000 and
    the surfaces with 10 (here 10 and 0.1, the training loss's) and drops the
    last stage's state cost;
  * one horizon, 10, with the model's dt equal to the plant's (the reference's
    evaluation uses horizon 20 at dt 0.1 on a plant stepped at 0.05);
  * the solver is the same first-order single shooting (apg_wing_mpc_solve),
    from u = (0.25, 0.5, 0.5, 0.5);
  * no `learnt_model`: planning through a LearntFixedWingDynamics module is not
    built.
`evaluate_fixed_wing.FixedWingEvaluator(MPC(...), FixedWingDynamics())` flies
whole batches of target lists with the solver inside the closed-loop kernel
(functional.wing_mpc_closed_loop): plant = the evaluator's environment, model =
this object's parameters.  Other fixed-wing names of the reference
("fixed_wing", "fixed_wing_2D") are not implemented."""
import numpy as np
import torch

from .. import functional as F
from ..dynamics.cartpole_dynamics import CartpoleDynamics, LearntCartpoleDynamics
from ..dynamics.fixed_wing_dynamics import FixedWingDynamics
from ..dynamics.quad_dynamics_flightmare import FlightmareDynamics

DYNAMICS = ("flightmare", "cartpole", "fixed_wing_3D")


class MPC:

    def __init__(self, horizon=10, dt=0.1, dynamics="flightmare", modified_params={},
                 iters=10, beta=None, alpha_thrust=None, alpha_rate=None, alpha=None,
                 alpha_surface=None, device=None, learnt_model=None, **kwargs):
        if dynamics not in DYNAMICS:
            raise NotImplementedError(
                f"MPC dynamics {dynamics!r}: implemented here: {', '.join(DYNAMICS)} "
                "(the quadrotor, the cart-pole and the 3D fixed wing)")
        if horizon not in (5, 10):
            raise ValueError("the batched MPC is built for horizon 5 or 10")
        if dynamics == "fixed_wing_3D":
            if horizon != 10:
                raise ValueError("the batched fixed-wing MPC is built for horizon 10")
            if learnt_model is not None:
                raise NotImplementedError(
                    "learnt_model: planning through a LearntFixedWingDynamics module is "
                    "not built (dynamics='flightmare' and 'cartpole' take one)")
        if learnt_model is not None:
            cart_module = isinstance(learnt_model, LearntCartpoleDynamics)
            if cart_module != (dynamics == "cartpole"):
                raise NotImplementedError(
                    "learnt_model: the solver plans through a LearntDynamics module "
                    "for dynamics='flightmare' and through a LearntCartpoleDynamics "
                    f"module for dynamics='cartpole' (got {type(learnt_model).__name__} "
                    f"with dynamics={dynamics!r})")
            if modified_params:
                raise ValueError(
                    "learnt_model brings its own parameters (the module's): "
                    "modified_params cannot be given together with it")
        self.horizon = horizon
        self.dt = dt
        self.dynamics_model = dynamics
        # a LearntDynamics / LearntCartpoleDynamics module: the solver's model is
        # that module
        self.learnt_model = learnt_model
        if dynamics == "cartpole":
            self.model = CartpoleDynamics(modified_params)
            self.options = dict(iters=iters, beta=beta, alpha=alpha)
        elif dynamics == "fixed_wing_3D":
            self.model = FixedWingDynamics(modified_params)
            self.options = dict(iters=iters, beta=beta, alpha_thrust=alpha_thrust,
                                alpha_surface=alpha_surface)
        else:
            self.model = FlightmareDynamics(modified_params=modified_params)
            self.options = dict(iters=iters, beta=beta, alpha_thrust=alpha_thrust,
                                alpha_rate=alpha_rate)
        if learnt_model is None:
            self.params = self.model.params
        else:
            # (a LearntCartpoleDynamics has no parameter struct: its parameters
            # are the module's tensors)
            self.params = None if dynamics == "cartpole" else learnt_model.params
        self.device = device
        # [B,H,4] ([B,H,1] cart-pole): the previous solution, not yet shifted
        self.warm_start = None
        self.last_cost = None

    def reset(self):
        """Forget the warm start: the next call starts from u = 0.5 (the
        cart-pole: u = 0; the fixed wing: (0.25, 0.5, 0.5, 0.5))."""
        self.warm_start = None
        self.last_cost = None

    def _shifted_warm_start(self, B):
        if self.warm_start is None or self.warm_start.shape[0] != B:
            return None
        w = self.warm_start
        return torch.cat((w[:, 1:], w[:, -1:]), 1)

    def predict_actions(self, current_state, ref_states=None):
        """The first action of this call's solve.  numpy in - a state [S] and,
        for the quadrotor, ref_states [H,9] (rows as `preprocess_quad` lays them
        out: columns 0:3 position, 6:9 velocity), for the fixed wing the target
        [3], for the cart-pole nothing - gives np.ndarray [1,A] like the
        reference (what its Evaluator wraps in torch.tensor([...])); tensors
        with a leading batch dimension give a tensor [B,A].  The warm start
        lives in the object and is shifted per call."""
        numpy_in = not torch.is_tensor(current_state)
        dev = torch.device(self.device or
                           ("cuda" if numpy_in else current_state.device))

        def on_device(x):
            return torch.as_tensor(np.asarray(x, dtype=np.float32) if numpy_in
                                   else x).to(dev, torch.float32)
        s = on_device(current_state)
        r = None if self.dynamics_model == "cartpole" else on_device(ref_states)
        if s.dim() == 1:
            s, r = s[None], None if r is None else r[None]
        solve = {"cartpole": self._solve_cartpole, "fixed_wing_3D": self._solve_wing,
                 "flightmare": self._solve_quad}[self.dynamics_model]
        res = solve(s, r)
        self.warm_start, self.last_cost = res["u"], res["cost"]
        action = res["u"][:, 0]
        return action.cpu().numpy() if numpy_in else action

    def _planner(self):
        return {} if self.learnt_model is None else dict(learnt=self.learnt_model)

    def _solve_cartpole(self, s, _):
        if s.dim() != 2 or s.shape[1] != 4:
            raise ValueError(f"state [4] or [B,4] expected, got {tuple(s.shape)}")
        return F.cartpole_mpc_solve(s, self.dt, self.params,
                                    u0=self._shifted_warm_start(s.shape[0]),
                                    horizon=self.horizon, **self.options, **self._planner())

    def _solve_wing(self, s, t):
        """The reference rows are built here (functional.wing_mpc_reference)."""
        if s.dim() != 2 or s.shape[1] != 12 or t.shape != (s.shape[0], 3):
            raise ValueError("state [B,12] and target [B,3] expected")
        ref = F.wing_mpc_reference(s, t, self.dt, self.horizon)
        return F.wing_mpc_solve(s, ref, self.dt, self.params,
                                u0=self._shifted_warm_start(s.shape[0]), **self.options)

    def _solve_quad(self, s, r):
        if r.shape[1:] != (self.horizon, 9) or s.shape != (r.shape[0], 12):
            raise ValueError(f"state [B,12] and reference rows [B,{self.horizon},9] expected")
        return F.quad_mpc_solve(s, r, self.dt, self.params,
                                u0=self._shifted_warm_start(s.shape[0]), **self.options,
                                **self._planner())
