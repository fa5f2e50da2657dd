"""Drop-in for neural_control.dynamics.cartpole_dynamics.CartpoleDynamics
(reference: neural_control/dynamics/cartpole_dynamics.py:21-119): same
constructor and `dyn(state, action, dt)` surface; HIP step kernel
(apg_cartpole_step_fwd / _bwd).  LearntCartpoleDynamics (:122-140): the
trainable simulator of the adapt flow (apg_cartpole_learnt_*)."""
import torch

from .. import functional as F

# neural_control/dynamics/config_cartpole.json:1-11
DEFAULT_CONFIG = {
    "masscart": 1.0, "masspole": 0.1, "length": 0.5, "max_force_mag": 30.0,
    "muc": 0.0005, "mup": 0.000002, "wind": 0.0, "vel_drag": 0.0,
    "contact": 0.0, "delay": 0.0,
}
gravity = 9.81


def _config(modified_params):
    """The config after `update(modified_params)` with the derived keys
    (cartpole_dynamics.py:30-36)."""
    cfg = dict(DEFAULT_CONFIG)
    cfg.update(modified_params)
    cfg["friction"] = .5      # cartpole_dynamics.py:34 (sic)
    cfg["total_mass"] = cfg["masspole"] + cfg["masscart"]
    cfg["polemass_length"] = cfg["masspole"] * cfg["length"]
    return cfg


class CartpoleDynamics:

    def __init__(self, modified_params={}, test_time=0, batch_size=1):
        self.batch_size = batch_size
        self.test_time = test_time
        self.cfg = _config(modified_params)
        self.timestamp = 0
        self.params = F.cartpole_params(self.cfg)

    def __call__(self, state, action, dt):
        return self.simulate_cartpole(state, action, dt)

    def simulate_cartpole(self, state, action, delta_t):
        """state [B,4] = [x, x_dot, theta, theta_dot], action [B,1] ->
        next state [B,4]."""
        self.timestamp += .05          # side effect kept (:57)
        return F.cartpole_step(state, action, delta_t, self.params)

    def rollout(self, state0, action_seq, dt):
        """H-step no-grad unroll in one kernel: states [B, H, 4]."""
        self.timestamp += .05 * action_seq.shape[1]
        return F.cartpole_rollout_fwd(F._f32c(state0), F._f32c(action_seq), dt,
                                      self.params)


class LearntCartpoleDynamics(torch.nn.Module, CartpoleDynamics):
    """LearntCartpoleDynamics (cartpole_dynamics.py:122-140 with
    learnt_dynamics.py:58-98): the physics on trainable parameters plus a
    5 -> 64 -> 4 relu residual on [state, action],
        forward(s, a, dt) = simulate_cartpole(s, a, dt) + state_transformer(s, a).
    Same constructor, parameter names, state_dict keys and init draws as the
    reference (its state_dicts load strictly): linear_state_1 (bias) and
    linear_state_2 (no bias) with their normal_(std=1e-4) re-draws, then `cfg`,
    a ParameterDict of [1] tensors in the config's order; not_trainable "all"
    or a list of keys freezes them.  Only max_force_mag, masspole, length,
    friction, total_mass and polemass_length enter the physics, each on its
    own (total_mass is not re-derived); the other keys get no gradient.
    forward is one launch, its backward one reverse launch pair that returns
    every parameter's gradient.  Nothing reads the analytic `params` of
    CartpoleDynamics: the module has none."""

    def __init__(self, modified_params={}, not_trainable=[]):
        torch.nn.Module.__init__(self)
        # CartpoleDynamics.__init__ without the analytic parameter struct
        self.batch_size = 1
        self.test_time = 0
        self.timestamp = 0
        cfg = _config(modified_params)
        # learnt_dynamics.LearntDynamics(4, 1): the draws in the reference's order
        std = 0.0001
        self.linear_state_1 = torch.nn.Linear(5, 64)
        torch.nn.init.normal_(self.linear_state_1.weight, mean=0.0, std=std)
        torch.nn.init.normal_(self.linear_state_1.bias, mean=0.0, std=std)
        self.linear_state_2 = torch.nn.Linear(64, 4, bias=False)
        torch.nn.init.normal_(self.linear_state_2.weight, mean=0.0, std=std)
        self.transform_action = False
        self.cfg = torch.nn.ParameterDict({
            key: torch.nn.Parameter(
                torch.tensor([val]),
                requires_grad=not (not_trainable == "all" or key in not_trainable))
            for key, val in cfg.items()})

    @property
    def params(self):
        raise AttributeError(
            "LearntCartpoleDynamics has no analytic parameter struct: its "
            "parameters are the tensors of `cfg` (functional.cartpole_learnt_*)")

    def forward(self, state, action, dt):
        """state [B, 4], action [B, 1] -> next state [B, 4]."""
        self.timestamp += .05          # (simulate_cartpole's side effect)
        return F.cartpole_learnt_step(self, state, action, dt)

    def simulate(self, state, action, dt):
        return self.simulate_cartpole(state, action, dt)

    def simulate_cartpole(self, state, action, delta_t):
        """The physics alone on the live parameters (no residual)."""
        self.timestamp += .05
        return F.cartpole_learnt_step(self, state, action, delta_t, residual=False)

    def state_transformer(self, state, action):
        """The residual network alone (learnt_dynamics.py:84-88), as torch
        ops: a helper of the reference's interface; forward does not call it."""
        state_action = torch.cat((state, action), dim=1)
        return self.linear_state_2(torch.relu(self.linear_state_1(state_action)))

    def rollout(self, state0, action_seq, dt):
        """H-step no-grad unroll through the LEARNT simulator: states [B, H, 4]."""
        with torch.no_grad():
            s, out = state0, []
            for k in range(action_seq.shape[1]):
                s = self(s, action_seq[:, k], dt)
                out.append(s)
        return torch.stack(out, 1)
