"""Drop-in for scripts/train_cartpole.py:30-165 (`TrainCartpole`) restricted
to the APG hot path: `run_epoch` (:118-165) with `make_reference` (:103-110).
The controller branch is one fused HIP launch (make_reference + H x cartpole
dynamics + cartpole_loss_mpc + adjoint); with the stock policy (`fused_policy`)
the policy's forward, its reverse pass, the weight gradients and momentum SGD
run inside the same call (apg_cartpole_mlp_train_step).  Quirks kept: the
policy ends in tanh with NO sigmoid (:127-130), `simple_model.Net` zeroes column 0 of its
input in place, run_epoch divides by the last batch index (:163).

With a LearntCartpoleDynamics as train dynamics (`train_norm_dynamics`, the
reference's adapt mode :245-262) run_epoch also fits the simulator
(train="dynamics") and the controller branch runs through it, fused into one
launch (apg_cartpole_learnt_rollout_fwd_bwd); the fit step itself is one fused
call as well (`fused_fit`, apg_cartpole_learnt_fit_fwd_bwd).  With
`fused_learnt_policy` (off by default) the controller step through the learnt
simulator is one fused call too, policy and momentum SGD inside
(apg_cartpole_learnt_mlp_train_step).  Two deliberate deviations make
that loop run at all: run_epoch accepts the `epoch` that TrainBase.run_dynamics
passes (the reference's raises TypeError), and init_optimizer builds the
simulator's optimizer for any nn.Module simulator (the reference's only for
the quad / wing learnt classes: AttributeError).

The evaluation side (:167-205, :220-238): `evaluate_model` flies the trainer's
10 test episodes through evaluate_cartpole.Evaluator - one kernel launch -
and runs the divergence-threshold ladder and the resampling of the data set
(SyntheticCartpoleDataset.resample_data); `train_control` is the training
loop around it."""
import torch

from . import _capi
from . import functional as F
from .dataset import SyntheticCartpoleDataset, TensorBatches
from .drone_loss import cartpole_loss_mpc
from .evaluate_cartpole import CartPoleEnv, CartpoleWrapper, Evaluator
from .models.simple_model import Net
from .train_base import TrainBase


class TrainCartpole(TrainBase):

    def __init__(self, train_dynamics, eval_dynamics, config,
                 train_image_dyn=0, train_seq_dyn=0, swingup=0):
        self.swingup = swingup
        self.config = config
        super().__init__(train_dynamics, eval_dynamics, **self.config)
        if self.sample_in not in ("eval_env", "train_env"):
            raise ValueError("sample in must be one of eval_env, train_env")
        if train_image_dyn or train_seq_dyn:
            raise NotImplementedError(
                "image / sequence dynamics are outside the APG hot path")
        if self.train_mode != "concurrent":
            raise ValueError(
                "autoregressive / LSTM training is only implemented "
                "for the Quadrotor! Use concurrent as train mode"
            )
        self._eval_env = None

    @property
    def eval_env(self):
        """CartPoleEnv on the dynamics `sample_in` names (:44-49); made on
        first use (its construction draws np.random.rand(4), as there)."""
        if self._eval_env is None:
            dyn = (self.eval_dynamics if self.sample_in == "eval_env"
                   else self.train_dynamics)
            self._eval_env = CartPoleEnv(dyn, self.delta_t)
        return self._eval_env

    def initialize_model(self, base_model=None, state_data=None, device=None,
                         seed=0):
        device = torch.device(device or "cuda")
        self.net = base_model if base_model is not None else Net(
            self.state_size, self.horizon * self.action_dim)
        self.net.to(device)
        if state_data is None:
            state_data = SyntheticCartpoleDataset(
                int(self.config.get("sample_data", 1000)), seed=seed,
                device=device, dt=self.delta_t)
        self.state_data = state_data
        self.model_wrapped = CartpoleWrapper(self.net, **self.config)
        self.init_optimizer()
        if "thresh_div_start" in self.config:          # (:101)
            self.config["thresh_div"] = self.config["thresh_div_start"]

    def dataset_tensors(self):
        return (self.state_data.states, self.state_data.labels)

    def make_reference(self, current_state):
        """ref_k = s0 * (1 - k/(H-1)) for k < H-1, last row zero (:103-110)."""
        ref_states = torch.zeros(
            current_state.size()[0], self.horizon, self.state_size,
            device=current_state.device)
        for k in range(self.horizon - 1):
            ref_states[:, k] = (
                current_state * (1 - 1 / (self.horizon - 1) * k))
        return ref_states

    def learnt_simulator(self):
        """Is the train dynamics the trainable LearntCartpoleDynamics?"""
        from .dynamics.cartpole_dynamics import LearntCartpoleDynamics
        return isinstance(self.train_dynamics, LearntCartpoleDynamics)

    def learnt_fused(self, B):
        """The controller step through the learnt simulator as ONE launch
        (apg_cartpole_learnt_rollout_fwd_bwd) rather than H module steps:
        measured faster at every batch size timed (profiles/
        cartpole_learnt_timing.jsonl), so chosen whenever the horizon fits."""
        return self.horizon <= _capi.MAX_HORIZON

    def _controller_loss(self, current_state, action_seq):
        """scripts/train_cartpole.py:133-148: make_reference, H steps of the
        train dynamics, cartpole_loss_mpc."""
        if not self.learnt_simulator():
            return F.cartpole_rollout_loss(current_state, action_seq,
                                           self.delta_t, self.train_dynamics.params)
        if self.learnt_fused(current_state.shape[0]):
            return F.cartpole_learnt_rollout_loss(
                self.train_dynamics, current_state, action_seq, self.delta_t)
        ref_states = self.make_reference(current_state)
        states, s = [], current_state
        for k in range(action_seq.size()[1]):
            s = self.train_dynamics(s, action_seq[:, k], dt=self.delta_t)
            states.append(s)
        return cartpole_loss_mpc(torch.stack(states, 1), ref_states, action_seq)

    # simulator-fit phase of the stock LearntCartpoleDynamics (six [1]
    # parameters, 5 -> 64 -> 4 residual, one CUDA device): TrainBase's fused
    # step.  On by default: measured against the base method at B = 8, 64 and
    # 65 536 it is ahead by more than both ways' chunk spreads at every size
    # (profiles/cartpole_learnt_timing.jsonl, `fit_step`).
    fused_fit = True
    _fit_system = "cartpole"

    def _fit_eval_in_kernel(self, eval_dynamics):
        """A plain CartpoleDynamics is stepped inside the kernel."""
        from .dynamics.cartpole_dynamics import CartpoleDynamics
        return type(eval_dynamics) is CartpoleDynamics

    def _fused_fit_prestep(self, in_kernel):
        """Both dynamics' `timestamp` side effects are kept."""
        self.train_dynamics.timestamp += .05        # (the module's forward)
        if in_kernel:
            self.eval_dynamics.timestamp += .05     # (simulate_cartpole)

    def train_dynamics_model(self, current_state, action_seq):
        """scripts/train_base.py:160-186 for the cart-pole simulator.  The
        reference's regulariser reads linear_state_2.bias, which this network
        does not have: l2_lambda > 0 is refused, as it fails there.  Then
        TrainBase's fused step (functional.cartpole_learnt_fit_fwd_bwd) under
        the rule of `_fusable_fit`, else the base method."""
        if self.l2_lambda > 0 and self.learnt_simulator():
            raise ValueError("l2_lambda > 0 needs linear_state_2.bias, which "
                             "LearntCartpoleDynamics does not have: set l2_lambda 0")
        return self._fused_train_dynamics_model(current_state, action_seq)

    fused_policy = True   # controller step with the stock policy inside the call

    def _fusable_policy(self, in_state, current_state):
        """The fused controller step (functional.cartpole_policy_train_step)
        serves the stock simple_model.Net(4, horizon) - contiguous float32
        parameters that require grad - rolled out through the plain analytic
        CartpoleDynamics, with policy and batch on one CUDA device.  Anything
        else - a learnt simulator, another policy, `fused_policy` False - takes
        the tape: net(in_state.clone()), the fused rollout, loss.backward().
        On by default for every batch size, under the rule of `_fusable_fit`:
        measured against the tape at (B, H) = (8, 10), (64, 10), (64, 5) and
        (65 536, 10) it is ahead by more than both ways' chunk spreads at every
        size (profiles/cartpole_train_timing.jsonl)."""
        from .dynamics.cartpole_dynamics import CartpoleDynamics
        if not (self.fused_policy and self.action_dim == 1 and self.state_size == 4
                and type(self.train_dynamics) is CartpoleDynamics
                and F.cartpole_policy_fusable(self.net, self.horizon)):
            return False
        dev = self.net.fc0.weight.device
        return all(t.device == dev and t.dtype == torch.float32 and t.is_contiguous()
                   and t.dim() == 2 and t.shape[1] == 4 and t.shape[0] >= 1
                   and not t.requires_grad
                   for t in (in_state, current_state))

    def _fused_policy_step(self, in_state, current_state):
        """One controller step in one fused call: loss and every `.grad`, and -
        where `_in_kernel_update` allows it (one process, plain momentum SGD, no
        step hooks) - the optimizer's update inside the call; otherwise
        (all-reduce,) optimizer.step() as `_step` does.  `in_state` is read, not
        written: no clone."""
        names = _capi.CARTPOLE_POLICY_PARAMS
        upd = self._in_kernel_update(
            names=names, tensors=F._cartpole_policy_tensors(self.net))
        res = F.cartpole_policy_train_step(
            self.net, in_state, current_state, self.delta_t,
            self.train_dynamics.params, update=upd)
        return self._step_direct(res["loss"].reshape(()), res["grads"], res["flat"],
                                 stepped=upd is not None)

    fused_learnt_policy = False   # the same through a LearntCartpoleDynamics

    def _fusable_learnt_policy(self, in_state, current_state):
        """The fused controller step through the learnt simulator
        (functional.cartpole_learnt_policy_train_step) serves the stock
        simple_model.Net(4, horizon) rolled out through a stock
        LearntCartpoleDynamics, with policy, simulator and batch on one CUDA
        device - the tensor conditions of `_fusable_policy`.  Off unless
        `fused_learnt_policy` is set: a trainer nobody configured takes the
        tape, as before (timings: profiles/cartpole_learnt_train_timing.jsonl)."""
        if not (self.fused_learnt_policy and self.action_dim == 1 and self.state_size == 4
                and F.cartpole_learnt_fusable(self.train_dynamics)
                and F.cartpole_policy_fusable(self.net, self.horizon)):
            return False
        dev = self.net.fc0.weight.device
        return (self.train_dynamics.linear_state_1.weight.device == dev
                and all(t.device == dev and t.dtype == torch.float32 and t.is_contiguous()
                        and t.dim() == 2 and t.shape[1] == 4 and t.shape[0] >= 1
                        and not t.requires_grad
                        for t in (in_state, current_state)))

    def _fused_learnt_policy_step(self, in_state, current_state):
        """`_fused_policy_step` through the learnt simulator, which is read and
        left as it is (no gradient; its `timestamp` stays, as in the fused
        rollout of `_controller_loss`)."""
        upd = self._in_kernel_update(
            names=_capi.CARTPOLE_POLICY_PARAMS, tensors=F._cartpole_policy_tensors(self.net))
        res = F.cartpole_learnt_policy_train_step(
            self.net, self.train_dynamics, in_state, current_state, self.delta_t, update=upd)
        return self._step_direct(res["loss"].reshape(()), res["grads"], res["flat"],
                                 stepped=upd is not None)

    def run_epoch(self, train="controller", epoch=0):
        """scripts/train_cartpole.py:118-165.  train "dynamics" fits a
        learnable simulator (TrainBase.train_dynamics_model) on the policy's
        actions, computed without grad (the reference's next controller step
        zeroes the policy gradient they would leave).  `epoch` is accepted for
        TrainBase.run_dynamics and not used, as there."""
        if train == "dynamics" and not isinstance(self.train_dynamics, torch.nn.Module):
            raise NotImplementedError(
                "dynamics epochs need a learnable simulator (LearntCartpoleDynamics)")
        if train not in ("controller", "dynamics"):
            raise ValueError("train must be 'controller' or 'dynamics'")
        self.results_dict["trained"].append(train)
        running_loss = None
        i = -1
        for i, data in enumerate(self.trainloader, 0):
            in_state, current_state = data
            if train == "dynamics":
                with torch.no_grad():
                    actions = self.net(in_state.clone())
                action_seq = torch.reshape(
                    actions, (-1, self.horizon, self.action_dim))
                loss = self.train_dynamics_model(current_state, action_seq).detach()
                self.count_finetune_data += len(current_state)
                running_loss = loss if running_loss is None else running_loss + loss
                continue
            if self._fusable_policy(in_state, current_state):
                loss = self._fused_policy_step(in_state, current_state).detach()
                running_loss = loss if running_loss is None else running_loss + loss
                continue
            if self._fusable_learnt_policy(in_state, current_state):
                loss = self._fused_learnt_policy_step(in_state, current_state).detach()
                running_loss = loss if running_loss is None else running_loss + loss
                continue
            # the policy zeroes column 0 of its input in place: hand it a
            # private copy, as DataLoader collation does in the reference
            actions = self.net(in_state.clone())  # tanh output, no sigmoid
            action_seq = torch.reshape(
                actions, (-1, self.horizon, self.action_dim))
            self.optimizer_controller.zero_grad()
            loss = self._controller_loss(current_state, action_seq)
            loss = self._step(loss).detach()
            running_loss = loss if running_loss is None else running_loss + loss
        epoch_loss = float(running_loss.item()) / i
        self.results_dict["loss_" + train].append(epoch_loss)
        print(f"Loss ({train}): {round(epoch_loss, 2)}")
        return epoch_loss

    def evaluate_model(self, epoch):
        """scripts/train_cartpole.py:167-205: 10 test episodes (swing-up or
        balancing) in one launch, the statistics into results_dict, a
        checkpoint, the divergence-threshold ladder and the resampling of the
        data set.  Returns (mean_vel, std_vel)."""
        evaluator = Evaluator(self.model_wrapped, self.eval_env)
        if self.swingup:
            res_eval = evaluator.evaluate_swingup(nr_iters=10)
        else:
            res_eval = evaluator.evaluate_in_environment(nr_iters=10)
        success_mean = res_eval["mean_vel"]
        success_std = res_eval["std_vel"]
        for key, val in res_eval.items():
            self.results_dict[key].append(val)
        self.results_dict["evaluate_at"].append(epoch)
        self.save_model(epoch, success_mean, success_std)

        # increase thresholds
        if epoch % 3 == 0 and self.config["thresh_div"] < self.thresh_div_end:
            self.config["thresh_div"] += self.config["thresh_div_step"]
            print("Curriculum learning: increase divergence threshold to",
                  self.config["thresh_div"])

        if (epoch + 1) % self.resample_every == 0:
            print("resample data...")
            self.state_data.resample_data(
                self.config["sample_data"], self.config["thresh_div"])
            if self.trainloader.tensors[0] is not self.state_data.states:
                # a data set of another size: a loader over the new tensors
                ld = self.trainloader
                self.trainloader = TensorBatches(
                    self.dataset_tensors(), ld.batch_size, shuffle=ld.shuffle)
        return success_mean, success_std


def train_control(base_model, config, swingup=0, device=None):
    """scripts/train_cartpole.py:220-238: train a controller from scratch or
    from `base_model` (a state_dict checkpoint file, checkpoint.load_policy),
    evaluating before every epoch.  Quirk kept: the learning rate is forced to
    1e-5.  The base finalize (the reference's dereferences a None
    state_to_img_net)."""
    from .checkpoint import load_policy
    from .dynamics.cartpole_dynamics import CartpoleDynamics
    config["learning_rate_controller"] = 1e-5
    modified_params = config["modified_params"]
    train_dynamics = CartpoleDynamics(modified_params)
    eval_dynamics = CartpoleDynamics(modified_params, test_time=1)
    trainer = TrainCartpole(train_dynamics, eval_dynamics, config, swingup=swingup)
    net = None if base_model is None else load_policy(base_model, system="cartpole")
    trainer.initialize_model(net, device=device)
    try:
        for epoch in range(trainer.config["nr_epochs"]):
            trainer.evaluate_model(epoch)
            print()
            print("Epoch", epoch)
            trainer.run_epoch(train="controller")
    except KeyboardInterrupt:
        pass
    trainer.finalize()
    return trainer


def train_norm_dynamics(base_model, config, not_trainable="all", device=None,
                        fused_learnt_policy=False):
    """scripts/train_cartpole.py:245-262 (`-t adapt`): fit a
    LearntCartpoleDynamics to CartpoleDynamics(modified_params) for the first
    epochs, then train the controller through it (TrainBase.run_dynamics),
    evaluating in the LEARNT environment (sample_in "train_env").
    base_model: a state_dict checkpoint file (checkpoint.load_policy) or None.
    finalize saves the simulator's state_dict as `dynamics_model`.
    fused_learnt_policy: the trainer's flag of that name - the controller
    epochs take the fused step through the learnt simulator.  Returns the
    trainer."""
    from .checkpoint import load_policy
    from .dynamics.cartpole_dynamics import CartpoleDynamics, LearntCartpoleDynamics
    modified_params = config["modified_params"]
    config["sample_in"] = "train_env"
    config["thresh_div_start"] = 0.2
    config["train_dyn_every"] = 1
    dev = torch.device(device or "cuda")
    train_dyn = LearntCartpoleDynamics(not_trainable=not_trainable).to(dev)
    eval_dyn = CartpoleDynamics(modified_params=modified_params)
    trainer = TrainCartpole(train_dyn, eval_dyn, config)
    trainer.fused_learnt_policy = bool(fused_learnt_policy)
    net = None if base_model is None else load_policy(base_model, system="cartpole")
    trainer.initialize_model(net, device=dev)
    trainer.run_dynamics(config)
    return trainer
