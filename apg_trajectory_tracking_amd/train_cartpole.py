"""Drop-in for scripts/train_cartpole.py:30-165 (`TrainCartpole`) restricted
to the APG hot path: `run_epoch` (:118-165) with `make_reference` (:103-110).
The controller branch is one fused HIP launch (make_reference + H x cartpole
dynamics + cartpole_loss_mpc + adjoint).  Quirks kept: the policy ends in
tanh with NO sigmoid (:127-130), `simple_model.Net` zeroes column 0 of its
input in place, run_epoch has no `epoch` argument and divides by the last
batch index (:163).

The evaluation side (:167-205, :220-238): `evaluate_model` flies the trainer's
10 test episodes through evaluate_cartpole.Evaluator - one kernel launch -
and runs the divergence-threshold ladder and the resampling of the data set
(SyntheticCartpoleDataset.resample_data); `train_control` is the training
loop around it."""
import torch

from . import functional as F
from .dataset import SyntheticCartpoleDataset, TensorBatches
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

    def run_epoch(self, train="controller"):
        if train != "controller":
            raise NotImplementedError(
                "learnt-dynamics training is outside the APG hot path")
        self.results_dict["trained"].append(train)
        running_loss = None
        i = -1
        for i, data in enumerate(self.trainloader, 0):
            in_state, current_state = data
            # the policy zeroes column 0 of its input in place: hand it a
            # private copy, as DataLoader collation does in the reference
            actions = self.net(in_state.clone())  # tanh output, no sigmoid
            action_seq = torch.reshape(
                actions, (-1, self.horizon, self.action_dim))
            self.optimizer_controller.zero_grad()
            loss = F.cartpole_rollout_loss(
                current_state, action_seq, self.delta_t,
                self.train_dynamics.params)
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
