#!/usr/bin/env python
"""G20: recordings of the REAL LearntCartpoleDynamics (neural_control/dynamics/
cartpole_dynamics.py:122-140) and of the adapt flow around it, written to
tests/golden/cartpole_learnt.npz.

Run once, where the reference is importable, as:
    python tests/golden/make_golden_cartpole_learnt.py
It imports the reference with the stubs of make_golden.py.  The file holds
arrays only:
  init.<key>         state_dict of LearntCartpoleDynamics() after
                     torch.manual_seed(INIT_SEED) (the init draws' order)
  fit.<key>          the "fitted" module: six parameters perturbed, residual
                     weights large enough to matter
  step.*             a batch of (state, action) pairs: the module's forward,
                     simulate_cartpole, the target CartpoleDynamics(MOD), the
                     summed squared error, every parameter's gradient + has-grad
                     flags (both not_trainable settings), dL/dstate, dL/daction
  train_<tag>.*      5 train_dynamics_model steps (scripts/train_base.py:160-186,
                     momentum SGD as init_optimizer builds it) from a seeded
                     module: losses and the state_dict after each step
  ctrl<B>.*          the controller branch of TrainCartpole.run_epoch
                     (scripts/train_cartpole.py:127-150) through the fitted
                     module with the shipped controller (G9), H = 10: loss and
                     policy gradients
  <case>.*           flights of the real Evaluator in CartPoleEnv(fitted
                     module), the fields of G19 (make_golden_cartpole_eval.py)
  (the balance cases use thresh_div 0.1 so that some flights fail and some
  do not; <case>.seconds is the reference's batch-1 CPU time for the call)."""
import os
import sys
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (stubs, sys.path, torch threads)
import make_golden_cartpole_eval as mge  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

from neural_control.controllers.network_wrapper import CartpoleWrapper  # noqa: E402
from neural_control.drone_loss import cartpole_loss_mpc  # noqa: E402
from neural_control.dynamics.cartpole_dynamics import (  # noqa: E402
    CartpoleDynamics, LearntCartpoleDynamics)
from neural_control.environments.cartpole_env import CartPoleEnv  # noqa: E402
from evaluate_cartpole import Evaluator  # noqa: E402

DT = 0.05
T = 250
INIT_SEED = 3
MOD = {"masspole": .2, "length": .7}
# the fitted module: physical parameters moved, residual weights scaled up
FIT_PARAMS = {"max_force_mag": 27.0, "masspole": 0.13, "length": 0.55,
              "friction": 0.45, "total_mass": 1.2, "polemass_length": 0.06}
FIT_STD = {"linear_state_1.weight": 0.5, "linear_state_1.bias": 0.3,
           "linear_state_2.weight": 0.01}


def fitted_module(not_trainable=()):
    torch.manual_seed(11)
    m = LearntCartpoleDynamics(not_trainable=list(not_trainable))
    with torch.no_grad():
        for k, v in FIT_PARAMS.items():
            m.cfg[k].fill_(v)
        m.linear_state_1.weight.normal_(0, FIT_STD["linear_state_1.weight"])
        m.linear_state_1.bias.normal_(0, FIT_STD["linear_state_1.bias"])
        m.linear_state_2.weight.normal_(0, FIT_STD["linear_state_2.weight"])
    return m


def state_batch(n, seed):
    """States across the range, theta near +-pi and large theta_dot
    included; actions in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    s = (torch.rand(n, 4, generator=g) * 2 - 1) * torch.tensor([2.4, 7.5, np.pi, 7.5])
    q = n // 8
    s[:q, 2] = np.pi - torch.rand(q, generator=g) * 1e-3
    s[q:2 * q, 2] = -np.pi + torch.rand(q, generator=g) * 1e-3
    s[2 * q:3 * q, 3] = (torch.rand(q, generator=g) * 2 - 1) * 25
    a = torch.rand(n, 1, generator=g) * 2 - 1
    return s.float(), a.float()


def sd_np(m, prefix):
    return {prefix + k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


def step_case():
    out = {}
    s, a = state_batch(256, 5)
    target = CartpoleDynamics(MOD)(s, a, dt=DT)
    out["step.state"], out["step.action"] = s.numpy(), a.numpy()
    out["step.target"] = target.numpy()
    for tag, nt in (("", []), ("_frozen", "all")):
        m = fitted_module()
        if nt == "all":
            for p in m.cfg.values():
                p.requires_grad_(False)
        sv, av = s.clone().requires_grad_(True), a.clone().requires_grad_(True)
        pred = m(sv, av, dt=DT)
        loss = torch.sum((pred - target)**2)
        loss.backward()
        if not tag:
            out["step.forward"] = mg.npy(pred)
            with torch.no_grad():
                out["step.simulate"] = mg.npy(m.simulate_cartpole(s, a, DT))
            out["step.loss"] = np.float64(loss.item())
            out["step.grad_state"] = mg.npy(sv.grad)
            out["step.grad_action"] = mg.npy(av.grad)
        for k, p in m.named_parameters():
            out[f"step{tag}.has_grad.{k}"] = np.int64(p.grad is not None)
            if p.grad is not None:
                out[f"step{tag}.grad.{k}"] = mg.npy(p.grad)
    return out


def train_case(tag, not_trainable):
    """Five train_dynamics_model steps (scripts/train_base.py:160-186) with
    the optimizer of init_optimizer (:144-150) for the learnt class."""
    import train_base
    torch.manual_seed(21)
    m = LearntCartpoleDynamics(not_trainable=not_trainable)
    s, a = state_batch(16, 6)
    action_seq = a[:, None, :].repeat(1, 10, 1)
    tr = types.SimpleNamespace(
        train_dynamics=m, eval_dynamics=CartpoleDynamics(MOD), delta_t=DT, l2_lambda=0,
        results_dict={"loss_dyn_per_step": []},
        optimizer_dynamics=torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9))
    out = {f"train_{tag}.state": s.numpy(), f"train_{tag}.action": a.numpy()}
    losses = []
    for k in range(5):
        loss = train_base.TrainBase.train_dynamics_model(tr, s, action_seq)
        losses.append(loss.item())
        for key, v in m.state_dict().items():
            out[f"train_{tag}.after{k}.{key}"] = v.detach().numpy().copy()
    out[f"train_{tag}.losses"] = np.array(losses, np.float64)
    return out


def ctrl_case(B):
    """The controller branch through the fitted module (run_epoch,
    scripts/train_cartpole.py:127-155 up to loss.backward())."""
    net = mge.shipped_net()
    m = fitted_module()
    for p in m.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(100 + B)
    s = ((torch.rand(B, 4, generator=g) * 2 - 1)
         * torch.tensor([1.0, 1.0, 0.3, 1.0])).float()
    H = 10
    current_state = s.clone()
    actions = net(s.clone())          # (the in-place zeroing hits the copy)
    action_seq = torch.reshape(actions, (-1, H, 1))
    ref = torch.zeros(B, H, 4)
    for k in range(H - 1):
        ref[:, k] = current_state * (1 - 1 / (H - 1) * k)
    inter = torch.zeros(B, H, 4)
    for k in range(H):
        current_state = m(current_state, action_seq[:, k], dt=DT)
        inter[:, k] = current_state
    loss = cartpole_loss_mpc(inter, ref, action_seq)
    loss.backward()
    out = {f"ctrl{B}.state": s.numpy(), f"ctrl{B}.loss": np.float64(loss.item())}
    for k, p in net.named_parameters():
        out[f"ctrl{B}.grad.{k}"] = mg.npy(p.grad)
    return out


def fly(mode, seed, nr_iters, straight=0, burn_in=None, thresh_div=.21):
    """mge.fly in CartPoleEnv(fitted module)."""
    net = mge.shipped_net()
    res = {}
    for ret in (0, 1):
        np.random.seed(seed)
        env = CartPoleEnv(fitted_module(), DT, thresh_div=thresh_div)
        rec = mge.Recorder(env)
        ev = Evaluator(CartpoleWrapper(net, horizon=10, action_dim=1), env)
        ev.initialize_straight = straight
        kw = dict(nr_iters=nr_iters, max_steps=T, return_success=ret)
        if burn_in is not None:
            kw["burn_in_steps"] = burn_in
        fn = ev.evaluate_swingup if mode == "swingup" else ev.evaluate_in_environment
        t0 = time.perf_counter()
        r = fn(**kw)
        dt_s = time.perf_counter() - t0
        res[ret] = (r, rec.flights, np.random.rand(), np.array(env.state), dt_s)
    (stats, flights, nxt, env_state, secs), (succ, flights1, nxt1, _, _) = res[0], res[1]
    assert nxt == nxt1 and len(flights) == len(flights1) == nr_iters
    steps = np.array([len(f["states"]) for f in flights], np.int32)
    states = np.zeros((nr_iters, T, 4), np.float32)
    actions = np.zeros((nr_iters, T), np.float32)
    for i, f in enumerate(flights):
        states[i, :steps[i]] = np.array(f["states"])
        actions[i, :steps[i]] = np.array(f["actions"])
    out = dict(start=np.array([f["start"] for f in flights]), steps=steps,
               states=states, actions=actions, next_rand=np.float64(nxt),
               env_state=env_state.astype(np.float64), seed=np.int64(seed),
               thresh_div=np.float64(thresh_div), straight=np.int64(straight),
               swingup=np.int64(mode == "swingup"),
               burn_in=np.int64(burn_in if burn_in is not None
                                else (100 if mode == "swingup" else 50)),
               seconds=np.float64(secs))
    if mode == "swingup":
        out["upright"] = np.asarray(succ, np.int32)
        out["mean_vel"] = np.float64(stats["mean_vel"])
        out["std_vel"] = np.float64(stats["std_vel"])
    else:
        out["success"] = np.asarray(succ[0], np.int32)
        for k in ("mean_vel", "std_vel", "mean_stable", "std_stable"):
            out[k] = np.float64(stats[k])
    return out


def main():
    arrays = {}
    torch.manual_seed(INIT_SEED)
    arrays.update(sd_np(LearntCartpoleDynamics(), "init."))
    arrays["init.seed"] = np.int64(INIT_SEED)
    arrays["init.keys"] = np.array(list(LearntCartpoleDynamics().state_dict().keys()))
    arrays.update(sd_np(fitted_module(), "fit."))
    arrays.update(step_case())
    arrays.update(train_case("all", []))
    arrays.update(train_case("frozen", "all"))
    for B in (8, 64):
        arrays.update(ctrl_case(B))
    cases = {"learnt_balance_a": fly("balance", 31, 10, thresh_div=.1),
             "learnt_balance_b": fly("balance", 32, 10, thresh_div=.1),
             "learnt_swingup": fly("swingup", 33, 10)}
    for name, d in cases.items():
        for k, v in d.items():
            arrays[f"{name}.{k}"] = v
        print(name, "steps", d["steps"].tolist(),
              "upright" if "upright" in d else "success",
              d.get("upright", d.get("success")).tolist(), f"{d['seconds']:.2f} s")
    print("train losses", arrays["train_all.losses"], arrays["train_frozen.losses"])
    mg.save("cartpole_learnt.npz", **arrays)


if __name__ == "__main__":
    main()
