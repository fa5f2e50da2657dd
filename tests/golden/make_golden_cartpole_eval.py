#!/usr/bin/env python
"""G19: recordings of the REAL cart-pole evaluator (Evaluator.
evaluate_in_environment / evaluate_swingup, scripts/evaluate_cartpole.py) with
the controller the reference ships (the `cartpole.w.*` state_dict of
checkpoints.npz, G9), written to tests/golden/cartpole_closed_loop.npz.

Run once, where the reference is importable, as:
    python tests/golden/make_golden_cartpole_eval.py
It imports the reference with the stubs of make_golden.py.  The file holds
arrays only: per case the start states, the state after every step and the
action applied, each flight's step count / success / upright flag, the
returned statistics and the next np.random.rand() after the call; plus one
construct_states output (distribution checks of the data set's resampling)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (stubs, sys.path, torch threads)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from neural_control.controllers.network_wrapper import CartpoleWrapper  # noqa: E402
from neural_control.dynamics.cartpole_dynamics import CartpoleDynamics  # noqa: E402
from neural_control.environments.cartpole_env import (  # noqa: E402
    CartPoleEnv, construct_states)
from neural_control.models.simple_model import Net as CartNet  # noqa: E402
from evaluate_cartpole import Evaluator  # noqa: E402

DT = 0.05          # configs/cartpole_config.json delta_t
T = 250            # max_steps of both evaluations


def shipped_net():
    ck = np.load(os.path.join(HERE, "checkpoints.npz"))
    sd = {k[len("cartpole.w."):]: torch.from_numpy(ck[k])
          for k in ck.files if k.startswith("cartpole.w.")}
    net = CartNet(4, sd["fc_out.weight"].shape[0])
    net.load_state_dict(sd)
    return net


class Recorder:
    """Wraps CartPoleEnv._step: the state entering the first step of a flight
    (after the reset / initialize_straight) and every state after a step."""

    def __init__(self, env):
        self.env, self.flights = env, []
        orig = env._step

        def step(action, *a, **k):
            if self.fresh:
                self.flights.append(dict(start=np.array(env.state, np.float32),
                                         states=[], actions=[]))
                self.fresh = False
            out = orig(action, *a, **k)
            f = self.flights[-1]
            f["states"].append(np.array(env.state, np.float32))
            f["actions"].append(float(np.asarray(action).reshape(-1)[0]))
            return out
        env._step = step
        for name in ("_reset_upright", "_reset_swingup"):
            fn = getattr(env, name)

            def reset(fn=fn):
                self.fresh = True
                return fn()
            setattr(env, name, reset)
        self.fresh = False


def fly(net, mode, seed, nr_iters, thresh_div=.21, straight=1, mp=None,
        burn_in=None):
    """One evaluator call recorded, then the same call again with
    return_success=1 (same seed: the same flights) for the per-flight flags."""
    res = {}
    for ret in (0, 1):
        np.random.seed(seed)
        env = CartPoleEnv(CartpoleDynamics(dict(mp or {})), DT, thresh_div=thresh_div)
        rec = Recorder(env)
        ev = Evaluator(CartpoleWrapper(net, horizon=10, action_dim=1), env)
        ev.initialize_straight = straight
        kw = dict(nr_iters=nr_iters, max_steps=T, return_success=ret)
        if burn_in is not None:
            kw["burn_in_steps"] = burn_in
        fn = ev.evaluate_swingup if mode == "swingup" else ev.evaluate_in_environment
        res[ret] = (fn(**kw), rec.flights, np.random.rand(), np.array(env.state))
    (stats, flights, nxt, env_state), (succ, flights1, nxt1, _) = res[0], res[1]
    assert nxt == nxt1 and len(flights) == len(flights1) == nr_iters
    for f, g in zip(flights, flights1):
        assert np.array_equal(np.array(f["states"]), np.array(g["states"]))
    steps = np.array([len(f["states"]) for f in flights], np.int32)
    states = np.zeros((nr_iters, T, 4), np.float32)
    actions = np.zeros((nr_iters, T), np.float32)
    for i, f in enumerate(flights):
        states[i, :steps[i]] = np.array(f["states"])
        actions[i, :steps[i]] = np.array(f["actions"])
    out = dict(start=np.array([f["start"] for f in flights]), steps=steps,
               states=states, actions=actions, next_rand=np.float64(nxt),
               env_state=env_state.astype(np.float64),
               seed=np.int64(seed), thresh_div=np.float64(thresh_div),
               straight=np.int64(straight), swingup=np.int64(mode == "swingup"),
               burn_in=np.int64(burn_in if burn_in is not None
                                else (100 if mode == "swingup" else 50)),
               masspole=np.float64((mp or {}).get("masspole", .1)),
               length=np.float64((mp or {}).get("length", .5)))
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
    net = shipped_net()
    torch.manual_seed(7)
    untrained = CartNet(4, 10)
    cases = {
        "balance_zero": fly(net, "balance", 11, 10),
        "balance_tight": fly(net, "balance", 12, 10, thresh_div=.002, straight=0),
        "balance_tight_mod": fly(net, "balance", 13, 10, thresh_div=.002, straight=0,
                                 mp={"masspole": .2, "length": .7}),
        "swingup": fly(net, "swingup", 14, 6),
        "swingup_untrained": fly(untrained, "swingup", 15, 4),
    }
    arrays = {}
    for name, d in cases.items():
        for k, v in d.items():
            arrays[f"{name}.{k}"] = v
        print(name, "steps", d["steps"].tolist(),
              "upright" if "upright" in d else "success",
              d.get("upright", d.get("success")).tolist())
    for k, v in untrained.state_dict().items():
        arrays["untrained.w." + k] = v.detach().numpy().copy()
    np.random.seed(16)
    cs = construct_states(400, DT, thresh_div=.11)
    arrays["construct.states"] = np.asarray(cs, np.float32)
    arrays["construct.thresh_div"] = np.float64(.11)
    arrays["construct.num"] = np.int64(400)
    mg.save("cartpole_closed_loop.npz", **arrays)


if __name__ == "__main__":
    main()
