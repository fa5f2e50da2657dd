#!/usr/bin/env python
"""Timing of one controller step of the cart-pole trainer THROUGH THE LEARNT
SIMULATOR (the body of TrainCartpole.run_epoch's controller branch with a
LearntCartpoleDynamics as train dynamics: policy forward, H learnt steps,
cartpole_loss_mpc, backward through rollout and policy, momentum SGD), one JSON
line per size, each naming the box, appended to `--out`:

  tape     fused_learnt_policy = False (the default): net(in_state.clone())
           under autograd, the fused learnt rollout launch, loss.backward(),
           optimizer.step()
  fused    fused_learnt_policy = True: apg_cartpole_learnt_mlp_train_step with
           the update inside the call (csrc/cartpole_train.hip)
  graph    the fused step captured once, replayed

at (B, H) = (8, 10), (64, 10) and (65 536, 10).  Measured as
tools/time_cartpole_train.py measures: `--chunks` chunks per way, the ways
alternating chunk by chunk, each chunk 3 untimed steps and `--calls` steps
between two device events (chunks x calls >= 200); reported: median, mean,
minimum and spread (largest minus smallest chunk) per way - a difference between
two ways below their spreads is none.  Parameters and momentum buffers are
restored before every chunk.

    python tools/time_cartpole_learnt_train.py [--chunks 9] [--calls 25] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_cartpole_train import DT, chunk_us, tape_step, warm_clocks  # noqa: E402

SIZES = ((8, 10), (64, 10), (65536, 10))


def simulator(dev):
    """A LearntCartpoleDynamics whose residual is large enough to matter."""
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        LearntCartpoleDynamics)
    torch.manual_seed(11)
    m = LearntCartpoleDynamics()
    with torch.no_grad():
        m.linear_state_1.weight.normal_(0, .3)
        m.linear_state_1.bias.normal_(0, .2)
        m.linear_state_2.weight.normal_(0, .01)
    return m.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", default=None)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "cartpole_learnt_train_timing.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cartpole_learnt_train.py measures on the GPU: none found")
    from apg_trajectory_tracking_amd import synthetic
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.models.simple_model import Net
    from apg_trajectory_tracking_amd.train_cartpole import TrainCartpole
    dev = torch.device("cuda:0")
    name = args.box or torch.cuda.get_device_name(0)
    warm_clocks(dev)
    with open(args.out, "a") as out:
        for B, H in SIZES:
            cfg = dict(delta_t=DT, batch_size=B, state_size=4, horizon=H, action_dim=1,
                       ref_dim=4, train_mode="concurrent", learning_rate_controller=1e-9,
                       learning_rate_dynamics=1e-3, l2_lambda=0, system="cartpole",
                       save_name="time_cartpole_learnt_train")
            s0 = synthetic.cartpole_batch(B, H, seed=100 + B)["state0"].float().to(dev)
            x = s0.clone()

            class Data:
                states, labels, num_sampled_states = x, s0, B
            torch.manual_seed(33)
            start = Net(4, H).state_dict()
            ways = {}
            for key in ("tape", "fused", "graph"):
                net = Net(4, H)
                net.load_state_dict(start)
                t = TrainCartpole(simulator(dev), CartpoleDynamics(), dict(cfg))
                t.initialize_model(base_model=net, state_data=Data, device=dev)
                t.fused_learnt_policy = key != "tape"
                assert not t._fusable_policy(x, s0)
                assert t._fusable_learnt_policy(x, s0) == t.fused_learnt_policy
                if key == "tape":
                    step = lambda t=t: tape_step(t, x, s0)
                else:
                    step = lambda t=t: t._fused_learnt_policy_step(x, s0)
                for _ in range(args.warm):
                    loss = step()
                torch.cuda.synchronize()
                loss = float(loss)
                if key == "graph":
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        step()
                    step = graph.replay
                    for _ in range(args.warm):
                        step()
                    torch.cuda.synchronize()
                ways[key] = dict(step=step, trainer=t, loss=loss, chunks=[])
            for _ in range(args.chunks):          # the ways alternate chunk by chunk
                for key, w in ways.items():
                    t = w["trainer"]
                    with torch.no_grad():
                        for k, v in t.net.state_dict().items():
                            v.copy_(start[k])
                        for st in t.optimizer_controller.state.values():
                            if torch.is_tensor(st.get("momentum_buffer")):
                                st["momentum_buffer"].zero_()
                    w["chunks"].append(chunk_us(w["step"], args.calls))
            rec = dict(tool="time_cartpole_learnt_train", box=name,
                       what="learnt_controller_step", B=B, H=H, chunks=args.chunks,
                       calls=args.calls, launches=1 if B <= 64 else 2)
            for key, w in ways.items():
                c = w["chunks"]
                rec[key + "_us"] = round(float(np.median(c)), 1)
                rec[key + "_us_mean"] = round(float(np.mean(c)), 1)
                rec[key + "_us_min"] = round(min(c), 1)
                rec[key + "_us_spread"] = round(max(c) - min(c), 1)
                rec[key + "_loss"] = w["loss"]
            rec["speedup"] = round(rec["tape_us"] / rec["fused_us"], 2)
            rec["ahead_by_more_than_both_spreads"] = bool(
                rec["tape_us"] - rec["fused_us"]
                > max(rec["fused_us_spread"], rec["tape_us_spread"]))
            text = json.dumps(rec)
            print(text, flush=True)
            out.write(text + "\n")
            out.flush()


if __name__ == "__main__":
    main()
