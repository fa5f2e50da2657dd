#!/usr/bin/env python
"""Timing of one controller step of the fixed-wing trainer THROUGH THE LEARNT
SIMULATOR (the body of TrainBase.run_epoch's concurrent branch with a
LearntFixedWingDynamics as train dynamics - the controller phase of the adapt
flow: policy forward, ten learnt steps, fixed_wing_mpc_loss, backward through
rollout and policy, momentum SGD), one JSON line per size, each naming the box,
appended to `--out`:

  tape     fused_learnt_policy = False (the default): sigmoid(net(...)) under
           autograd, the fused learnt rollout launch
           (apg_wing_learnt_rollout_fwd_bwd), loss.backward(), optimizer.step()
  fused    fused_learnt_policy = True: apg_wing_learnt_mlp_train_step with the
           update inside the call (csrc/mlp_wing.hip); the layout change of the
           batch (functional.to_soa_multi) is part of it
  graph    the fused step captured once, replayed

at B = 8, 64 and 65 536, H = 10.  Measured as tools/time_cartpole_train.py
measures: `--chunks` chunks per way, the ways alternating chunk by chunk, each
chunk 3 untimed steps and `--calls` steps between two device events (chunks x
calls >= 200); reported: median, mean, minimum and spread (largest minus smallest
chunk) per way - a difference between two ways below their spreads is none.
Parameters and momentum buffers are restored before every chunk.  The simulator
is the recorded module after the reference's own optimizer steps
(tests/golden/learnt_wing.npz, `steps.w.`: a general inertia matrix and a
residual that matters).

    python tools/time_wing_learnt_train.py [--chunks 9] [--calls 25] [--out FILE]
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

from time_cartpole_train import chunk_us, warm_clocks  # noqa: E402

SIZES = (8, 64, 65536)
H, DT = 10, 0.05


def simulator(dev):
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
        LearntFixedWingDynamics)
    g = np.load(os.path.join(REPO, "tests", "golden", "learnt_wing.npz"))
    dyn = LearntFixedWingDynamics()
    dyn.load_state_dict({k[len("steps.w."):]: torch.from_numpy(g[k]) for k in g.files
                         if k.startswith("steps.w.")})
    return dyn.to(dev)


def tape_step(t, batch):
    """run_epoch's concurrent branch for one batch, fused_learnt_policy False."""
    in_state, state0, in_ref, ref = batch
    plan = torch.sigmoid(t.net(in_state, in_ref))
    return t.train_controller_model(state0, plan.view(-1, t.horizon, t.action_dim),
                                    in_ref, ref).detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", default=None)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "wing_learnt_train_timing.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_wing_learnt_train.py measures on the GPU: none found")
    from apg_trajectory_tracking_amd import synthetic
    from apg_trajectory_tracking_amd.dataset import SyntheticWingDataset
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    from apg_trajectory_tracking_amd.models.hutter_model import Net
    from apg_trajectory_tracking_amd.train_fixed_wing import TrainFixedWing
    dev = torch.device("cuda:0")
    name = args.box or torch.cuda.get_device_name(0)
    warm_clocks(dev)
    mean = torch.tensor(SyntheticWingDataset.MEAN).float()
    std = torch.tensor(SyntheticWingDataset.STD).float()
    with open(args.out, "a") as out:
        for B in SIZES:
            cfg = dict(delta_t=DT, delta_t_train=DT, epoch_size=B, self_play=0, batch_size=B,
                       state_size=12, horizon=H, train_mode="concurrent", ref_dim=3,
                       action_dim=4, learning_rate_controller=1e-12,
                       learning_rate_dynamics=1e-4, system="wing", sample_in="train_env",
                       save_name="time_wing_learnt_train")
            d = synthetic.wing_batch(B, H, DT, seed=100 + (B % 1000))
            normed = ((d["state0"] - mean) / std)[:, 3:]
            in_ref = d["ref"][:, -1] - d["state0"][:, :3]
            batch = tuple(v.to(dev).contiguous() for v in (normed, d["state0"], in_ref, d["ref"]))

            class Data:
                num_sampled_states = B
            (Data.normed_states, Data.states, Data.in_ref_states, Data.ref_states) = batch
            torch.manual_seed(33)
            start = Net(9, 1, 3, 4 * H, conv=False).state_dict()
            ways = {}
            for key in ("tape", "fused", "graph"):
                net = Net(9, 1, 3, 4 * H, conv=False)
                net.load_state_dict(start)
                t = TrainFixedWing(simulator(dev), FixedWingDynamics(), dict(cfg))
                t.state_data = Data
                t.net = net.to(dev)
                t.init_optimizer()
                t.fused_learnt_policy = key != "tape"
                assert t.train_concurrent_fused(None, None, None, None, probe=True) is False
                assert t._fusable_learnt_policy() == t.fused_learnt_policy
                if key == "tape":
                    step = lambda t=t: tape_step(t, batch)
                else:
                    step = lambda t=t: t.train_concurrent_fused(*batch).detach()
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
            rec = dict(tool="time_wing_learnt_train", box=name,
                       what="learnt_controller_step", B=B, H=H, chunks=args.chunks,
                       calls=args.calls)
            for key, w in ways.items():
                c = w["chunks"]
                rec[key + "_us"] = round(float(np.median(c)), 1)
                rec[key + "_us_mean"] = round(float(np.mean(c)), 1)
                rec[key + "_us_min"] = round(min(c), 1)
                rec[key + "_us_spread"] = round(max(c) - min(c), 1)
                rec[key + "_loss"] = w["loss"]
            rec["speedup"] = round(rec["tape_us"] / rec["fused_us"], 2)
            rec["graph_speedup"] = round(rec["tape_us"] / rec["graph_us"], 2)
            rec["ahead_by_more_than_both_spreads"] = bool(
                rec["tape_us"] - rec["fused_us"]
                > max(rec["fused_us_spread"], rec["tape_us_spread"]))
            text = json.dumps(rec)
            print(text, flush=True)
            out.write(text + "\n")
            out.flush()


if __name__ == "__main__":
    main()
