#!/usr/bin/env python
"""Timing of the controller phase through the learnt fixed-wing simulator
(csrc/wing_learnt.hip), one JSON line per shape, each naming the box, appended
to profiles/wing_learnt_timing.jsonl:

  controller_step   one controller step of the adapt flow (policy forward,
                    H steps through LearntFixedWingDynamics,
                    fixed_wing_mpc_loss, backward to the policy parameters;
                    no optimizer step) through TrainFixedWing.
                    train_controller_model, two ways in the same build:
                    fused (apg_wing_learnt_rollout_fwd_bwd, fused_learnt =
                    True) and the module's step-by-step autograd unroll
                    (fused_learnt = False: H module calls, each with its
                    device-to-host read of the 50 physical parameters)
  shapes            B = 8, H = 10 (the reference's configs/wing_config.json);
                    B = 64, H = 20; B = 65 536, H = 10
Device events around each timed call, median (and minimum) over `--reps`
calls per way, taken in two alternating rounds, each after 5 untimed calls.
The simulator is the fitted module of G16
(tests/golden/learnt_wing.npz, `steps.w.`: a general inertia matrix and a
residual that matters).

    python tools/time_wing_learnt.py [--reps 50] [--box NAME] [--out FILE]
"""
import argparse
import json
import os
import platform
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DT = 0.05
SHAPES = ((8, 10), (64, 20), (65536, 10))


def box(args):
    if args.box:
        return args.box
    if torch.cuda.is_available():
        return torch.cuda.get_device_name(0)
    return platform.processor() or platform.machine()


def timed(fn, reps):
    """Per-call device-event times in us, after 5 untimed calls."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return times


def fitted(dev):
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
        LearntFixedWingDynamics)
    g = np.load(os.path.join(REPO, "tests", "golden", "learnt_wing.npz"))
    dyn = LearntFixedWingDynamics()
    dyn.load_state_dict({k[len("steps.w."):]: torch.from_numpy(g[k]) for k in g.files
                         if k.startswith("steps.w.")})
    return dyn.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--box", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "wing_learnt_timing.jsonl"))
    args = ap.parse_args()
    name = box(args)
    from apg_trajectory_tracking_amd import synthetic
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    from apg_trajectory_tracking_amd.models.hutter_model import Net
    from apg_trajectory_tracking_amd.train_fixed_wing import TrainFixedWing
    dev = torch.device("cuda:0")
    dyn = fitted(dev)     # (its parameters require grad, as in the trainer's flow)
    with open(args.out, "a") as out:
        for B, H in SHAPES:
            cfg = dict(delta_t=DT, delta_t_train=DT, epoch_size=B, self_play=0, batch_size=B,
                       state_size=12, horizon=H, ref_dim=3, action_dim=4,
                       train_mode="concurrent", system="wing", sample_in="train_env",
                       save_name="time_wing_learnt")
            t = TrainFixedWing(dyn, FixedWingDynamics(), cfg)
            torch.manual_seed(0)
            t.net = net = Net(9, 1, 3, 4 * H, conv=False).to(dev)
            t.optimizer_controller = torch.optim.SGD(net.parameters(), lr=0.0)
            t._step = lambda loss: (loss.backward(), loss)[1]    # no optimizer step
            d = synthetic.wing_batch(B, H, DT, seed=40)
            s0, ref = d["state0"].to(dev), d["ref"].to(dev)
            in_state, in_ref = s0[:, 3:].contiguous(), (ref[:, 0] - s0[:, :3]).contiguous()

            def step():
                plan = torch.sigmoid(net(in_state, in_ref))
                return t.train_controller_model(s0, plan.view(B, H, 4), in_ref, ref)
            # the two ways alternate (two rounds each), so that a drift of the
            # box shows up as a difference between a way's own rounds
            res = {"fused": [], "stepwise": []}
            rounds = {"fused": [], "stepwise": []}
            for _ in range(2):
                for key, flag in (("fused", True), ("stepwise", False)):
                    t.fused_learnt = flag
                    assert t._fusable_learnt() == flag
                    times = timed(step, max(args.reps // 2, 5))
                    res[key] += times
                    rounds[key].append(round(float(np.median(times)), 1))
                    res[key + "_loss"] = float(step().detach())
            med = {k: float(np.median(res[k])) for k in ("fused", "stepwise")}
            line = json.dumps(dict(
                tool="time_wing_learnt", box=name, what="controller_step", B=B, H=H,
                fused_us=round(med["fused"], 1), fused_us_min=round(min(res["fused"]), 1),
                fused_us_rounds=rounds["fused"],
                stepwise_us=round(med["stepwise"], 1),
                stepwise_us_min=round(min(res["stepwise"]), 1),
                stepwise_us_rounds=rounds["stepwise"],
                speedup=round(med["stepwise"] / med["fused"], 1),
                fused_loss=res["fused_loss"], stepwise_loss=res["stepwise_loss"]))
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
