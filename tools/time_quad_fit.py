#!/usr/bin/env python
"""Timing of one simulator-fit step of the learnt quadrotor
(TrainDrone.train_dynamics_model on LearntDynamics, optimizer step included),
one JSON line per batch size, each naming the box, appended to
profiles/quad_fit_timing.jsonl:

  fused      fused_fit = True: apg_quad_learnt_fit_fwd_bwd (csrc/quad_fit.hip)
             + the momentum-SGD launch
  unfused    fused_fit = False: TrainBase.train_dynamics_model - the module
             call (action transform, step kernel, residual in torch), the
             target step, the loss and the four norms, autograd with the
             closed-form reductions of _LearntStep.backward, the optimizer
  graph      the fused step captured once in a graph, replayed
  shapes     B = 8, 64 and 65 536, l2_lambda = 0.01

Clocks warmed by half a second of matrix products at the start and by `--warm`
untimed steps per way; then `--chunks` chunks per way, the ways alternating
chunk by chunk, each chunk 3 untimed steps and then `--calls` steps between two
device events (the second one synchronised).  Reported: the median over a
way's chunks of the per-step time, the minimum, and the spread (largest minus
smallest chunk) - a difference between two ways below their spreads is none.
The simulator starts from the fitted module of G10 (tests/golden/
learnt_dynamics.npz, `steps.w.`: a residual that matters) and is restored
before every chunk, so every chunk times the same arithmetic.

    python tools/time_quad_fit.py [--chunks 9] [--calls 20] [--box NAME] [--out FILE]
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

DT = 0.1
SIZES = (8, 64, 65536)
INIT = {"rotational_drag": [.01, .02, .03]}
MOD = dict(translational_drag=[.1, .2, .3], rotational_drag=[.01, .02, .03], mass=1.0)


def box(args):
    if args.box:
        return args.box
    if torch.cuda.is_available():
        return torch.cuda.get_device_name(0)
    return platform.processor() or platform.machine()


def fitted_weights():
    g = np.load(os.path.join(REPO, "tests", "golden", "learnt_dynamics.npz"))
    return {k[len("steps.w."):]: torch.from_numpy(g[k]) for k in g.files
            if k.startswith("steps.w.")}


def warm_clocks(dev, seconds=0.5):
    import time
    x = torch.randn(4096, 4096, device=dev)
    end = time.time() + seconds
    while time.time() < end:
        for _ in range(10):
            x @ x
        torch.cuda.synchronize()


def chunk_us(fn, calls):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--box", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "quad_fit_timing.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_quad_fit.py measures on the GPU: none found")
    name = box(args)
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    from apg_trajectory_tracking_amd.train_base import momentum_sgd
    from apg_trajectory_tracking_amd.train_drone import TrainDrone
    dev = torch.device("cuda:0")
    start = {k: v.to(dev) for k, v in fitted_weights().items()}
    warm_clocks(dev)
    with open(args.out, "a") as out:
        for B in SIZES:
            cfg = dict(delta_t=DT, delta_t_train=DT, epoch_size=B, self_play=0, batch_size=B,
                       state_size=12, horizon=10, ref_dim=9, action_dim=4,
                       train_mode="concurrent", system="quad", sample_in="train_env",
                       learning_rate_dynamics=1e-7, l2_lambda=0.01, save_name="time_quad_fit")
            gen = torch.Generator().manual_seed(62)      # G10's recipe
            s0 = torch.randn(B, 12, generator=gen)
            s0[:, 3:6] *= 0.4
            s0 = s0.to(dev)
            actions = torch.rand(B, 10, 4, generator=gen).to(dev)
            ways = {}
            for key in ("fused", "unfused", "graph"):
                dyn = LearntDynamics(initial_params=dict(INIT)).to(dev)
                dyn.load_state_dict(start)
                t = TrainDrone(dyn, FlightmareDynamics(modified_params=dict(MOD)), dict(cfg))
                t.optimizer_dynamics = momentum_sgd(dyn.parameters(), 1e-7)
                t.grad_sync_dynamics = None
                t.fused_fit = key != "unfused"
                assert t._fusable_fit(s0, actions) == t.fused_fit
                step = lambda t=t: t.train_dynamics_model(s0, actions)
                for _ in range(args.warm):
                    step()
                torch.cuda.synchronize()
                loss = float(t.results_dict["loss_dyn_per_step"][-1])
                if key == "graph":
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        step()
                    step = graph.replay
                    for _ in range(args.warm):
                        step()
                    torch.cuda.synchronize()
                ways[key] = dict(step=step, dyn=dyn, trainer=t, loss=loss, chunks=[])
            for _ in range(args.chunks):          # the ways alternate chunk by chunk
                for key, w in ways.items():
                    with torch.no_grad():
                        for k, v in w["dyn"].state_dict().items():
                            v.copy_(start[k])
                    del w["trainer"].results_dict["loss_dyn_per_step"][:]
                    w["chunks"].append(chunk_us(w["step"], args.calls))
            rec = dict(tool="time_quad_fit", box=name, what="fit_step", B=B, l2_lambda=0.01,
                       chunks=args.chunks, calls=args.calls)
            for key, w in ways.items():
                c = w["chunks"]
                rec[key + "_us"] = round(float(np.median(c)), 1)
                rec[key + "_us_min"] = round(min(c), 1)
                rec[key + "_us_spread"] = round(max(c) - min(c), 1)
                rec[key + "_loss"] = w["loss"]
            rec["speedup"] = round(rec["unfused_us"] / rec["fused_us"], 2)
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
