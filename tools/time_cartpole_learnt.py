#!/usr/bin/env python
"""Timing of the learnt cart-pole path (csrc/cartpole_learnt.hip and the
learnt closed loop), one JSON line per measurement, each naming the box:

  controller   one controller step of the adapt flow through the learnt
               simulator (policy forward, H = 10 steps, cartpole_loss_mpc,
               backward): fused (apg_cartpole_learnt_rollout_fwd_bwd, one
               launch) against the module's step-by-step autograd unroll, at
               B = 8 (the config's batch) and 65 536
  fit          one train_dynamics_model step (forward, eval target, loss,
               backward with all 646 parameter gradients, momentum SGD)
  closed_loop  learnt against analytic closed loop, 10 and 65 536 balance
               flights of 250 steps from the zero start
  fit_step     (--fit, measured as tools/time_quad_fit.py measures) one
               TrainCartpole.train_dynamics_model step, optimizer included, at
               B = 8, 64 and 65 536 three ways: fused (fused_fit = True:
               apg_cartpole_learnt_fit_fwd_bwd + the momentum-SGD launch),
               unfused (fused_fit = False: the base method - module forward,
               eval step, loss in torch, autograd, optimizer) and graph (the
               fused step captured once, replayed).  `--chunks` chunks per way,
               the ways alternating chunk by chunk, each chunk 3 untimed steps
               and `--calls` steps between two device events; reported: median,
               minimum and spread (largest minus smallest chunk) per way - a
               difference between two ways below their spreads is none.  The
               module is restored before every chunk.  Appended to `--out`.
Device events around each timed call, median over `--reps`, after 5 untimed
calls.  The reference's batch-1 CPU loop is not timed here (the reference is
not on a GPU box): tests/golden/make_golden_cartpole_learnt.py records its
time per evaluator call in G20 (`<case>.seconds`); `--reference-cpu` prints
that as a line of its own, labelled as a CPU measurement.

    python tools/time_cartpole_learnt.py [--reps 50] [--box NAME]
    python tools/time_cartpole_learnt.py --reference-cpu [--box NAME]
    python tools/time_cartpole_learnt.py --fit [--chunks 9] [--calls 20] [--out FILE]
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
sys.path.insert(0, os.path.join(REPO, "tests"))

DT, H, T = 0.05, 10, 250


def box(args):
    if args.box:
        return args.box
    if torch.cuda.is_available():
        return torch.cuda.get_device_name(0)
    return platform.processor() or platform.machine()


def timed(fn, reps):
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
    return float(np.median(times)), float(np.min(times))


def fitted(dev):
    from test_cartpole_learnt_cpu import fitted as fit, g20
    return fit(g20()).to(dev)


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


def time_fit(args, name):
    """The fit step three ways at three sizes, one JSON line per size."""
    if not torch.cuda.is_available():
        raise SystemExit("time_cartpole_learnt.py --fit measures on the GPU: none found")
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.train_base import momentum_sgd
    from apg_trajectory_tracking_amd.train_cartpole import TrainCartpole
    dev = torch.device("cuda:0")
    start = {k: v.clone() for k, v in fitted(dev).state_dict().items()}
    warm_clocks(dev)
    with open(args.out, "a") as out:
        for B in (8, 64, 65536):
            cfg = {"system": "cartpole", "delta_t": DT, "state_size": 4, "batch_size": B,
                   "nr_epochs": 1, "sample_in": "train_env", "horizon": H, "action_dim": 1,
                   "l2_lambda": 0, "learning_rate_dynamics": 1e-9,
                   "save_name": "time_cartpole_fit"}
            gen = torch.Generator().manual_seed(5)           # G20's step recipe
            s0 = ((torch.rand(B, 4, generator=gen) * 2 - 1)
                  * torch.tensor([2.4, 7.5, np.pi, 7.5])).to(dev)
            seq = (torch.rand(B, H, 1, generator=gen) * 2 - 1).to(dev)
            ways = {}
            for key in ("fused", "unfused", "graph"):
                dyn = fitted(dev)
                t = TrainCartpole(dyn, CartpoleDynamics({"masspole": .2, "length": .7}),
                                  dict(cfg))
                t.optimizer_dynamics = momentum_sgd(dyn.parameters(), 1e-9)
                t.grad_sync_dynamics = None
                t.fused_fit = key != "unfused"
                assert t._fusable_fit(s0, seq) == t.fused_fit
                step = lambda t=t: t.train_dynamics_model(s0, seq)
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
            rec = dict(tool="time_cartpole_learnt", box=name, what="fit_step", B=B,
                       chunks=args.chunks, calls=args.calls)
            for key, w in ways.items():
                c = w["chunks"]
                rec[key + "_us"] = round(float(np.median(c)), 1)
                rec[key + "_us_min"] = round(min(c), 1)
                rec[key + "_us_spread"] = round(max(c) - min(c), 1)
                rec[key + "_loss"] = w["loss"]
            rec["speedup"] = round(rec["unfused_us"] / rec["fused_us"], 2)
            text = json.dumps(rec)
            print(text, flush=True)
            out.write(text + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--box", default=None)
    ap.add_argument("--reference-cpu", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "cartpole_learnt_timing.jsonl"))
    args = ap.parse_args()
    name = box(args)
    if args.fit:
        return time_fit(args, name)
    if args.reference_cpu:
        g = np.load(os.path.join(REPO, "tests", "golden", "cartpole_learnt.npz"))
        for case in ("learnt_balance_a", "learnt_balance_b", "learnt_swingup"):
            print(json.dumps(dict(
                tool="time_cartpole_learnt", box=name, what="reference_cpu_evaluator",
                device="cpu", case=case, flights=int(len(g[case + ".steps"])),
                steps_flown=int(g[case + ".steps"].sum()),
                seconds=round(float(g[case + ".seconds"]), 3))))
        return
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.train_base import TrainBase, momentum_sgd
    from test_cartpole_eval_cpu import golden_net
    from test_gpu_cartpole_learnt import _unroll_loss
    from conftest import load_golden
    dev = torch.device("cuda:0")
    net = golden_net(load_golden("cartpole_closed_loop.npz"), "shipped").to(dev)
    m = fitted(dev)
    gen = torch.Generator().manual_seed(0)

    def line(**kw):
        print(json.dumps(dict(tool="time_cartpole_learnt", box=name, **kw)), flush=True)

    for B in (8, 65536):
        s0 = ((torch.rand(B, 4, generator=gen) * 2 - 1)
              * torch.tensor([1.0, 1.0, 0.3, 1.0])).to(dev)
        frozen = [p.requires_grad for p in m.parameters()]
        for p in m.parameters():
            p.requires_grad_(False)

        def fused():
            net.zero_grad()
            acts = net(s0.clone()).reshape(-1, H, 1)
            F.cartpole_learnt_rollout_loss(m, s0, acts, DT).backward()

        def unrolled():
            net.zero_grad()
            _unroll_loss(m, net, s0, DT).backward()
        uf = timed(fused, args.reps)
        uu = timed(unrolled, args.reps)
        line(what="controller_step", B=B, H=H, fused_us=round(uf[0], 1),
             fused_us_min=round(uf[1], 1), stepwise_us=round(uu[0], 1),
             stepwise_us_min=round(uu[1], 1))
        for p, r in zip(m.parameters(), frozen):
            p.requires_grad_(r)

        import types
        a = (torch.rand(B, 1, generator=gen) * 2 - 1).to(dev)
        seq = a[:, None, :].repeat(1, H, 1)
        mf = fitted(dev)
        tr = types.SimpleNamespace(
            train_dynamics=mf, eval_dynamics=CartpoleDynamics({"masspole": .2, "length": .7}),
            delta_t=DT, l2_lambda=0, results_dict={"loss_dyn_per_step": []},
            optimizer_dynamics=momentum_sgd(mf.parameters(), 1e-9))
        uf = timed(lambda: TrainBase.train_dynamics_model(tr, s0, seq), args.reps)
        line(what="dynamics_fit_step", B=B, us=round(uf[0], 1), us_min=round(uf[1], 1))

    params = CartpoleDynamics().params
    for n in (10, 65536):
        s0 = torch.zeros(n, 4, device=dev)
        ul = timed(lambda: F.cartpole_mlp_closed_loop(net, s0, DT, None, max_steps=T,
                                                      learnt=m), max(args.reps // 5, 5))
        ua = timed(lambda: F.cartpole_mlp_closed_loop(net, s0, DT, params, max_steps=T),
                   max(args.reps // 5, 5))
        line(what="closed_loop_balance", flights=n, max_steps=T,
             learnt_us=round(ul[0], 1), analytic_us=round(ua[0], 1))


if __name__ == "__main__":
    main()
