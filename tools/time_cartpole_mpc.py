#!/usr/bin/env python
"""Timing of the batched cart-pole shooting MPC (csrc/cartpole_mpc.hip), one
JSON line per measurement, each naming the box; printed and appended to `--out`
(profiles/cartpole_mpc_timing.jsonl):

  solve        one solve of B = 65 536 trajectories, iters = 10, H = 10
               (apg_cartpole_mpc_solve: one launch, the iterations in registers)
               next to the same job composed from what the library offered
               before: iters x (the fused rollout launch
               apg_cartpole_rollout_fwd_bwd for J and dJ/du + the heavy-ball
               update as torch ops) and one more launch for the final cost, on
               the same device tensors.  The composed path steps the WRAPPED
               model, so it is a timing comparator only; on near-upright starts
               (no window crosses +-pi) the two are checked against each other
               before they are timed.
  closed_loop  10 and 65 536 episodes x 250 control steps with the solver in
               the loop (apg_cartpole_mpc_closed_loop, iters = 10, swing-up mode:
               no episode stops) next to the shipped network controller on the
               same starts (apg_cartpole_mlp_closed_loop).  Per control step the
               solver does 11 forward and 10 reverse sweeps of 10 model steps
               where the policy does one network evaluation.
Device events around each timed call, median over `--reps` (closed loop:
reps / 5), after 5 untimed calls.

    python tools/time_cartpole_mpc.py [--reps 50] [--box NAME] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import platform
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

DT, H, T, ITERS = 0.05, 10, 250, 10


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--box", default=None)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--out",
                    default=os.path.join(REPO, "profiles", "cartpole_mpc_timing.jsonl"))
    args = ap.parse_args()
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    import cartpole_mpc_restatement as R
    from test_cartpole_eval_cpu import golden_net
    dev = torch.device("cuda:0")
    name = args.box or torch.cuda.get_device_name(0) or platform.machine()
    B = args.batch
    params = CartpoleDynamics().params

    def line(**kw):
        text = json.dumps(dict(tool="time_cartpole_mpc", box=name, **kw))
        print(text, flush=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")

    # ---- (a) one solve next to the composed path ------------------------------
    s0 = R.near_upright(B, torch.Generator().manual_seed(1)).float().to(dev)
    s_soa = s0.t().contiguous()
    beta, alpha = F.CARTPOLE_MPC_DEFAULTS["beta"], F.CARTPOLE_MPC_DEFAULTS["alpha"]
    out = {}

    def composed():
        u = torch.zeros(H, 1, B, device=dev)
        m = torch.zeros_like(u)
        for _ in range(ITERS):
            res = F.cartpole_rollout_fwd_bwd(s_soa, u, DT, params, layout="soa",
                                             want_grad_state0=False, want_loss=False, out=out)
            out.update(loss_partials=res["loss_partials"], grad_actions=res["grad_actions"])
            m = beta * m + alpha * res["grad_actions"]
            u = (u - m).clamp_(-1.0, 1.0)
        F.cartpole_rollout_fwd_bwd(s_soa, u, DT, params, layout="soa",
                                   want_grad_state0=False, want_loss=False, out=out)
        return u

    fused = lambda: F.cartpole_mpc_solve(s0, DT, params, iters=ITERS)
    diff = float((fused()["u"].permute(1, 2, 0) - composed()).abs().max())
    assert diff < 1e-4, diff
    # the fused call's host side transposes [B, ...] tensors in and out; time the
    # launch on the device-native tensors as well
    lib, opt = F.lib(), F.cartpole_mpc_options(ITERS)
    u_dev = torch.empty(H, B, device=dev)
    cost = torch.empty(B, device=dev)

    def fused_native():
        F.check(lib.apg_cartpole_mpc_solve(
            s_soa.data_ptr(), None, DT, ctypes.byref(params), ctypes.byref(opt), B, H,
            u_dev.data_ptr(), cost.data_ptr(), None, F.stream_of(s_soa)),
            "apg_cartpole_mpc_solve")
    tf, tn, tc = timed(fused, args.reps), timed(fused_native, args.reps), timed(composed, args.reps)
    line(what="solve", B=B, H=H, iters=ITERS, fused_us=round(tf[0], 1),
         fused_us_min=round(tf[1], 1), fused_soa_us=round(tn[0], 1),
         fused_soa_us_min=round(tn[1], 1), composed_us=round(tc[0], 1),
         composed_us_min=round(tc[1], 1), fused_over_composed=round(tn[0] / tc[0], 4),
         max_abs_u_difference=diff)

    # ---- (b) closed loop next to the shipped network controller -----------------
    net = golden_net(None, "shipped").to(dev)
    reps = max(args.reps // 5, 5)
    for n in (10, B):
        starts = R.swingup(n, torch.Generator().manual_seed(2)).float().to(dev)
        kw = dict(max_steps=T, mode="swingup", burn_in=100)
        tm = timed(lambda: F.cartpole_mpc_closed_loop(starts, DT, params, iters=ITERS, **kw),
                   reps)
        tp = timed(lambda: F.cartpole_mlp_closed_loop(net, starts, DT, params, **kw), reps)
        res = F.cartpole_mpc_closed_loop(starts, DT, params, iters=ITERS, **kw)
        pol = F.cartpole_mlp_closed_loop(net, starts, DT, params, **kw)
        line(what="closed_loop", flights=n, max_steps=T, mode="swingup", iters=ITERS,
             mpc_us=round(tm[0], 1), mpc_us_min=round(tm[1], 1), policy_us=round(tp[0], 1),
             policy_us_min=round(tp[1], 1), mpc_steps_per_s=round(n * T / tm[0] * 1e6),
             policy_steps_per_s=round(n * T / tp[0] * 1e6),
             mpc_over_policy=round(tm[0] / tp[0], 2),
             mpc_upright=round(float(res["upright"].float().mean()), 4),
             policy_upright=round(float(pol["upright"].float().mean()), 4))


if __name__ == "__main__":
    main()
