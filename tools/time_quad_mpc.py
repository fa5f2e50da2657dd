#!/usr/bin/env python
"""Timing of the batched shooting MPC (csrc/quad_mpc.hip), one JSON line per
measurement, each naming the box; printed and appended to `--out`
(profiles/quad_mpc_timing.jsonl):

  solve        one solve of B = 65 536 trajectories, iters = 10, H = 10
               (apg_quad_mpc_solve: one launch, the iterations in registers)
               against the same job composed from what the library offered
               before: iters x (the fused rollout launch apg_quad_rollout_fwd_bwd
               for J and dJ/du + the heavy-ball update as torch ops) and one
               more launch for the final cost, on the same device tensors.  The
               two are checked against each other before they are timed.
  closed_loop  65 536 flights x 251 control steps with the solver in the loop
               (apg_quad_mpc_closed_loop, iters = 10) next to the shipped
               network controller on the same trajectories
               (apg_quad_mlp_closed_loop): closed-loop steps per second of both
               and their ratio.  Per control step the solver does 11 forward
               and 10 reverse sweeps of 10 model steps where the policy does
               one network evaluation.
Device events around each timed call, median over `--reps` (closed loop:
reps / 5), after 5 untimed calls.

    python tools/time_quad_mpc.py [--reps 50] [--box NAME] [--out FILE]
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

DT, H, T, ITERS = 0.1, 10, 251, 10


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "quad_mpc_timing.jsonl"))
    args = ap.parse_args()
    from apg_trajectory_tracking_amd import functional as F, synthetic
    from apg_trajectory_tracking_amd.checkpoint import build_policy
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    from conftest import load_golden
    from quad_mpc_restatement import experiment_windows
    dev = torch.device("cuda:0")
    name = args.box or torch.cuda.get_device_name(0) or platform.machine()
    B = args.batch
    params = FlightmareDynamics().params

    def line(**kw):
        text = json.dumps(dict(tool="time_quad_mpc", box=name, **kw))
        print(text, flush=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")

    # ---- (a) one solve against the composed path -----------------------------
    s0, ref = experiment_windows(B=B)
    s0, ref = s0.to(dev), ref.to(dev)
    s_soa, r_soa = s0.t().contiguous(), ref.permute(1, 2, 0).contiguous()
    alpha = torch.tensor(
        [F.MPC_DEFAULTS["alpha_thrust"]] + [F.MPC_DEFAULTS["alpha_rate"]] * 3,
        device=dev)[None, :, None]
    beta = F.MPC_DEFAULTS["beta"]
    out = {}

    def composed():
        u = torch.full((H, 4, B), 0.5, device=dev)
        m = torch.zeros_like(u)
        for _ in range(ITERS):
            res = F.quad_rollout_fwd_bwd(s_soa, u, r_soa, DT, params, layout="soa",
                                         want_grad_state0=False, want_loss=False, out=out)
            out.update(loss_partials=res["loss_partials"], grad_actions=res["grad_actions"])
            m = beta * m + alpha * res["grad_actions"]
            u = (u - m).clamp_(0.0, 1.0)
        F.quad_rollout_fwd_bwd(s_soa, u, r_soa, DT, params, layout="soa",
                               want_grad_state0=False, want_loss=False, out=out)
        return u

    fused = lambda: F.quad_mpc_solve(s0, ref, DT, params, iters=ITERS)
    diff = float((fused()["u"].permute(1, 2, 0) - composed()).abs().max())
    assert diff < 1e-4, diff
    # the fused call's host side permutes [B, ...] tensors in and out; time the
    # launch on the device-native tensors as well
    lib, opt, w = F.lib(), F.quad_mpc_options(ITERS), F.quad_loss_weights()
    import ctypes
    u_dev = torch.empty(H, 4, B, device=dev)
    cost = torch.empty(B, device=dev)

    def fused_native():
        u_dev.fill_(0.5)
        F.check(lib.apg_quad_mpc_solve(
            s_soa.data_ptr(), r_soa.data_ptr(), 9, DT, ctypes.byref(params), ctypes.byref(w),
            ctypes.byref(opt), B, H, u_dev.data_ptr(), cost.data_ptr(), None,
            F.stream_of(s_soa)), "apg_quad_mpc_solve")
    tf, tn, tc = timed(fused, args.reps), timed(fused_native, args.reps), timed(composed, args.reps)
    line(what="solve", B=B, H=H, iters=ITERS, fused_us=round(tf[0], 1),
         fused_us_min=round(tf[1], 1), fused_soa_us=round(tn[0], 1),
         fused_soa_us_min=round(tn[1], 1), composed_us=round(tc[0], 1),
         composed_us_min=round(tc[1], 1), fused_over_composed=round(tn[0] / tc[0], 4),
         max_abs_u_difference=diff)

    # ---- (b) closed loop next to the shipped network controller -----------------
    ck = load_golden("checkpoints.npz")
    net = build_policy("quad", {k[len("quad.w."):]: torch.from_numpy(ck[k])
                                for k in ck.files if k.startswith("quad.w.")}).to(dev)
    traj = synthetic.quad_eval_trajectories(B, 501, DT, seed=42)
    traj[:, :, 2] += 3
    traj = traj.to(dev)
    kw = dict(max_steps=T, thresh_div=3.0, thresh_stable=1.0)
    reps = max(args.reps // 5, 5)
    tm = timed(lambda: F.quad_mpc_closed_loop(traj, DT, params, iters=ITERS, **kw), reps)
    tp = timed(lambda: F.quad_mlp_closed_loop(net, traj, DT, params, **kw), reps)
    res = F.quad_mpc_closed_loop(traj, DT, params, iters=ITERS, **kw)
    pol = F.quad_mlp_closed_loop(net, traj, DT, params, **kw)
    line(what="closed_loop", flights=B, max_steps=T, iters=ITERS, mpc_us=round(tm[0], 1),
         mpc_us_min=round(tm[1], 1), policy_us=round(tp[0], 1), policy_us_min=round(tp[1], 1),
         mpc_steps_per_s=round(B * T / tm[0] * 1e6), policy_steps_per_s=round(B * T / tp[0] * 1e6),
         mpc_over_policy=round(tm[0] / tp[0], 2),
         mpc_mean_divergence_m=round(float(res["div"].mean()), 4),
         policy_mean_divergence_m=round(float(pol["div"].mean()), 4))


if __name__ == "__main__":
    main()
