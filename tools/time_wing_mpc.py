#!/usr/bin/env python
"""Timing of the batched fixed-wing shooting MPC (csrc/wing_mpc.hip), one JSON
line per measurement, each naming the box; printed and appended to `--out`
(profiles/wing_mpc_timing.jsonl):

  solve        one solve at B = 8, 64 and 65 536, iters = 10, H = 10
               (apg_wing_mpc_solve on device-native tensors: one launch, the
               iterations inside the kernel) next to the same job composed from
               what the library offered before: iters x (the fused rollout launch
               apg_wing_rollout_fwd_bwd for J and dJ/du + the heavy-ball update
               as torch ops) and one more launch for the final cost, on the same
               device tensors.  The composed path steps the rollout kernel's
               model (hardware sin / cos): the two are checked against each
               other before they are timed.
  closed_loop  64 and 65 536 flights x 100 control steps with the solver in the
               loop (apg_wing_mpc_closed_loop, iters = 10) next to the shipped
               network controller on the same targets
               (apg_wing_mlp_closed_loop), and the mean target error of both.
               Per control step the solver does 11 forward and 10 reverse sweeps
               of 10 model steps where the policy does one network evaluation.
Device events around each timed call, the contenders alternating call by call,
median over `--reps` (closed loop: reps / 5) with the minimum and the 10 % and
90 % quantiles, after 5 untimed calls of each.

    python tools/time_wing_mpc.py [--reps 50] [--box NAME] [--out FILE]
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

DT, H, T, ITERS = 0.05, 10, 100, 10


def timed_alternating(fns, reps):
    """{name: (median, min, q10, q90)} in microseconds; one call of each
    contender per round, in turn"""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return {k: tuple(round(float(x), 1) for x in (
        np.median(v), np.min(v), np.quantile(v, 0.1), np.quantile(v, 0.9)))
        for k, v in times.items()}


def stats(prefix, t):
    return {f"{prefix}_us": t[0], f"{prefix}_us_min": t[1], f"{prefix}_us_q10": t[2],
            f"{prefix}_us_q90": t[3]}


def mean_target_error(out, max_steps, thresh_div):
    """FixedWingEvaluator.run_eval's statistic from a closed-loop dict"""
    steps = out["steps"].to(torch.int64)
    ev = torch.stack((out["div_pass"], out["div_fail"]), 2).double()
    flown = torch.arange(ev.shape[0], device=ev.device)[:, None] < steps[None]
    valid = (ev >= 0) & flown[:, :, None]
    total = torch.where(valid, ev, torch.zeros_like(ev)).sum((0, 2))
    cut = steps == max_steps
    return float(((total + cut * thresh_div) / (valid.sum((0, 2)) + cut)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--box", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wing_mpc_timing.jsonl"))
    args = ap.parse_args()
    from apg_trajectory_tracking_amd import functional as F, synthetic
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    import wing_flight_cases
    from conftest import wing_loop_policy
    dev = torch.device("cuda:0")
    name = args.box or torch.cuda.get_device_name(0) or platform.machine()
    params = FixedWingDynamics().params
    beta, alpha = F.WING_MPC_DEFAULTS["beta"], F.WING_MPC_DEFAULTS["alpha_thrust"]

    def line(**kw):
        text = json.dumps(dict(tool="time_wing_mpc", box=name, **kw))
        print(text, flush=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")

    # ---- (a) one solve next to the composed path ------------------------------
    lib, opt, w = F.lib(), F.wing_mpc_options(ITERS), F.wing_loss_weights()
    for B in (8, 64, 65536):
        d = synthetic.wing_batch(B, H, DT, seed=3)
        s_soa = d["state0"].t().contiguous().to(dev)
        r_soa = d["ref"].permute(1, 2, 0).contiguous().to(dev)
        start = torch.tensor(F.WING_MPC_START, device=dev)[None, :, None].expand(H, 4, B)
        out = {}

        def composed():
            u = start.contiguous()
            m = torch.zeros_like(u)
            for _ in range(ITERS):
                res = F.wing_rollout_fwd_bwd(s_soa, u, r_soa, DT, params, layout="soa",
                                             want_grad_state0=False, want_loss=False, out=out)
                out.update(loss_partials=res["loss_partials"], grad_actions=res["grad_actions"])
                m = beta * m + alpha * res["grad_actions"]
                u = (u - m).clamp_(0.0, 1.0)
            F.wing_rollout_fwd_bwd(s_soa, u, r_soa, DT, params, layout="soa",
                                   want_grad_state0=False, want_loss=False, out=out)
            return u

        u_dev, cost = torch.empty(H, 4, B, device=dev), torch.empty(B, device=dev)

        def fused():
            u_dev.copy_(start)
            F.check(lib.apg_wing_mpc_solve(
                s_soa.data_ptr(), r_soa.data_ptr(), DT, ctypes.byref(params), ctypes.byref(w),
                ctypes.byref(opt), B, H, u_dev.data_ptr(), cost.data_ptr(), None,
                F.stream_of(s_soa)), "apg_wing_mpc_solve")
            return u_dev

        diff = float((fused() - composed()).abs().max())
        assert diff < 1e-3, diff
        t = timed_alternating(dict(fused=fused, composed=composed), args.reps)
        line(what="solve", B=B, H=H, iters=ITERS, **stats("fused", t["fused"]),
             **stats("composed", t["composed"]),
             fused_over_composed=round(t["fused"][0] / t["composed"][0], 4),
             max_abs_u_difference=diff)

    # ---- (b) closed loop next to the shipped network controller -----------------
    net = wing_loop_policy(dev)
    data = wing_flight_cases.data()
    mean, std = data["mean"].tolist(), data["std"].tolist()
    reps = max(args.reps // 5, 5)
    for n in (64, 65536):
        g = torch.Generator().manual_seed(2)
        targets = torch.cat((torch.full((n, 1, 1), 50.0),
                             (torch.rand(n, 1, 2, generator=g) - .5) * 10), 2).to(dev)
        mpc = lambda: F.wing_mpc_closed_loop(targets, DT, params, max_steps=T, iters=ITERS)
        pol = lambda: F.wing_mlp_closed_loop(net, targets, DT, params, mean, std, max_steps=T)
        t = timed_alternating(dict(mpc=mpc, policy=pol), reps)
        line(what="closed_loop", flights=n, max_steps=T, iters=ITERS, **stats("mpc", t["mpc"]),
             **stats("policy", t["policy"]),
             mpc_steps_per_s=round(n * T / t["mpc"][0] * 1e6),
             policy_steps_per_s=round(n * T / t["policy"][0] * 1e6),
             mpc_over_policy=round(t["mpc"][0] / t["policy"][0], 2),
             mpc_mean_target_error=round(mean_target_error(mpc(), T, 10.0), 4),
             policy_mean_target_error=round(mean_target_error(pol(), T, 10.0), 4))


if __name__ == "__main__":
    main()
