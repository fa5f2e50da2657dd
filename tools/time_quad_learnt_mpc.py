#!/usr/bin/env python
"""Timing of the shooting MPC that plans through the learnt simulator
(csrc/quad_mpc.hip: apg_quad_learnt_mpc_solve, apg_quad_learnt_mpc_closed_loop),
one JSON line per measurement, each naming the box; printed and appended to
`--out` (profiles/quad_learnt_mpc_timing.jsonl):

  solve        one solve of B = 65 536 trajectories, iters = 10, H = 10 (pack +
               one launch, the iterations inside it) against the same job
               composed from what the library offered before: iters x (the
               fused learnt rollout apg_quad_learnt_rollout_fwd_bwd for J and
               dJ/du + the heavy-ball update as torch ops) and one more launch
               for the final cost, on the same device tensors.  The two are
               checked against each other before they are timed.
  closed_loop  65 536 flights x 251 control steps, the plant the fitted
               simulator of tests/golden/closed_loop_learnt.npz: once with the
               solver planning on the nominal model (apg_quad_mpc_closed_loop)
               and once planning on the plant's own module
               (apg_quad_learnt_mpc_closed_loop) - both times and both mean
               divergences.
Device events around each timed call, median over `--reps` (closed loop:
reps / 5), after 5 untimed calls.

    python tools/time_quad_learnt_mpc.py [--reps 50] [--box NAME] [--out FILE]
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

DT, H, T, ITERS = 0.1, 10, 251, 10


def timed(fn, reps, warm=5):
    for _ in range(warm):
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
                    default=os.path.join(REPO, "profiles", "quad_learnt_mpc_timing.jsonl"))
    args = ap.parse_args()
    from apg_trajectory_tracking_amd import functional as F, synthetic
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    import quad_learnt_mpc_restatement as L
    from quad_mpc_restatement import experiment_windows
    dev = torch.device("cuda:0")
    name = args.box or torch.cuda.get_device_name(0) or platform.machine()
    B = args.batch
    dyn = L.module("loop", dev)

    def line(**kw):
        text = json.dumps(dict(tool="time_quad_learnt_mpc", box=name, **kw))
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

    def rollout(u):
        res = F.quad_learnt_rollout_fwd_bwd(dyn, s_soa, u, r_soa, DT, layout="soa",
                                            want_grad_state0=False, out=out)
        out.update({k: v for k, v in res.items() if v is not None})
        return res

    def composed():
        u = torch.full((H, 4, B), 0.5, device=dev)
        m = torch.zeros_like(u)
        for _ in range(ITERS):
            m = beta * m + alpha * rollout(u)["grad_actions"]
            u = (u - m).clamp_(0.0, 1.0)
        rollout(u)
        return u

    fused = lambda: F.quad_mpc_solve(s0, ref, DT, dyn.params, iters=ITERS, learnt=dyn)
    diff = (fused()["u"].permute(1, 2, 0) - composed()).abs().amax((0, 1))
    # (a ReLU kink taken the other way sends a trajectory elsewhere: the median
    # says whether the two are the same job, the maximum is reported)
    assert float(diff.median()) < 1e-5, float(diff.median())
    lib, opt, w = F.lib(), F.quad_mpc_options(ITERS), F.quad_loss_weights()
    model = F._learnt_model(dyn)
    u_dev = torch.empty(H, 4, B, device=dev)
    cost = torch.empty(B, device=dev)
    ws = torch.empty(lib.apg_quad_learnt_mpc_workspace_floats(), device=dev)

    def fused_native():
        u_dev.fill_(0.5)
        F.check(lib.apg_quad_learnt_mpc_solve(
            s_soa.data_ptr(), r_soa.data_ptr(), 9, DT, ctypes.byref(dyn.params),
            ctypes.byref(model), ctypes.byref(w), ctypes.byref(opt), B, H, u_dev.data_ptr(),
            cost.data_ptr(), None, ws.data_ptr(), F.stream_of(s_soa)),
            "apg_quad_learnt_mpc_solve")
    tf, tn, tc = timed(fused, args.reps), timed(fused_native, args.reps), timed(composed, args.reps)
    line(what="solve", B=B, H=H, iters=ITERS, fused_us=round(tf[0], 1),
         fused_us_min=round(tf[1], 1), fused_soa_us=round(tn[0], 1),
         fused_soa_us_min=round(tn[1], 1), composed_us=round(tc[0], 1),
         composed_us_min=round(tc[1], 1), fused_over_composed=round(tn[0] / tc[0], 4),
         median_abs_u_difference=float(diff.median()), max_abs_u_difference=float(diff.max()))

    # ---- (b) closed loop on the learnt plant: nominal model, learnt model --------
    traj = synthetic.quad_eval_trajectories(B, 501, DT, seed=42)
    traj[:, :, 2] += 3
    traj = traj.to(dev)
    kw = dict(learnt=dyn, iters=ITERS, max_steps=T, thresh_div=3.0, thresh_stable=1.0)
    nominal_params = FlightmareDynamics().params
    nominal = lambda: F.quad_mpc_closed_loop(traj, DT, dyn.params, model_params=nominal_params,
                                             **kw)
    learnt = lambda: F.quad_mpc_closed_loop(traj, DT, dyn.params, model_learnt=dyn, **kw)
    reps = max(args.reps // 5, 5)
    tn_, tl = timed(nominal, reps), timed(learnt, reps)
    rn, rl = nominal(), learnt()
    line(what="closed_loop", flights=B, max_steps=T, iters=ITERS,
         plant="closed_loop_learnt.npz",
         nominal_model_us=round(tn_[0], 1), nominal_model_us_min=round(tn_[1], 1),
         learnt_model_us=round(tl[0], 1), learnt_model_us_min=round(tl[1], 1),
         learnt_over_nominal=round(tl[0] / tn_[0], 2),
         learnt_model_steps_per_s=round(B * T / tl[0] * 1e6),
         nominal_model_mean_divergence_m=round(float(rn["div"].mean()), 4),
         learnt_model_mean_divergence_m=round(float(rl["div"].mean()), 4))


if __name__ == "__main__":
    main()
