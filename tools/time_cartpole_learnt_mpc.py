#!/usr/bin/env python
"""Timing of the cart-pole shooting MPC that plans through the learnt simulator
(csrc/cartpole_mpc.hip: cart_mpc_learnt_solve_kernel,
cart_mpc_learnt_closed_loop_kernel), one JSON line per measurement, each naming
the box; printed and appended to `--out`
(profiles/cartpole_learnt_mpc_timing.jsonl):

  solve        one solve at B = 8, 64 and 65 536, H = 10, iters = 10
               (apg_cartpole_learnt_mpc_solve on device-native [..][B] tensors)
               next to, alternating in the same run,
               (a) apg_cartpole_mpc_solve on the nominal parameters: what the
                   residual costs;
               (b) the same solve composed from what the library offered
                   before: iters x (apg_cartpole_learnt_rollout_fwd_bwd for J
                   and dJ/du + the heavy-ball update as torch ops) and one more
                   launch for the final cost.  Its model WRAPS the angle: a
                   timing yardstick only; on near-upright starts (no window
                   crosses +-pi) the two are checked against each other before
                   they are timed (median difference of u, share of
                   trajectories beyond 1e-4: a ReLU kink within float32's
                   reach sends either path along another gradient).
  closed_loop  64 and 65 536 flights x 250 control steps on the learnt plant,
               swing-up mode (no flight stops): the solver on the learnt model
               (apg_cartpole_learnt_mpc_closed_loop) next to the solver on the
               nominal model (apg_cartpole_mpc_closed_loop) on the same plant.
The model is the fitted module of tests/golden/cartpole_learnt.npz.  Device
events around each timed call after 5 untimed calls of each contender; the
contenders alternate call by call; median, minimum and the 10 % / 90 %
quantiles over `--reps` calls (closed loop at 65 536 flights: reps / 10).

    python tools/time_cartpole_learnt_mpc.py [--reps 50] [--box NAME] [--out FILE]
"""
import argparse
import copy
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


def timed(fns, reps):
    """{name: callable} -> {name: dict(median, min, p10, p90) in us}; the
    callables alternate call by call."""
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
    return {k: dict(us=round(float(np.median(v)), 1), us_min=round(float(np.min(v)), 1),
                    us_p10=round(float(np.quantile(v, 0.1)), 1),
                    us_p90=round(float(np.quantile(v, 0.9)), 1)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--box", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "cartpole_learnt_mpc_timing.jsonl"))
    args = ap.parse_args()
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    import cartpole_learnt_mpc_restatement as L
    import cartpole_mpc_restatement as R
    dev = torch.device("cuda:0")
    name = args.box or torch.cuda.get_device_name(0) or platform.machine()
    params = CartpoleDynamics().params
    mod = copy.deepcopy(L.module()).to(dev)
    lib, opt = F.lib(), F.cartpole_mpc_options(ITERS)
    tensors = F._cartpole_learnt_tensors(mod)
    learnt = F._cartpole_learnt_model(tensors)
    beta, alpha = F.CARTPOLE_MPC_DEFAULTS["beta"], F.CARTPOLE_MPC_DEFAULTS["alpha"]

    def line(**kw):
        text = json.dumps(dict(tool="time_cartpole_learnt_mpc", box=name, **kw))
        print(text, flush=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")

    def flat(t):
        return {f"{k}_{q}": v for k, d in t.items() for q, v in d.items()}

    # ---- one solve ---------------------------------------------------------------
    for B in (8, 64, 65536):
        s0 = R.near_upright(B, torch.Generator().manual_seed(1)).float().to(dev)
        s_soa = s0.t().contiguous()
        u_dev = torch.empty(H, B, device=dev)
        cost = torch.empty(B, device=dev)
        stream = F.stream_of(s_soa)
        out = {}

        def fused():
            F.check(lib.apg_cartpole_learnt_mpc_solve(
                s_soa.data_ptr(), None, DT, ctypes.byref(learnt), ctypes.byref(opt), B, H,
                u_dev.data_ptr(), cost.data_ptr(), None, stream),
                "apg_cartpole_learnt_mpc_solve")

        def nominal():
            F.check(lib.apg_cartpole_mpc_solve(
                s_soa.data_ptr(), None, DT, ctypes.byref(params), ctypes.byref(opt), B, H,
                u_dev.data_ptr(), cost.data_ptr(), None, stream), "apg_cartpole_mpc_solve")

        def composed():
            u = torch.zeros(H, 1, B, device=dev)
            m = torch.zeros_like(u)
            for _ in range(ITERS):
                res = F.cartpole_learnt_rollout_fwd_bwd(
                    mod, s_soa, u, DT, layout="soa", want_grad_state0=False, want_loss=False,
                    out=out)
                out.update(loss_partials=res["loss_partials"],
                           grad_actions=res["grad_actions"])
                m = beta * m + alpha * res["grad_actions"]
                u = (u - m).clamp_(-1.0, 1.0)
            F.cartpole_learnt_rollout_fwd_bwd(mod, s_soa, u, DT, layout="soa",
                                              want_grad_state0=False, want_loss=False, out=out)
            return u

        fused()
        # (a trajectory that passes a ReLU kink of the residual within float32's
        # reach may descend along another gradient in either path: the check is
        # on the median and on the share beyond 1e-4, not on the maximum)
        per = (u_dev[:, None, :] - composed()).abs().amax((0, 1))
        diff, beyond = float(per.median()), float((per > 1e-4).float().mean())
        assert diff < 1e-6 and beyond < 0.01, (diff, beyond)
        t = timed(dict(fused=fused, nominal=nominal, composed=composed), args.reps)
        line(what="solve", B=B, H=H, iters=ITERS, **flat(t),
             fused_over_nominal=round(t["fused"]["us"] / t["nominal"]["us"], 3),
             fused_over_composed=round(t["fused"]["us"] / t["composed"]["us"], 4),
             median_abs_u_difference=diff, share_beyond_1e_4=beyond)

    # ---- the closed loop on the learnt plant -----------------------------------------
    for n in (64, 65536):
        starts = R.swingup(n, torch.Generator().manual_seed(2)).float().to(dev)
        kw = dict(learnt=mod, max_steps=T, mode="swingup", burn_in=100, iters=ITERS)
        fly = dict(
            learnt_model=lambda: F.cartpole_mpc_closed_loop(starts, DT, None, model_learnt=mod,
                                                            **kw),
            nominal_model=lambda: F.cartpole_mpc_closed_loop(starts, DT, None,
                                                             model_params=params, **kw))
        t = timed(fly, max(args.reps // 10, 3) if n > 64 else args.reps)
        up = {k: round(float(fn()["upright"].float().mean()), 4) for k, fn in fly.items()}
        line(what="closed_loop", flights=n, max_steps=T, mode="swingup", iters=ITERS,
             plant="learnt", **flat(t),
             learnt_over_nominal=round(t["learnt_model"]["us"] / t["nominal_model"]["us"], 3),
             learnt_model_steps_per_s=round(n * T / t["learnt_model"]["us"] * 1e6),
             learnt_model_upright=up["learnt_model"], nominal_model_upright=up["nominal_model"])


if __name__ == "__main__":
    main()
