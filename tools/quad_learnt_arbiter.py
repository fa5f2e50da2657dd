"""The device / float32-oracle / float64-oracle figures of the fused rollout
through the learnt quadrotor simulator (apg_quad_learnt_rollout_fwd_bwd), one
JSON line per case of tests/test_gpu_quad_learnt_rollout.py's arbiter test: the
statistics conftest.assert_no_worse_than_fp32 returns for the states (all
trajectories), dL/dactions and dL/dstate0 (trajectories off a ReLU kink), the
number of trajectories set aside, and the loss errors.  Cases, inputs and the
kink rule are those of tests/quad_loss_cases.py.  A comparison that misses the
arbiter's factors is recorded with "missed": true, not dropped.

    python tools/quad_learnt_arbiter.py profiles/quad_learnt_arbiter.jsonl
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import test_gpu_quad_learnt_rollout as T                          # noqa: E402
from conftest import assert_no_worse_than_fp32                     # noqa: E402


def arbiter(dev, f32, f64, what):
    try:
        stats, missed = assert_no_worse_than_fp32(dev, f32, f64, what), False
    except AssertionError as e:
        stats, missed = dict(e.args[0]), True
    out = {k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in stats.items()
           if k != "what"}
    out["tail_ratio"] = round(stats["tail_mean_dev"] / stats["tail_mean_f32"], 3)
    out["worst_ratio"] = round(stats["worst_dev"] / stats["worst_f32"], 3)
    out["missed"] = missed
    return out


def main(path):
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rows = []
    for which, H, layout, ref_cols in T.ARBITER:
        got, f32, f64, keep, tag = T.measure(dev, which, H, layout, ref_cols)
        row = dict(case=tag, weights=which, H=H, layout=layout, ref_cols=ref_cols,
                   batch=int(len(keep)), set_aside=int((~keep).sum()),
                   loss_err=float("%.3g" % (abs(got["loss"] - f64["loss"]) / f64["loss"])),
                   partials_err=float("%.3g" % (np.abs(got["partials"] - f64["partials"])
                                                / f64["partials"]).max()))
        row["states"] = arbiter(got["states"], f32["states"], f64["states"], tag + " states")
        for k in ("grad_actions", "grad_state0"):
            row[k] = arbiter(got[k][keep], f32[k][keep], f64[k][keep], f"{tag} {k}")
        rows.append(row)
    with open(path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    missed = [r["case"] for r in rows
              if any(r[k]["missed"] for k in ("states", "grad_actions", "grad_state0"))]
    print("%d lines -> %s; missed the arbiter: %s" % (len(rows), path, missed))


if __name__ == "__main__":
    main(sys.argv[1])
