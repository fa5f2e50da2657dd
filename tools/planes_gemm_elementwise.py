"""Worst element-wise error |C - ref64| / (|A| @ |B|^T) of every block shape of
csrc/planes_gemm.hip, per operand family, next to the bound
tests/test_gpu_planes_gemm_shapes.py holds it to: the cases, operands and
bounds are those of tests/planes_gemm_cases.py.  One JSON line per (kernel,
block shape, family, launch path); errors and bounds in units of 2^-24.

    python tools/planes_gemm_elementwise.py profiles/planes_gemm_elementwise.jsonl
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import planes_gemm_cases as pc                                    # noqa: E402
from apg_trajectory_tracking_amd import _capi, functional as F    # noqa: E402


def main(path):
    dev = torch.device("cuda:0")
    rows = {}

    def note(key, c, N, wgs, R, bound, err):
        r = rows.setdefault(key, dict(
            kernel=key[0], MB=key[1], NB=key[2], family=key[3], path=key[4], N=N,
            workgroups=wgs, R=R, bound_u=bound / pc.U, worst_u=0.0, worst_case=None, cases=0))
        r["cases"] += 1
        r["R"], r["bound_u"] = max(r["R"], R), max(r["bound_u"], bound / pc.U)
        if float(err.max()) >= r["worst_u"] * pc.U:
            r["worst_u"], r["worst_case"] = round(float(err.max()) / pc.U, 3), c.name

    cases = pc.accepted_cases()
    for family in ("aligned", "decades"):
        for c in cases:
            kind = pc.kind_of(c)
            N, wgs = pc.PLAN[family, kind[0]]
            err, _ = pc.run_case(F, dev, c, family, N, wgs)
            w = wgs or pc.default_wgs(_capi.lib(), c)
            bound, R = pc.bound_of(c, family, N, w)
            note(kind + (family, "single"), c, N, w, R, bound, err)
        # the grouped stream launch, by the calls of the GPU test
        for call in pc.grouped_calls(cases):
            ops = [pc.operands(c, family, 100, seed=50 + i) for i, c in enumerate(call)]
            ps = [pc.problem(F, dev, c, *o) for c, o in zip(call, ops)]
            F.planes_gemm_multi([p["kw"] for p in ps])
            for c, (A, Bp), p in zip(call, ops, ps):
                err = pc.elementwise_err(pc.result(c, p), *pc.reference(c, A, Bp))
                err = np.where(np.isfinite(err), err, np.inf)
                bound, R = pc.bound_of(c, family, 100, 1)
                note(pc.kind_of(c) + (family, "grouped"), c, 100, None, R, bound, err)
    with open(path, "w") as f:
        for key in sorted(rows, key=str):
            f.write(json.dumps(rows[key]) + "\n")
    over = [r for r in rows.values() if not r["worst_u"] <= r["bound_u"]]
    print("%d lines -> %s; over their bound: %d" % (len(rows), path, len(over)))
    for r in over:
        print("OVER", r)


if __name__ == "__main__":
    main(sys.argv[1])
