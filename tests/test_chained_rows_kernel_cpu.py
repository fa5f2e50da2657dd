"""The chained instantiation of quad_rollout_rows_kernel (csrc/quad.hip,
`CHAINED` = the launches of a two-lane chain) as the compiler reports it, and a
dry check of the GPU test's tolerance: no GPU needed."""
import json
import re

import pytest

import chained_rows_cases as cc
from conftest import rel_err

# The chained instantiation ships with its own store timing only; stashing the
# attitude angles (two waves per SIMD) did not ship, so one wave per SIMD is
# what it has to have (profiles/ab_chained_rows_kernel.txt)
CHAINED_OCCUPANCY = 1


def _rows_kernels():
    from apg_trajectory_tracking_amd import build
    build.build()
    with open(build.RESOURCES) as f:
        res = json.load(f)
    out = {}
    for k, v in res.items():
        m = re.search(r"quad_rollout_rows_kernelILi(\d+)ELb([01])ELb([01])E", k)
        if m:
            key = (int(m.group(1)), m.group(2) == "1", m.group(3) == "1")
            assert key not in out, k
            out[key] = v
    return out


def test_chained_and_serial_instantiations_are_built_at_their_register_budgets():
    rows = _rows_kernels()
    assert sorted(rows) == sorted((H, so, ch) for H in (5, 10) for so in (False, True)
                                  for ch in (False, True)), sorted(rows)
    for (H, so, chained), v in rows.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (H, so, chained, v)
        if chained:
            assert v["occupancy"] >= CHAINED_OCCUPANCY, (H, so, v)
            assert v["vgprs"] + v["agprs"] <= 512 // CHAINED_OCCUPANCY, (H, so, v)
    # the serial instantiations are the parent's: same registers, one wave per
    # SIMD at H = 10, two at H = 5
    serial = {k[:2]: (v["vgprs"], v["agprs"], v["occupancy"])
              for k, v in rows.items() if not k[2]}
    assert serial == {(10, False): (256, 29, 1), (10, True): (256, 30, 1),
                      (5, False): (179, 0, 2), (5, True): (181, 0, 2)}, serial


@pytest.mark.parametrize("kind,B,H", cc.cases(),
                         ids=[f"{k}-B{B}-H{H}" for k, B, H in cc.cases()])
def test_gpu_test_tolerance_holds_for_the_float32_oracle_itself(kind, B, H):
    """tests/test_gpu_chained_rows_kernel.py holds the kernel to 1e-4 of the
    tensor scale against the float64 oracle on these inputs.  The reference's
    own float32 arithmetic meets that bound on every one of them, so the bound
    asks nothing of the kernel that float32 cannot give."""
    for plan in range(cc.NPLANS):
        w64, w32 = cc.oracle64(kind, B, H, plan), cc.oracle32(kind, B, H, plan)
        errs = {k: rel_err(w32[k], w64[k]) for k in ("states", "grad_actions", "grad_state0")}
        errs["loss"] = abs(w32["loss"] - w64["loss"]) / abs(w64["loss"])
        print(kind, B, H, plan, errs)
        assert max(errs.values()) < cc.TOL, errs
