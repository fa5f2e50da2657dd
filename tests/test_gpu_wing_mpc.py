"""The batched fixed-wing shooting MPC on the MI355X (apg_wing_mpc_solve,
apg_wing_mpc_closed_loop through functional / controllers.MPC /
evaluate_fixed_wing.FixedWingEvaluator) under the same float64 arbiter as the
host twins (tests/test_wing_mpc_cpu.py, tests/wing_mpc_restatement.py).  kernel
== twin is NOT demanded bit for bit (the device compiler contracts and orders
operations in its own way): both stand under the same arbiter.  Every test
launches once; none repeats a failing launch."""
import numpy as np
import pytest
import torch

import wing_flight_cases
import wing_mpc_restatement as R
from conftest import wing_loop_policy
from test_wing_mpc_cpu import (ITERS, check_evaluator, check_loop, check_mismatch_differs,
                               check_mpc_object, check_solve, check_u0_semantics)

pytestmark = pytest.mark.gpu
DT = R.DT
F64, F32 = torch.float64, torch.float32
N = R.to_numpy


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def nominal():
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    return FixedWingDynamics().params


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("B", [1, 64, 65, 200])
def test_solve_kernel_under_the_fp64_arbiter(dev, B, iters):
    """The first B starts of the twin's solve case: a lone lane, a full wave, a
    ragged second workgroup, several workgroups with a ragged tail (at B = 200
    the harder half is in).  One restated run of 20 iterations per dtype serves
    every case: a trajectory's solve does not depend on the batch around it."""
    from apg_trajectory_tracking_amd import functional as F
    s0, ref, f64 = R.solve_case(F64)
    _, _, f32 = R.solve_case(F32)
    cut = lambda r: dict(u=r["u"][:B], cost=r["cost"][:B], trace=r["trace"][:, :B])
    got = F.wing_mpc_solve(s0[:B].to(dev), ref[:B].to(dev), DT, nominal(), iters=iters,
                           want_trace=True)
    check_solve(got, cut(f32[iters]), cut(f64[iters]), f"kernel B={B} iters={iters}")


def test_u0_semantics(dev):
    from apg_trajectory_tracking_amd import functional as F
    check_u0_semantics(lambda s0, ref, u0, iters: F.wing_mpc_solve(
        s0, ref, DT, nominal(), u0=u0, iters=iters), dev)
    # and no trace unless it is asked for
    s0, ref, _ = R.solve_case(F64)
    assert F.wing_mpc_solve(s0[:4].to(dev), ref[:4].to(dev), DT, nominal())["trace"] is None


def _loop_on_device(dev, case, T=R.LOOP_T, targets=None):
    from apg_trajectory_tracking_amd import functional as F
    st = R.LOOP_SETTINGS[case]
    tg = R.loop_targets() if targets is None else targets
    out = F.wing_mpc_closed_loop(
        tg.to(dev), DT, R.params(st["plant"]), model_params=nominal(), max_steps=T,
        thresh_div=st["thresh_div"], thresh_stable=R.THRESH_STABLE, test_time=st["test_time"],
        want_trajectory=True, iters=10)
    return R.from_device_layout(out)


def test_closed_loop_kernel_vs_the_restated_loop(dev):
    """As test_closed_loop_twin_vs_the_restated_loop, the kernel in the twin's
    place: 70 flights = one full workgroup and a ragged second one; flights
    32..39 end early while their wave flies on."""
    check_loop(_loop_on_device(dev, "nominal"), "nominal", "kernel nominal")


@pytest.mark.parametrize("case", ["break", "reset"])
def test_closed_loop_kernel_with_failing_flights(dev, case):
    """As test_closed_loop_twin_with_failing_flights."""
    f64 = check_loop(_loop_on_device(dev, case), case, f"kernel {case}")
    assert int((f64["failures"] > 0).sum()) >= 1


def test_closed_loop_kernel_model_mismatch(dev):
    """As test_closed_loop_twin_model_mismatch: plant mass 1.3 / CL_alpha 4.0,
    model nominal."""
    got = _loop_on_device(dev, "mismatch")
    check_loop(got, "mismatch", "kernel mismatch")
    check_mismatch_differs(got, "kernel mismatch")


def test_mpc_object_surface_and_warm_start(dev):
    loop = _loop_on_device(dev, "nominal", T=2, targets=R.loop_targets()[:, :1])
    check_mpc_object(loop, "cuda")


def test_evaluator_flies_the_mpc_and_reports_its_statistics(dev):
    check_evaluator("cuda")


def test_optimality_gap_of_the_shipped_controller(dev):
    """functional.wing_policy_optimality_gap on the shipped fixed-wing controller
    (a Net(9, 1, 3, 40, conv=False)), B = 128 starts of synthetic.wing_batch, 50
    iterations: a descent method started at the policy's own plan ends at or
    below the policy's cost.  Heavy ball is not monotone per iteration, so a few
    trajectories may end above: as many as the float64 restatement itself shows
    from the same plans, no more.  "Above" is judged beyond 1e-6 relative."""
    from apg_trajectory_tracking_amd import functional as F, synthetic
    net = wing_loop_policy(dev)
    assert net.fc_out.weight.shape[0] == 40
    d = wing_flight_cases.data()
    B, iters = 128, 50
    batch = synthetic.wing_batch(B, R.H, DT, seed=17)
    s0, ref = batch["state0"], batch["ref"]
    before = s0.clone()
    gap = F.wing_policy_optimality_gap(net, d["mean"], d["std"], s0.to(dev), ref.to(dev), DT,
                                       nominal(), iters=iters)
    assert torch.equal(s0, before)
    acts = gap["actions"].cpu()
    assert acts.shape == (B, R.H, 4) and float(acts.min()) >= 0 and float(acts.max()) <= 1
    # the plan is the module's own forward on the data set's inputs
    with torch.no_grad():
        normed = ((s0 - torch.from_numpy(d["mean"])) / torch.from_numpy(d["std"]))[:, 3:]
        want = torch.sigmoid(wing_loop_policy("cpu")(normed, ref[:, -1] - s0[:, :3]))
    assert float((acts.reshape(B, 40) - want).abs().max()) < 1e-5
    pol, warm, cold = N(gap["policy"]), N(gap["mpc_from_policy"]), N(gap["mpc"])
    with R.few_threads():
        r64 = R.solve(F64, s0, ref, acts, DT, iters)
    pol64, warm64 = N(r64["trace"][0]), N(r64["cost"])
    assert np.abs(pol - pol64).max() <= 1e-4 * pol64.max()
    above64 = int((warm64 > pol64 * (1 + 1e-6)).sum())
    above = int((warm > pol * (1 + 1e-6)).sum())
    print("optimality gap: mean policy cost %.4f, MPC from the policy %.4f, MPC from the cold "
          "start %.4f; above the policy: %d (float64 restatement: %d)"
          % (pol.mean(), warm.mean(), cold.mean(), above, above64))
    assert warm.mean() < pol.mean()
    assert above <= above64
