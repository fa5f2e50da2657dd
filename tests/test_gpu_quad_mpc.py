"""The batched shooting MPC on the MI355X (apg_quad_mpc_solve,
apg_quad_mpc_closed_loop through functional / controllers.MPC / QuadEvaluator)
under the same float64 arbiter as the host twins (tests/test_quad_mpc_cpu.py,
tests/quad_mpc_restatement.py).  kernel == twin is NOT demanded bit for bit
(the device compiler contracts and orders operations in its own way, and the
plant's step uses the hardware sin / cos, see make_trig): both stand under the
same arbiter.  Every test launches once; none repeats a failing launch."""
import ast
import functools

import numpy as np
import pytest
import torch

import quad_mpc_restatement as R
from conftest import assert_no_worse_than_fp32, load_golden
from test_quad_mpc_cpu import check_loop, check_solve, clamp_is_exercised

pytestmark = pytest.mark.gpu
DT = 0.1
F64, F32 = torch.float64, torch.float32
N = R.to_numpy
ITERS = (1, 10, 20)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def solve_case(B):
    """(state0, ref, u0, {iters: float64}, {iters: float32}) - one restated run
    of 20 iterations per dtype serves the three iteration counts."""
    s0, ref = R.experiment_windows(B=B)
    u0 = torch.full((B, R.H, 4), 0.5)
    return (s0, ref, u0, R.solve_snapshots(F64, s0, ref, u0, DT, ITERS),
            R.solve_snapshots(F32, s0, ref, u0, DT, ITERS))


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("B", [256, 65536 + 7])
def test_solve_kernel_under_the_fp64_arbiter(dev, B, iters):
    """The experiment's windows at B = 256 and with a ragged tail wave.
    Measured on the MI355X: the device's median error of `u` equals the float32
    restatement's (1.5e-7 against 1.6e-7 of the trajectory's scale).  The
    tightest case is B = 65 543, 20 iterations, `u`: its worst trajectory - one
    where the fixed step carries rounding noise from iteration to iteration
    with a gain above one - ends 8.07e-5 away from float64 (float32
    restatement 7.72e-5 on the same trajectory; bar 1e-4); at 10 iterations
    1.94e-5 against 1.42e-5.  Costs and traces stay below 7e-6 everywhere."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    s0, ref, u0, f64, f32 = solve_case(B)
    if iters == 20:
        clamp_is_exercised(f64[20]["u"])
    got = F.quad_mpc_solve(s0.to(dev), ref.to(dev), DT, FlightmareDynamics().params,
                           u0=u0.to(dev), iters=iters, want_trace=True)
    check_solve(got, f32[iters], f64[iters], f"kernel B={B} iters={iters}")
    # u0 = None is u = 0.5, and the caller's start tensor is left alone
    if B == 256 and iters == 10:
        again = F.quad_mpc_solve(s0.to(dev), ref.to(dev), DT, FlightmareDynamics().params)
        assert torch.equal(again["u"], got["u"]) and again["trace"] is None
        six = torch.cat((ref[:, :, :3], ref[:, :, 6:9]), 2).to(dev)
        packed = F.quad_mpc_solve(s0.to(dev), six, DT, FlightmareDynamics().params)
        assert torch.equal(packed["u"], got["u"])


def _loop_on_device(dev, mismatch, **kw):
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    traj, _ = R.loop_case(F64, mismatch)
    plant = FlightmareDynamics(modified_params=R.DRAGS if mismatch else {})
    out = F.quad_mpc_closed_loop(
        traj.to(dev), DT, plant.params, model_params=FlightmareDynamics().params,
        iters=10, max_steps=250, thresh_div=R.LOOP_THRESH_DIV, thresh_stable=1.0,
        test_time=0, want_trajectory=True, **kw)
    return dict(div=out["div"].t(), steps=out["steps"].long().cpu(),
                drone=out["drone"].permute(2, 0, 1), actions=out["actions"].permute(2, 0, 1),
                cost=out["cost"].t())


def test_closed_loop_kernel_vs_the_restated_loop(dev):
    """As test_closed_loop_twin_vs_the_restated_loop, the kernel in the twin's place."""
    got = _loop_on_device(dev, False)
    f64 = check_loop(got, False, "kernel nominal")
    _, f32 = R.loop_case(F32, False)
    assert_no_worse_than_fp32(N(got["cost"]), N(f32["cost"]), N(f64["cost"]), "kernel cost")


def test_closed_loop_kernel_model_mismatch(dev):
    """As test_closed_loop_twin_model_mismatch: plant with the two drags, model nominal."""
    got = _loop_on_device(dev, True)
    f64 = check_loop(got, True, "kernel mismatch")
    _, nominal = R.loop_case(F64, False)
    assert float(f64["div"].mean()) > float(nominal["div"].mean())
    assert float(got["div"].mean()) > float(nominal["div"].mean())


def test_evaluator_flies_the_mpc_and_reports_the_six_statistics(dev):
    """`QuadEvaluator(MPC(...), FlightmareDynamics()).run_eval(nr_test=64)`: the
    six statistics equal the ones computed from the float64 restatement's div /
    steps on the same 64 trajectories."""
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    from apg_trajectory_tracking_amd.evaluate_drone import QuadEvaluator
    ev = QuadEvaluator(MPC(horizon=10, dt=DT), FlightmareDynamics(), dt=DT)
    traj = ev.reference_batch(64, seed=42)
    got = ev.run_eval(nr_test=64, trajectories=traj)
    assert len(got) == 6
    ref = R.closed_loop(F64, traj, DT, 10, 251, 1.0, 1.0, 0)
    steps = ref["steps"].numpy()
    valid = np.arange(ref["div"].shape[1])[None] < steps[:, None]
    div = (N(ref["div"]) * valid).sum(1) / np.maximum(steps, 1)
    stable = (valid & (N(ref["div"]) < 1.0)).sum(1)
    full = div[stable == steps[-1]]
    want = (np.mean(stable), np.std(stable), np.mean(full), np.std(full), np.mean(div),
            np.std(div))
    print("run_eval:", got, "restatement:", want, "resets:", ref["resets"])
    assert np.allclose(got, want, rtol=1e-3, atol=1e-4), (got, want)
    # follow_trajectory works unchanged on top
    refs, drone, divs, acts = ev.follow_trajectory("rand", max_nr_steps=20, thresh_div=3,
                                                   thresh_stable=1, trajectories=traj[:4])
    assert len(divs) == 4 and drone[0].shape == (21, 12) and acts[0].shape == (20, 4)
    assert np.abs(N(divs[0]) - N(ref["div"][0, :20])).max() < 1e-4


def test_evaluator_flies_the_mpc_through_the_learnt_simulator(dev):
    """Plant = LearntDynamics (action transform, analytic step, residual), model
    = the MPC's nominal parameters, against the restatement through
    torch_port.LearntQuadOracle with the acceptance rule of
    test_closed_loop_learnt_simulator_large_batch_vs_oracle: same `steps` on
    > 97 % of the flights, `div` within 2e-3 on all but 3 % of those (the
    residual makes resets possible here)."""
    from apg_trajectory_tracking_amd import synthetic
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    from apg_trajectory_tracking_amd.evaluate_drone import QuadEvaluator
    from oracle import torch_port as tp
    g = load_golden("closed_loop_learnt.npz")
    init = {kv.split("=")[0]: ast.literal_eval(kv.split("=")[1]) for kv in g["init"]}
    weights = {k[len("dyn."):]: g[k] for k in g.files if k.startswith("dyn.")}
    dyn = LearntDynamics(initial_params=init)
    dyn.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    dyn = dyn.to(dev)
    B, L, steps = 300, 40, 30
    traj = synthetic.quad_eval_trajectories(B, L, DT, seed=9)
    traj[:, :, 2] += 3
    for test_time in (0, 1):
        ev = QuadEvaluator(MPC(horizon=10, dt=DT), dyn, dt=DT, test_time=test_time)
        assert ev.learnt is dyn
        with torch.no_grad():
            out = ev._closed_loop(traj.to(dev), max_steps=steps, thresh_div=0.6,
                                  thresh_stable=1.0, test_time=test_time)
        ref = R.closed_loop(F32, traj, DT, 10, steps, 0.6, 1.0, test_time,
                            plant=tp.LearntQuadOracle(weights, init))
        print("learnt plant, test_time", test_time, "failed (flight, step) pairs:",
              ref["resets"], "steps:", ref["steps"].float().mean().item())
        same = [i for i in range(B) if int(out["steps"][i]) == int(ref["steps"][i])]
        assert len(same) > 0.97 * B, test_time
        bad = [i for i in same
               if np.abs(N(out["div"][:int(ref["steps"][i]), i])
                         - N(ref["div"][i, :int(ref["steps"][i])])).max() > 2e-3]
        assert len(bad) <= 0.03 * B, (test_time, len(bad))


def test_optimality_gap_of_the_shipped_controller(dev):
    """functional.quad_policy_optimality_gap on the shipped quad controller
    (tests/golden/checkpoints.npz): a descent method started at the policy's
    own plan ends at or below the policy's cost.  Heavy ball is not monotone per
    iteration, so a handful of trajectories may end above: as many as the
    float64 restatement itself shows from the same plans, no more.  "Above"
    is judged beyond float32's rounding of the two costs (1e-6 relative: both
    are sums of ~100 positive float32 terms)."""
    from apg_trajectory_tracking_amd import functional as F, synthetic
    from apg_trajectory_tracking_amd.checkpoint import build_policy
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    ck = load_golden("checkpoints.npz")
    net = build_policy("quad", {k[len("quad.w."):]: torch.from_numpy(ck[k])
                                for k in ck.files if k.startswith("quad.w.")}).to(dev).eval()
    B, iters = 512, 50
    d = synthetic.quad_polynomial_batch(B, 10, DT, seed=3, ref_length=20)
    params = FlightmareDynamics().params
    gap = F.quad_policy_optimality_gap(net, d["state0"].to(dev), d["in_ref"].to(dev),
                                       d["ref"].to(dev), DT, params, iters=iters)
    acts = gap["actions"].cpu()
    assert acts.shape == (B, 10, 4) and float(acts.min()) >= 0 and float(acts.max()) <= 1
    pol, warm, cold = N(gap["policy"]), N(gap["mpc_from_policy"]), N(gap["mpc"])
    r64 = R.solve(F64, d["state0"], d["ref"][:, :10], acts, DT, iters)
    pol64, warm64 = N(r64["trace"][0]), N(r64["cost"])
    assert np.abs(pol - pol64).max() <= 1e-4 * pol64.max()
    above64 = int((warm64 > pol64).sum())
    above = int((warm > pol * (1 + 1e-6)).sum())
    print("optimality gap: mean policy cost %.4f, MPC from the policy %.4f, MPC from 0.5 %.4f; "
          "mean gap %.4f (%.1f %%); above the policy: %d (float64 restatement: %d)"
          % (pol.mean(), warm.mean(), cold.mean(), (pol - warm).mean(),
             100 * (pol - warm).mean() / pol.mean(), above, above64))
    assert above <= above64
    assert warm.mean() < pol.mean()
