"""The shooting MPC that plans through the learnt simulator on the MI355X
(apg_quad_learnt_mpc_solve, apg_quad_learnt_mpc_closed_loop through functional
/ controllers.MPC / QuadEvaluator) under the same float64 arbiter as the host
twins (tests/test_quad_learnt_mpc_cpu.py, tests/quad_learnt_mpc_restatement.py).
kernel == twin is NOT demanded bit for bit (the device compiler contracts and
orders operations in its own way, and the plant's step uses the hardware sin /
cos): both stand under the same arbiter.  Every test launches once; none
repeats a failing launch."""
import numpy as np
import pytest
import torch

import quad_learnt_mpc_restatement as L
import quad_mpc_restatement as R
from conftest import assert_no_worse_than_fp32, load_golden
from test_quad_learnt_mpc_cpu import check_solve, experiment

pytestmark = pytest.mark.gpu
DT = L.DT
F64, F32 = torch.float64, torch.float32
N = R.to_numpy


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def solve(dev, dyn, s0, ref, u0=None, **kw):
    from apg_trajectory_tracking_amd import functional as F
    return F.quad_mpc_solve(s0.to(dev), ref.to(dev), DT, dyn.params,
                            u0=None if u0 is None else u0.to(dev), learnt=dyn, **kw)


@pytest.mark.parametrize("iters", [1, 10])
@pytest.mark.parametrize("which", ["golden", "steps"])
def test_solve_kernel_under_the_fp64_arbiter(dev, which, iters):
    """Cases S1 and S2 of test_solve_twin_under_the_fp64_arbiter, the kernel in
    the twin's place: same arbiter, same caps."""
    s0, ref, u0 = L.windows()
    got = solve(dev, L.module(which, dev), s0, ref, u0, iters=iters, want_trace=True)
    check_solve(got, L.solve_case(which, F32)[iters], L.solve_case(which, F64)[iters], iters,
                f"kernel {which} iters={iters}")


def test_tail_shapes_and_repeatability(dev):
    """S1's first B = 1, 63, 65 rows and 257 rows (the 256 windows and row 0
    once more) give the bits of the B = 256 run, row for row; the caller's
    start tensor is left alone; a second call gives the same bits."""
    s0, ref, u0 = L.windows()
    dyn = L.module("golden", dev)
    start = u0.to(dev)
    full = solve(dev, dyn, s0, ref, start, want_trace=True)
    assert torch.equal(start, u0.to(dev))
    again = solve(dev, dyn, s0, ref, start, want_trace=True)
    for k in ("u", "cost", "trace"):
        assert torch.equal(again[k], full[k]), k
    none = solve(dev, dyn, s0, ref)            # u0 = None is u = 0.5
    assert torch.equal(none["u"], full["u"]) and none["trace"] is None
    for B in (1, 63, 65):
        part = solve(dev, dyn, s0[:B], ref[:B], u0[:B], want_trace=True)
        assert torch.equal(part["u"], full["u"][:B]), B
        assert torch.equal(part["cost"], full["cost"][:B]), B
        assert torch.equal(part["trace"], full["trace"][:, :B]), B
    idx = torch.cat((torch.arange(256), torch.zeros(1, dtype=torch.long)))
    more = solve(dev, dyn, s0[idx], ref[idx], u0[idx], want_trace=True)
    assert torch.equal(more["u"], full["u"][idx.to(dev)])
    assert torch.equal(more["cost"], full["cost"][idx.to(dev)])
    assert torch.equal(more["trace"], full["trace"][:, idx.to(dev)])


def test_a_zero_residual_is_the_analytic_kernel(dev):
    """A freshly constructed LearntDynamics: u and cost of the learnt-model
    kernel equal those of apg_quad_mpc_solve on the module's parameters within
    1e-6."""
    from apg_trajectory_tracking_amd import functional as F
    s0, ref, u0 = L.windows()
    dyn = L.module("zero", dev)
    got = solve(dev, dyn, s0, ref, u0)
    want = F.quad_mpc_solve(s0.to(dev), ref.to(dev), DT, dyn.params, u0=u0.to(dev))
    assert np.abs(N(got["u"]) - N(want["u"])).max() <= 1e-6
    assert np.abs(N(got["cost"]) - N(want["cost"])).max() <= 1e-6 * N(want["cost"]).max()


@pytest.mark.parametrize("test_time", [0, 1])
@pytest.mark.parametrize("plant", ["learnt", "drags"])
def test_evaluator_flies_the_learnt_model(dev, plant, test_time):
    """test_closed_loop_twin_vs_the_restated_loop through
    QuadEvaluator(MPC(learnt_model=m), env)._closed_loop: the learnt plant (the
    same module) and the analytic plant with the two drags."""
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    from apg_trajectory_tracking_amd.evaluate_drone import QuadEvaluator
    dyn = L.module("loop", dev)
    env = dyn if plant == "learnt" else FlightmareDynamics(modified_params=R.DRAGS)
    ev = QuadEvaluator(MPC(horizon=10, dt=DT, learnt_model=dyn), env, dt=DT,
                       test_time=test_time)
    assert ev.learnt is (dyn if plant == "learnt" else None)
    with torch.no_grad():
        out = ev._closed_loop(L.loop_trajectories(300).to(dev), max_steps=30, thresh_div=0.6,
                              thresh_stable=1.0, test_time=test_time)
    L.same_flights(out["steps"].cpu(), out["div"].t().cpu(), L.loop_case(plant, test_time), 300,
                   f"kernel plant={plant} test_time={test_time}")


def test_planning_with_the_adapted_model_pays(dev):
    """The experiment of the CPU test on the device: the nominal arm is the
    existing kernel (apg_quad_mpc_closed_loop, learnt plant, nominal model)."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    plant = L.module("loop", dev)
    traj = L.loop_trajectories(32, 120).to(dev)

    def fly(model):
        kw = (dict(model_learnt=plant) if model == "learnt"
              else dict(model_params=FlightmareDynamics().params))
        o = F.quad_mpc_closed_loop(traj, DT, plant.params, learnt=plant, iters=10,
                                   max_steps=100, thresh_div=3.0, thresh_stable=1.0,
                                   test_time=0, want_trajectory=True, **kw)
        return dict(div=o["div"].t(), steps=o["steps"], start=o["start_states"].permute(2, 0, 1),
                    drone=o["drone"].permute(2, 0, 1))
    experiment(fly)


def test_optimality_gap_on_the_learnt_model(dev):
    """functional.quad_policy_optimality_gap(..., learnt=module) on the shipped
    quad controller: the policy's plan (unrolled through the module where the
    policy is a one-step one), its cost and both MPC costs are the learnt
    model's.  The policy cost stands under the arbiter against the float64
    oracle's cost of the same plan through LearntQuadOracle; a descent started
    at the plan ends above it (beyond 1e-6 relative) on no more trajectories
    than the float64 restatement shows from the same plans."""
    from apg_trajectory_tracking_amd import functional as F, synthetic
    from apg_trajectory_tracking_amd.checkpoint import build_policy
    ck = load_golden("checkpoints.npz")
    net = build_policy("quad", {k[len("quad.w."):]: torch.from_numpy(ck[k])
                                for k in ck.files if k.startswith("quad.w.")}).to(dev).eval()
    dyn = L.module("loop", dev)
    B, iters = 512, 50
    d = synthetic.quad_polynomial_batch(B, 10, DT, seed=3, ref_length=20)
    gap = F.quad_policy_optimality_gap(net, d["state0"].to(dev), d["in_ref"].to(dev),
                                       d["ref"].to(dev), DT, dyn.params, iters=iters, learnt=dyn)
    acts = gap["actions"].cpu()
    assert acts.shape == (B, 10, 4) and float(acts.min()) >= 0 and float(acts.max()) <= 1
    window = d["ref"][:, :10]
    r64 = L.solve_snapshots(F64, L.oracle("loop", F64), d["state0"], window, acts, DT, (0, iters))
    pol32 = R.cost(L.oracle("loop", F32), d["state0"], window, acts, DT)
    pol, warm, cold = N(gap["policy"]), N(gap["mpc_from_policy"]), N(gap["mpc"])
    pol64, warm64 = N(r64[0]["cost"]), N(r64[iters]["cost"])
    assert_no_worse_than_fp32(pol[:, None], N(pol32)[:, None], pol64[:, None], "policy cost")
    above64 = int((warm64 > pol64).sum())
    above = int((warm > pol * (1 + 1e-6)).sum())
    print("optimality gap on the learnt model: mean policy cost %.4f, MPC from the policy %.4f, "
          "MPC from 0.5 %.4f; above the policy: %d (float64 restatement: %d)"
          % (pol.mean(), warm.mean(), cold.mean(), above, above64))
    assert above <= above64
    assert warm.mean() < pol.mean()
    # and the learnt model is what was judged: on the nominal one the plan costs otherwise
    nominal = F.quad_mpc_solve(d["state0"].to(dev), window.to(dev), DT, dyn.params,
                               u0=gap["actions"], iters=0)["cost"]
    assert np.abs(N(nominal) - pol).max() > 1e-3 * pol.max()


def test_a_solve_can_be_captured(dev):
    """One solve recorded into a torch.cuda.graph on a side stream and replayed
    twice gives the bits of the eager call: pack and solve run on the caller's
    stream, nothing is allocated or synchronised inside the library."""
    s0, ref, u0 = L.windows()
    dyn = L.module("golden", dev)
    s, r, u = s0.to(dev), ref.to(dev), u0.to(dev)
    eager = solve(dev, dyn, s, r, u, want_trace=True)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        got = solve(dev, dyn, s, r, u, want_trace=True)
    for _ in range(2):
        for k in ("u", "cost", "trace"):
            got[k].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        for k in ("u", "cost", "trace"):
            assert torch.equal(got[k], eager[k]), k
