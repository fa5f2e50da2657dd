"""The cart-pole shooting MPC that plans through the learnt simulator on the
MI355X (apg_cartpole_learnt_mpc_solve, apg_cartpole_learnt_mpc_closed_loop through
functional / controllers.MPC / evaluate_cartpole.Evaluator) under the same
float64 arbiter as the host twins (tests/test_cartpole_learnt_mpc_cpu.py,
tests/cartpole_learnt_mpc_restatement.py).  kernel == twin is NOT demanded bit
for bit: both stand under the same arbiter.  Every test launches once; none
repeats a failing launch."""
import copy
import functools

import numpy as np
import pytest
import torch

import cartpole_learnt_mpc_restatement as L
import cartpole_mpc_restatement as R
from conftest import assert_no_worse_than_fp32
from test_cartpole_learnt_mpc_cpu import (check_learnt_loop, clamp_is_exercised,
                                          neither_swapped_nor_aliased,
                                          zero_residual_is_the_analytic_solver)
from test_cartpole_mpc_cpu import check_solve

pytestmark = pytest.mark.gpu
DT = L.DT
F64, F32 = torch.float64, torch.float32
N = R.to_numpy


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def on(dev, which="fitted"):
    """A copy of the restatement's module on the device (the cached one stays on
    the host)."""
    return copy.deepcopy(L.module(which)).to(dev)


def solve(dev, mod, s0, u0=None, **kw):
    from apg_trajectory_tracking_amd import functional as F
    return F.cartpole_mpc_solve(s0.to(dev), DT, None, u0=None if u0 is None else u0.to(dev),
                                learnt=mod, **kw)


def loop(dev, s0, model, plant=None, plant_params=None, steps=L.LOOP_STEPS, horizon=L.H):
    """model: a device module, or None: the analytic solver on the nominal
    parameters; plant: a device module, or None: `plant_params`."""
    from apg_trajectory_tracking_amd import functional as F
    kw = dict(model_params=R.params()) if model is None else dict(model_learnt=model)
    out = F.cartpole_mpc_closed_loop(
        s0.to(dev), DT, None if plant is not None else R.params(plant_params), learnt=plant,
        max_steps=steps, mode="balance", thresh_div=0.21, burn_in=0, want_trajectory=True,
        iters=10, horizon=horizon, **kw)
    return R.from_device_layout(out)


@pytest.mark.parametrize("iters", [1, 10, 20])
def test_solve_kernel_under_the_fp64_arbiter(dev, iters):
    """The thirds of test_solve_twin_under_the_fp64_arbiter, B = 256."""
    s0, parts, f64 = L.solve_case(F64)
    _, _, f32 = L.solve_case(F32)
    if iters == 20:
        clamp_is_exercised(f64[20]["u"][parts[1]])
    got = solve(dev, on(dev), s0, iters=iters, want_trace=True)
    check_solve(got, f32[iters], f64[iters], f"kernel iters={iters}")


@functools.lru_cache(maxsize=None)
def ragged_case(dtype, B=4096 + 7):
    """-> starts, the restated solve, and (float64) the kink flags of the run."""
    s0, _ = R.thirds(B)
    model = L.LearntModel(L.module(), dtype).watch(B)
    return s0, L.solve(model, dtype, s0, torch.zeros(B, L.H, 1), DT, 10), model.kink


def test_a_ragged_many_workgroup_solve(dev):
    """B = 4 096 + 7 (65 workgroups, a last wave of 7 lanes), R.thirds starts,
    10 iterations.  Among thousands of full-range starts some come within
    float32's reach of a ReLU kink: where the float64 run has a hidden
    pre-activation with |z_j| < 1e-5 (|b1_j| + sum_i |W1_ji| |x_i|) at any step of
    any sweep (L.KINK, the quadrotor's rule), a float32 evaluation may take the
    other branch and descends along another gradient from there on (on the CPU:
    trajectory 2354 carries the flag, and the float32 RESTATEMENT and the host
    twin both end 2.06e-3 from float64 in u there, equal to each other).  Those
    trajectories are set aside by the float64 run's flags alone - 6.0 % of them;
    void above 12 % - the others stand under the arbiter; on ALL trajectories u
    stays in the box, every value is finite and the last trace row is the
    returned cost."""
    s0, f64, kink = ragged_case(F64)
    _, f32, _ = ragged_case(F32)
    share = float(kink.double().mean())
    print("ragged solve: kink share %.4f" % share)
    assert share <= 0.12, f"void: kink share {share}"
    got = solve(dev, on(dev), s0, iters=10, want_trace=True)
    u = got["u"].cpu()
    assert got["u"].shape == (4103, L.H, 1) and bool(torch.isfinite(u).all())
    assert float(u.min()) >= -1.0 and float(u.max()) <= 1.0
    assert bool(torch.isfinite(got["trace"]).all())
    assert torch.equal(got["trace"][-1], got["cost"])
    ok = ~kink
    rows = lambda d: dict(u=d["u"].cpu()[ok], cost=d["cost"].cpu()[ok],
                          trace=d["trace"].cpu()[:, ok])
    check_solve(rows(got), rows(f32), rows(f64), "kernel B=4103")


def test_horizon_five(dev):
    """The H = 5 instantiations: the solve under the arbiter (the 96 starts of
    the twin's test) and both closed-loop kernels - learnt and analytic plant -
    against the float32 restatement, 16 near-upright starts, 12 steps (some
    flights leave early; |theta| never within 1.9e-3 of thresh_div)."""
    s0, _, f64 = L.solve_case(F64, 96, 5, 2)
    _, _, f32 = L.solve_case(F32, 96, 5, 2)
    m = on(dev)
    check_solve(solve(dev, m, s0, iters=10, horizon=5, want_trace=True), f32[10], f64[10],
                "kernel H=5")
    starts = L.loop_starts()[32:48]
    model = L.LearntModel(L.module(), F32)
    for plant, restated in ((m, R.LearntPlant(L.module(), F32)), (None, tp_plant(None))):
        got = loop(dev, starts, m, plant=plant, steps=12, horizon=5)
        want = L.closed_loop(F32, starts, DT, 10, 12, model, restated, horizon=5)
        assert want["margin"] > 1e-3        # void if a flight grazes thresh_div
        L.same_flights(got, want, "kernel H=5 plant=%s" % ("learnt" if plant else "analytic"))


def test_tail_shapes_and_repeatability(dev):
    """The first B = 1, 63, 65 rows and 257 rows (the 256 starts and row 0 once
    more) give the bits of the B = 256 run, row for row; the caller's u0 is left
    alone; a second call gives the same bits."""
    s0, _, f64 = L.solve_case(F64)
    u0 = f64[1]["u"].float()                 # some start that is not 0
    mod = on(dev)
    start = u0.to(dev)
    full = solve(dev, mod, s0, start, want_trace=True)
    assert torch.equal(start, u0.to(dev))
    again = solve(dev, mod, s0, start, want_trace=True)
    for k in ("u", "cost", "trace"):
        assert torch.equal(again[k], full[k]), k
    for B in (1, 63, 65):
        part = solve(dev, mod, s0[:B], u0[:B], want_trace=True)
        assert torch.equal(part["u"], full["u"][:B]), B
        assert torch.equal(part["cost"], full["cost"][:B]), B
        assert torch.equal(part["trace"], full["trace"][:, :B]), B
    idx = torch.cat((torch.arange(256), torch.zeros(1, dtype=torch.long)))
    more = solve(dev, mod, s0[idx], u0[idx], want_trace=True)
    assert torch.equal(more["u"], full["u"][idx.to(dev)])
    assert torch.equal(more["cost"], full["cost"][idx.to(dev)])
    assert torch.equal(more["trace"], full["trace"][:, idx.to(dev)])
    # u0 = None is u0 = 0
    zero = solve(dev, mod, s0, torch.zeros(256, L.H, 1))
    none = solve(dev, mod, s0)
    assert torch.equal(none["u"], zero["u"]) and none["trace"] is None


def test_a_zero_residual_is_the_analytic_kernel(dev):
    from apg_trajectory_tracking_amd import functional as F
    zero_residual_is_the_analytic_solver(
        lambda mod, s0: solve(dev, on(dev, "zero"), s0),
        lambda s0: F.cartpole_mpc_solve(s0.to(dev), DT, R.params()))


def test_balance_loop_kernel_on_the_learnt_plant_with_the_learnt_model(dev):
    """As test_balance_loop_twin_on_the_learnt_plant_with_the_learnt_model, the
    kernel in the twin's place (one module in both roles)."""
    m = on(dev)
    check_learnt_loop(loop(dev, L.loop_starts(), m, plant=m), "kernel")


def test_planning_with_the_adapted_model_pays(dev):
    """As the twins' test: both arms from the kernels on the learnt plant."""
    m = on(dev)
    learnt = loop(dev, L.loop_starts(), m, plant=m)
    nominal = loop(dev, L.loop_starts(), None, plant=m)
    L.pays(learnt, nominal, "kernels")


def test_model_and_plant_are_neither_swapped_nor_aliased(dev):
    """Two row tables in one launch: model = fitted with plant = second flies
    another path than the roles swapped; and the analytic plant under the learnt
    model against the float32 restatement."""
    s0 = L.loop_starts()[16:32]
    mods = {id(L.module(w)): on(dev, w) for w in ("fitted", "second")}
    neither_swapped_nor_aliased(
        lambda model, plant: loop(dev, s0, mods[id(model)], plant=mods[id(plant)], steps=12))
    got = loop(dev, s0, mods[id(L.module())], plant_params=R.MISMATCH, steps=12)
    want = L.closed_loop(F32, s0, DT, 10, 12, L.LearntModel(L.module(), F32),
                         tp_plant(R.MISMATCH))
    L.same_flights(got, want, "kernel analytic plant")


def tp_plant(modified):
    from oracle import torch_port as tp
    return tp.CartpoleOracle(modified, dtype=F32)


def test_evaluator_flies_the_mpc_with_the_learnt_model(dev):
    """`Evaluator(MPC(horizon=10, dt=0.05, dynamics="cartpole", learnt_model=m),
    CartPoleEnv(m, 0.05, thresh_div=0.21))._fly(...)` flies the case of
    test_balance_loop_kernel_on_the_learnt_plant_with_the_learnt_model."""
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.evaluate_cartpole import CartPoleEnv, Evaluator
    m = on(dev)
    np.random.seed(2)
    ev = Evaluator(MPC(horizon=10, dt=DT, dynamics="cartpole", learnt_model=m),
                   CartPoleEnv(m, DT, thresh_div=0.21))
    with torch.no_grad():
        out = R.from_device_layout(ev._fly(L.loop_starts().numpy(), L.LOOP_STEPS, "balance", 0))
    check_learnt_loop(out, "evaluator")
    assert ev.last_flights["cost"].shape == (L.LOOP_STEPS, 64)


def test_optimality_gap_on_the_learnt_model(dev):
    """functional.cartpole_policy_optimality_gap(..., learnt=m) on the shipped
    controller, B = 512 near-upright starts, 50 iterations: the policy cost
    under the arbiter against the float64 restatement of the same plan through
    the learnt model; the warm descent ends above the policy on no more
    trajectories than the float64 restatement shows ("above": beyond 1e-6
    relative); the same plan costs otherwise on the nominal model."""
    from apg_trajectory_tracking_amd import functional as F
    from test_cartpole_eval_cpu import golden_net
    net = golden_net(None, "shipped").to(dev).eval()
    B, iters = 512, 50
    s0 = R.near_upright(B, torch.Generator().manual_seed(13)).float()
    m = on(dev)
    gap = F.cartpole_policy_optimality_gap(net, s0.to(dev), DT, None, iters=iters, learnt=m)
    acts = gap["actions"].cpu()
    assert acts.shape == (B, L.H, 1) and float(acts.abs().max()) <= 1
    pol, warm, cold = N(gap["policy"]), N(gap["mpc_from_policy"]), N(gap["mpc"])
    r64 = L.solve(L.LearntModel(L.module(), F64), F64, s0, acts, DT, iters)
    pol64, warm64 = N(r64["trace"][0]), N(r64["cost"])
    pol32 = N(L.cost(L.LearntModel(L.module(), F32), s0, acts, DT))
    assert_no_worse_than_fp32(pol[:, None], pol32[:, None], pol64[:, None], "policy cost")
    above64 = int((warm64 > pol64 * (1 + 1e-6)).sum())
    above = int((warm > pol * (1 + 1e-6)).sum())
    nominal = N(F.cartpole_mpc_solve(s0.to(dev), DT, R.params(), u0=gap["actions"],
                                     iters=0)["cost"])
    apart = float(np.abs(pol - nominal).max() / nominal.max())
    print("optimality gap on the learnt model: mean policy cost %.4f (nominal model %.4f, "
          "largest difference %.3e relative), MPC from the policy %.4f, MPC from 0 %.4f; above "
          "the policy: %d (float64 restatement: %d)"
          % (pol.mean(), nominal.mean(), apart, warm.mean(), cold.mean(), above, above64))
    assert warm.mean() < pol.mean()
    assert above <= above64
    assert apart > 1e-3


def test_a_solve_can_be_captured_and_reads_the_parameters_on_the_device(dev):
    """One solve recorded into a torch.cuda.graph on a side stream and replayed
    twice gives the eager call's bits; after an in-place change of
    m.cfg["length"] a further replay gives the bits of an eager call made after
    that change: the six parameters are read inside the kernel."""
    s0, _, _ = L.solve_case(F64)
    m = on(dev)
    s = s0.to(dev)
    eager = solve(dev, m, s, want_trace=True)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        got = solve(dev, m, s, want_trace=True)
    for _ in range(2):
        for k in ("u", "cost", "trace"):
            got[k].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        for k in ("u", "cost", "trace"):
            assert torch.equal(got[k], eager[k]), k
    with torch.no_grad():
        m.cfg["length"].fill_(0.7)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    changed = solve(dev, m, s, want_trace=True)
    assert not torch.equal(changed["u"], eager["u"])
    for k in ("u", "cost", "trace"):
        assert torch.equal(got[k], changed[k]), k
