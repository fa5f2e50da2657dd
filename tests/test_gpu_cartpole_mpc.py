"""The batched cart-pole shooting MPC on the MI355X (apg_cartpole_mpc_solve,
apg_cartpole_mpc_closed_loop through functional / controllers.MPC /
evaluate_cartpole.Evaluator) under the same float64 arbiter as the host twins
(tests/test_cartpole_mpc_cpu.py, tests/cartpole_mpc_restatement.py).  kernel ==
twin is NOT demanded bit for bit (the device compiler contracts and orders
operations in its own way): both stand under the same arbiter.  Every test
launches once; none repeats a failing launch."""
import functools

import numpy as np
import pytest
import torch

import cartpole_mpc_restatement as R
from conftest import assert_no_worse_than_fp32, load_golden
from test_cartpole_mpc_cpu import check_balance, check_solve, check_swingup, clamp_is_exercised

pytestmark = pytest.mark.gpu
DT = 0.05
F64, F32 = torch.float64, torch.float32
N = R.to_numpy
ITERS = (1, 10, 20)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def nominal():
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    return CartpoleDynamics().params


@functools.lru_cache(maxsize=None)
def large_case(dtype, B=65536 + 7):
    s0, parts = R.thirds(B)
    return s0, parts, R.solve_snapshots(dtype, s0, torch.zeros(B, R.H, 1), DT, ITERS)


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("B", [256, 65536 + 7])
def test_solve_kernel_under_the_fp64_arbiter(dev, B, iters):
    """The thirds of test_solve_twin_under_the_fp64_arbiter at B = 256 and with
    a ragged tail wave (B = 65 543); one restated run of 20 iterations per dtype
    serves the three iteration counts."""
    from apg_trajectory_tracking_amd import functional as F
    case = R.solve_case if B == 256 else large_case
    s0, parts, f64 = case(F64)
    _, _, f32 = case(F32)
    if iters == 20:
        clamp_is_exercised(f64[20]["u"][parts[1]])
    got = F.cartpole_mpc_solve(s0.to(dev), DT, nominal(), iters=iters, want_trace=True)
    check_solve(got, f32[iters], f64[iters], f"kernel B={B} iters={iters}")
    # u0 = None is u0 = 0, and the caller's start tensor is left alone
    if B == 256 and iters == 10:
        u0 = torch.zeros(B, R.H, 1, device=dev)
        again = F.cartpole_mpc_solve(s0.to(dev), DT, nominal(), u0=u0)
        assert torch.equal(again["u"], got["u"]) and again["trace"] is None
        assert torch.equal(again["cost"], got["cost"])
        assert float(u0.abs().max()) == 0.0
        plan = got["u"].clone()
        warm = F.cartpole_mpc_solve(s0.to(dev), DT, nominal(), u0=plan, iters=3)
        assert torch.equal(plan, got["u"]) and not torch.equal(warm["u"], plan)


def _loop_on_device(dev, s0, mode, steps, burn_in, plant_params=None):
    from apg_trajectory_tracking_amd import functional as F
    out = F.cartpole_mpc_closed_loop(
        s0.to(dev), DT, R.params(plant_params), model_params=nominal(), max_steps=steps,
        mode=mode, thresh_div=0.21, burn_in=burn_in, want_trajectory=True, iters=10)
    return R.from_device_layout(out)


def test_balance_loop_kernel_vs_the_restated_loop(dev):
    """As test_balance_loop_twin_vs_the_restated_loop, the kernel in the twin's place."""
    s0, _ = R.balance_case(F64, False)
    check_balance(_loop_on_device(dev, s0, "balance", 60, 0), False, "kernel nominal")


def test_balance_loop_kernel_model_mismatch(dev):
    """As test_balance_loop_twin_model_mismatch: plant masspole 0.2 / length 0.7,
    model nominal."""
    s0, _ = R.balance_case(F64, True)
    check_balance(_loop_on_device(dev, s0, "balance", 60, 0, R.MISMATCH), True,
                  "kernel mismatch")


def test_swingup_loop_kernel_vs_the_restated_loop(dev):
    """As test_swingup_loop_twin_vs_the_restated_loop, the kernel in the twin's place."""
    s0, _ = R.swingup_case(F64)
    check_swingup(_loop_on_device(dev, s0, "swingup", 30, 10), "kernel")


def test_large_balance_batch_vs_the_restated_loop(dev):
    """B = 65 536 + 37 balance flights (many workgroups, a ragged last wave, waves
    that leave early) for 20 steps against the float32 restatement on a strided
    subset of 512.  Near-upright starts, every fourth one unrecoverable
    (R.balance_starts); the 1e-4 parity bar per column, as
    test_large_random_swingup_batch_vs_cpu_restatement has it."""
    B, T = 65536 + 37, 20
    s0 = R.balance_starts(64, seed=31).repeat(B // 64 + 1, 1)[:B].clone()
    gen = torch.Generator().manual_seed(32)
    s0[:, 1] += 0.05 * torch.randn(B, generator=gen)      # no two flights alike
    out = _loop_on_device(dev, s0, "balance", T, 0)
    idx = torch.from_numpy(np.unique(np.concatenate(
        [np.arange(0, B, 138), np.arange(B - 37, B)])))
    assert len(idx) >= 512
    ref = R.closed_loop(F32, s0[idx], DT, 10, T, "balance", 0.21, 0)
    assert ref["margin"] > 1e-3
    assert 0 < int((ref["steps"] < T).sum()) < len(idx)
    assert torch.equal(out["steps"][idx], ref["steps"])
    assert torch.equal(out["upright"][idx], ref["upright"])
    got, want = N(out["states"][idx]), N(ref["states"])
    scale = np.abs(want).max((0, 1))
    err = np.abs(got - want).max((0, 1))
    print("large balance batch: column errors", err, "scales", scale)
    assert np.all(err <= 1e-4 * scale + 1e-6), (err, scale)
    np.testing.assert_allclose(N(out["vel_sum"][idx]), N(ref["vel_sum"]), rtol=1e-4, atol=1e-5)
    # every flight of the batch was flown: steps in [1, T], stopped ones not upright
    assert int(out["steps"].min()) >= 1 and int(out["steps"].max()) == T
    assert bool((out["steps"][out["upright"]] == T).all())


def _restated_statistics(starts, mode, steps, burn_in, thresh_div):
    ref = R.closed_loop(F64, torch.from_numpy(starts), DT, 10, steps, mode, thresh_div, burn_in)
    if mode == "swingup":
        n = len(starts) * max(steps - burn_in - 1, 0)
        mean = float(ref["vel_sum"].sum()) / n
        return {"mean_vel": mean, "std_vel": mean}
    st = N(ref["steps"])
    n = st.sum()
    mean = float(ref["vel_sum"].sum()) / n
    var = float(ref["vel_sq"].sum()) / n - mean**2
    return {"mean_vel": mean, "std_vel": float(np.sqrt(max(var, 0.0))),
            "mean_stable": float(np.mean(st - 1)), "std_stable": float(np.std(st - 1))}


def test_evaluator_flies_the_mpc_and_reports_its_statistics(dev):
    """`Evaluator(MPC(horizon=10, dt=0.05, dynamics="cartpole"), CartPoleEnv(
    CartpoleDynamics(), 0.05, thresh_div=0.3))` with initialize_straight = 0:
    the four statistics of evaluate_in_environment(64, 60) and the two of
    evaluate_swingup(64, 30, burn_in 10) equal those computed from the float64
    restatement on the same drawn starts; the numpy stream is left where the
    network controller's evaluator leaves it."""
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.evaluate_cartpole import (CartPoleEnv, CartpoleWrapper,
                                                               Evaluator)
    from test_cartpole_eval_cpu import golden_net
    np.random.seed(1)
    env = CartPoleEnv(CartpoleDynamics(), DT, thresh_div=0.3)
    ev = Evaluator(MPC(horizon=10, dt=DT, dynamics="cartpole"), env)
    ev.initialize_straight = 0
    net_ev = Evaluator(CartpoleWrapper(golden_net(None, "shipped").to(dev)), env)
    net_ev.initialize_straight = 0

    np.random.seed(7)
    starts = ev.balance_starts(64)
    np.random.seed(7)
    got = ev.evaluate_in_environment(nr_iters=64, max_steps=60)
    after = np.random.rand()
    np.random.seed(7)
    net_ev.evaluate_in_environment(nr_iters=64, max_steps=60)
    assert np.random.rand() == after
    want = _restated_statistics(starts, "balance", 60, 0, 0.3)
    print("evaluate_in_environment:", got, "restatement:", want)
    assert set(got) == set(want)
    for k in want:
        assert np.isclose(got[k], want[k], rtol=1e-3), (k, got, want)
    assert ev.last_flights["cost"].shape == (60, 64)

    np.random.seed(8)
    starts = ev.swingup_starts(64)
    np.random.seed(8)
    got = ev.evaluate_swingup(nr_iters=64, max_steps=30, burn_in_steps=10)
    after = np.random.rand()
    np.random.seed(8)
    net_ev.evaluate_swingup(nr_iters=64, max_steps=30, burn_in_steps=10)
    assert np.random.rand() == after
    want = _restated_statistics(starts, "swingup", 30, 10, 0.3)
    print("evaluate_swingup:", got, "restatement:", want)
    for k in want:
        assert np.isclose(got[k], want[k], rtol=1e-3), (k, got, want)


def learnt_starts():
    return R.balance_starts(64, seed=41)


def test_evaluator_flies_the_mpc_through_the_learnt_simulator(dev):
    """Plant = LearntCartpoleDynamics (the fitted module of
    tests/golden/cartpole_learnt.npz: physics on its six live parameters plus
    the residual), model = the MPC's nominal parameters; balance, 64 flights,
    40 steps, against the restated loop with the learnt plant restated on the
    oracle (R.LearntPlant), float32.  Acceptance as the quadrotor's learnt-plant
    test: `steps` equal on >= 97 % of the flights, states within 2e-3 on all
    but 3 % of those.  Checked on the CPU for these starts: the float32
    restatement against the float64 one has `steps` equal on 100 % of the
    flights and 0 % of them beyond 2e-3 (largest state difference 3.4e-7; half
    of the flights stop early, |theta| never within 9.9e-4 of thresh_div)."""
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.evaluate_cartpole import CartPoleEnv, Evaluator
    from test_cartpole_learnt_cpu import fitted, g20
    m = fitted(g20())
    s0, T = learnt_starts(), 40
    ref = R.closed_loop(F32, s0, DT, 10, T, "balance", 0.21, 0, plant=R.LearntPlant(m, F32))
    np.random.seed(2)
    env = CartPoleEnv(m.to(dev), DT, thresh_div=0.21)
    ev = Evaluator(MPC(horizon=10, dt=DT, dynamics="cartpole"), env)
    with torch.no_grad():
        out = R.from_device_layout(ev._fly(s0.numpy(), T, "balance", 0))
    B = s0.shape[0]
    same = out["steps"] == ref["steps"]
    print("learnt plant: steps equal on %d of %d flights, mean steps %.1f"
          % (int(same.sum()), B, float(ref["steps"].float().mean())))
    assert int(same.sum()) >= 0.97 * B
    d = (out["states"].double() - ref["states"].double()).abs().amax((1, 2))
    bad = int((d[same] > 2e-3).sum())
    print("learnt plant: beyond 2e-3: %d, largest difference %.3e" % (bad, float(d[same].max())))
    assert bad <= 0.03 * int(same.sum())
    # the residual is in the loop: the analytic plant on the module's start
    # parameters flies another path
    nominal_path = _loop_on_device(dev, s0, "balance", T, 0)
    assert float((nominal_path["states"] - out["states"]).abs().max()) > 1e-3


def test_optimality_gap_of_the_shipped_controller(dev):
    """functional.cartpole_policy_optimality_gap on the shipped cart-pole
    controller, B = 512 near-upright starts, 50 iterations: a descent method
    started at the policy's own plan ends at or below the policy's cost.  Heavy
    ball is not monotone per iteration, so a few trajectories may end above: as
    many as the float64 restatement itself shows from the same plans, no more.
    "Above" is judged beyond 1e-6 relative (float32's rounding of the two
    costs)."""
    from apg_trajectory_tracking_amd import functional as F
    from test_cartpole_eval_cpu import golden_net
    net = golden_net(None, "shipped").to(dev).eval()
    B, iters = 512, 50
    s0 = R.near_upright(B, torch.Generator().manual_seed(13)).float()
    before = s0.clone()
    gap = F.cartpole_policy_optimality_gap(net, s0.to(dev), DT, nominal(), iters=iters)
    assert torch.equal(s0, before)
    acts = gap["actions"].cpu()
    assert acts.shape == (B, R.H, 1) and float(acts.abs().max()) <= 1
    pol, warm, cold = N(gap["policy"]), N(gap["mpc_from_policy"]), N(gap["mpc"])
    r64 = R.solve(F64, s0, acts, DT, iters)
    pol64, warm64 = N(r64["trace"][0]), N(r64["cost"])
    assert np.abs(pol - pol64).max() <= 1e-4 * pol64.max()
    above64 = int((warm64 > pol64 * (1 + 1e-6)).sum())
    above = int((warm > pol * (1 + 1e-6)).sum())
    print("optimality gap: mean policy cost %.4f, MPC from the policy %.4f, MPC from 0 %.4f; "
          "above the policy: %d (float64 restatement: %d)"
          % (pol.mean(), warm.mean(), cold.mean(), above, above64))
    assert warm.mean() < pol.mean()
    assert above <= above64
