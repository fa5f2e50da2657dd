"""The batched cart-pole shooting MPC (include/apg.h: apg_cartpole_mpc_solve,
apg_cartpole_mpc_closed_loop) through its host twins (include/apg_cpu_mpc.h) -
the per-lane solver of csrc/cartpole_mpc_math.h compiled for the CPU - against
the float64 restatement of the algorithm in tests/cartpole_mpc_restatement.py
(model: oracle.torch_port.CartpoleOracle with the unwrapped angle, cost:
torch_port.cartpole_loss_mpc, gradient: torch autograd), with the float32
restatement as the yardstick for rounding (conftest.assert_no_worse_than_fp32,
its defaults).  Runs without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cartpole_mpc_restatement as R
import kernel_names
from conftest import assert_no_worse_than_fp32

DT = 0.05
F64, F32 = torch.float64, torch.float32
N = R.to_numpy


@pytest.fixture(scope="module")
def tw():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        from apg_trajectory_tracking_amd import build as b
        if not os.path.exists(b.LIB_CPU):
            pytest.fail("libapg_cpu.so is not built and there is no hipcc to build it")
    return R.twins()


def check_solve(got, f32, f64, what):
    """u, cost and every row of the trace under the fp64 arbiter; u in the box"""
    u = N(got["u"])
    assert u.shape == N(f64["u"]).shape
    assert u.min() >= -1.0 and u.max() <= 1.0
    assert_no_worse_than_fp32(u, N(f32["u"]), N(f64["u"]), what + " u")
    assert_no_worse_than_fp32(N(got["cost"])[:, None], N(f32["cost"])[:, None],
                              N(f64["cost"])[:, None], what + " cost")
    for i in range(f64["trace"].shape[0]):
        assert_no_worse_than_fp32(N(got["trace"][i])[:, None], N(f32["trace"][i])[:, None],
                                  N(f64["trace"][i])[:, None], f"{what} trace[{i}]")
    # the last row of the trace IS the returned cost
    assert np.array_equal(N(got["trace"][-1]), N(got["cost"]))


def clamp_is_exercised(u64_full_range):
    """Between 10 % and 90 % of the unknowns of the full-range third sit on a
    bound in the float64 restatement after 20 iterations (measured: 17.5 %; at
    10 iterations only 9.2 %); otherwise the inputs do not test the projection
    and the test is void."""
    on_bound = float(((u64_full_range <= -1.0) | (u64_full_range >= 1.0)).double().mean())
    print("full-range unknowns on a bound:", on_bound)
    assert 0.10 < on_bound < 0.90, on_bound


@pytest.mark.parametrize("iters", [1, 10, 20])
def test_solve_twin_under_the_fp64_arbiter(tw, iters):
    """B = 256 starts in thirds - near-upright, full range U(-1,1) [2.4, 7.5,
    pi, 7.5], swing-up as _reset_swingup draws them - from u = 0, H = 10.
    Measured (worst trajectory, relative to its own scale): u twin 2.0e-6 /
    float32 restatement 9.3e-7 at 20 iterations, cost 9.9e-7 / 4.7e-7."""
    s0, parts, f64 = R.solve_case(F64)
    _, _, f32 = R.solve_case(F32)
    if iters == 20:
        clamp_is_exercised(f64[20]["u"][parts[1]])
    check_solve(R.twin_solve(tw, s0, None, DT, iters), f32[iters], f64[iters],
                f"twin iters={iters}")


def test_the_rule_optimises():
    """Float64 restatement, B = 512 per draw.  Near-upright: the mean cost after
    10 iterations is below 0.2 x the start (measured 0.070).  Near-upright, full
    range and swing-up: no trajectory's cost after 20 iterations is above its
    start cost (measured 0 of 512 each).  The twin inherits both through
    test_solve_twin_under_the_fp64_arbiter."""
    gen = torch.Generator().manual_seed(23)
    for name, draw in (("near-upright", R.near_upright), ("full range", R.full_range),
                       ("swing-up", R.swingup)):
        s0 = draw(512, gen).float()
        tr = R.solve(F64, s0, torch.zeros(512, R.H, 1), DT, 20)["trace"]
        above = int((tr[20] > tr[0]).sum())
        print("%s: mean cost start %.3f, 10 iterations %.3f, 20 iterations %.3f; above the "
              "start: %d" % (name, float(tr[0].mean()), float(tr[10].mean()),
                             float(tr[20].mean()), above))
        if name == "near-upright":
            assert float(tr[10].mean()) < 0.2 * float(tr[0].mean())
        assert above == 0


def test_first_order_optimality_after_200_iterations(tw):
    """Norm of the projected float64 gradient (components that point out of
    the box at an active bound removed) after 200 iterations, relative to its
    value at u = 0, over the 256 starts of the solve test.  Measured:
    restatement 2.72e-3, twin 2.72e-3 (the near-upright third alone: 8.2e-4
    both); the twin is held to 2 x the restatement's value."""
    s0, _, _ = R.solve_case(F64)
    z = torch.zeros(s0.shape[0], R.H, 1)
    g0 = R.projected_gradient_norm(s0, z, DT)
    r64 = R.projected_gradient_norm(s0, R.solve(F64, s0, z, DT, 200)["u"], DT) / g0
    rtw = R.projected_gradient_norm(s0, R.twin_solve(tw, s0, None, DT, 200)["u"], DT) / g0
    print("projected gradient / start: restatement %.3e, twin %.3e" % (r64, rtw))
    assert r64 < 1.0
    assert rtw <= 2.0 * r64


def test_the_model_is_the_unwrapped_one(tw):
    """theta = 3.1, theta_dot = 2: the angle crosses pi inside the horizon.  The
    twin's cost at u = 0 is the unwrapped restatement's (measured 497.37) and
    far from the wrapped one's (2039.17)."""
    s = torch.tensor([[0.0, 0.0, 3.1, 2.0]])
    z = torch.zeros(1, R.H, 1)
    got = float(R.twin_solve(tw, s, None, DT, 0)["trace"][0])
    unwrapped = float(R.solve(F64, s, z, DT, 0)["trace"][0])
    wrapped = float(R.solve(F64, s, z, DT, 0, wrapped=True)["trace"][0])
    print("cost at u = 0: twin %.4f, unwrapped %.4f, wrapped %.4f" % (got, unwrapped, wrapped))
    assert abs(got - unwrapped) <= 1e-5 * unwrapped
    assert abs(got - wrapped) > 1.0


def _short_loop(tw, steps=3):
    s0 = R.balance_starts(16, seed=9)[4:]     # the near-upright ones
    return s0, R.twin_closed_loop(tw, s0, DT, 10, steps, "swingup", 0.21, 0)


def test_warm_start_solve_shift_solve_is_the_closed_loops_second_step(tw):
    s0, loop = _short_loop(tw)
    first = R.twin_solve(tw, s0, None, DT, 10)
    assert np.abs(N(first["u"][:, 0, 0]) - N(loop["actions"][:, 0])).max() <= 1e-6
    s1 = loop["states"][:, 0]
    second = R.twin_solve(tw, s1, R.shift(first["u"]), DT, 10)
    assert np.abs(N(second["u"][:, 0, 0]) - N(loop["actions"][:, 1])).max() <= 1e-6
    assert np.abs(N(second["cost"]) - N(loop["cost"][:, 1])).max() <= 1e-5 * N(second["cost"]).max()
    # and the warm start matters: from u = 0 the second solve ends elsewhere
    cold = R.twin_solve(tw, s1, None, DT, 10)
    assert np.abs(N(cold["u"][:, 0, 0]) - N(loop["actions"][:, 1])).max() > 1e-4


def check_balance(got, mismatch, what):
    """`got` ([B, ...] as the restatement lays it out) against the float64
    restatement of the whole loop; the float32 restatement as yardstick."""
    _, f64 = R.balance_case(F64, mismatch)
    _, f32 = R.balance_case(F32, mismatch)
    steps = f64["steps"]
    early, full = float((steps < 60).double().mean()), float((steps == 60).double().mean())
    print(what, "float64 restatement: stop early %.3f, run to the end %.3f, smallest distance "
          "of |theta| to thresh_div %.4f" % (early, full, f64["margin"]))
    # void unless no flight grazes the threshold and both outcomes occur
    assert f64["margin"] > 1e-3
    assert early >= 0.10 and full >= 0.50
    same_balance_flights(got, f32, f64, what)
    return f64


def same_balance_flights(got, f32, f64, what):
    """Every output of a balance loop, by name, against its restatement."""
    assert torch.equal(got["steps"], f64["steps"])
    assert torch.equal(got["upright"], f64["upright"])
    for k in ("states", "actions", "cost"):
        assert_no_worse_than_fp32(N(got[k]), N(f32[k]), N(f64[k]), f"{what} {k}")
    np.testing.assert_allclose(N(got["vel_sum"]), N(f64["vel_sum"]), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(N(got["vel_sq"]), N(f64["vel_sq"]), rtol=1e-4, atol=1e-5)


def test_balance_loop_twin_vs_the_restated_loop(tw):
    """64 flights, 60 steps, thresh_div 0.21, 10 iterations: 48 near-upright
    starts and 16 at theta = +-0.19 with theta_dot = +-3 outwards, which no
    controller recovers.  Measured in the float64 restatement: 25 % stop early,
    75 % run to the end, |theta| never within 0.103 of thresh_div."""
    s0, _ = R.balance_case(F64, False)
    check_balance(R.twin_closed_loop(tw, s0, DT, 10, 60, "balance", 0.21, 0), False,
                  "twin nominal")


def test_balance_loop_twin_model_mismatch(tw):
    """Plant {"masspole": 0.2, "length": 0.7}, model nominal (measured: smallest
    distance to thresh_div 0.098).  Swapped roles fly another path: `model` and
    `plant` are neither swapped nor aliased."""
    s0, _ = R.balance_case(F64, True)
    got = R.twin_closed_loop(tw, s0, DT, 10, 60, "balance", 0.21, 0, plant_params=R.MISMATCH)
    check_balance(got, True, "twin mismatch")
    swapped = R.twin_closed_loop(tw, s0, DT, 10, 60, "balance", 0.21, 0,
                                 model_params=R.MISMATCH)
    assert np.abs(N(swapped["states"]) - N(got["states"])).max() > 1e-3


def test_every_field_of_the_flight_struct_is_the_one_it_is_named(tw):
    """ApgCartpoleFlight through the twin on the smallest case whose outputs all
    differ from each other: B = 3, H = 5, T = 4, balance; flight 0 starts beyond
    thresh_div (one step, not upright), flight 1 at theta = 0.19 falling outwards
    (stops early), flight 2 stays up - so steps = (1, <4, 4) is not upright = (0,
    0, 1), and with |x_dot| away from 0 and 1 vel_sum is not vel_sq.  Each output
    is held by name against the float64 restatement at the tolerances of the
    balance tests above; a same-typed neighbour swapped in the struct, in the
    ctypes mirror or in a forwarding layer fails one of them.  Flown again with
    states / actions NULL, the other outputs keep their bits."""
    s0 = torch.tensor([[0.1, 0.4, 0.30, 0.2],
                       [-0.2, -0.5, 0.19, 3.0],
                       [0.05, 0.3, 0.02, -0.1]])
    flown = dict(iters=10, max_steps=4, mode="balance", thresh_div=0.21, burn_in=0, horizon=5)
    f64, f32 = (R.closed_loop(dt, s0, DT, **flown) for dt in (F64, F32))
    print("float64 restatement: steps", f64["steps"].tolist(), "upright",
          f64["upright"].tolist(), "margin %.4f" % f64["margin"])
    assert f64["margin"] > 1e-3                     # clear of thresh_div
    assert f64["steps"][0] == 1 and f64["steps"][1] < 4 and f64["steps"][2] == 4
    assert f64["upright"].tolist() == [False, False, True]
    got = R.twin_closed_loop(tw, s0, DT, **flown)
    same_balance_flights(got, f32, f64, "flight struct")
    assert not np.allclose(N(got["vel_sum"]), N(got["vel_sq"]), rtol=1e-2)
    bare = R.twin_closed_loop(tw, s0, DT, want_trajectory=False, **flown)
    for k in ("steps", "upright", "vel_sum", "vel_sq", "cost"):
        assert torch.equal(bare[k], got[k]), k
    assert not bare["states"].any() and not bare["actions"].any()


def check_swingup(got, what):
    """At most 3 % of the flights differ from the float64 restatement by more
    than 2e-3 in any state (a flight sitting exactly on the wrap may take the
    other branch: a condition, not a tolerance); `upright` equal on the others."""
    _, f64 = R.swingup_case(F64)
    wraps = float(f64["wraps"].double().mean())
    print(what, "float64 restatement: flights that wrap at least once %.3f" % wraps)
    assert wraps >= 0.50
    assert (got["steps"] == 30).all()
    d = (got["states"].double() - f64["states"]).abs().amax((1, 2))
    beyond = d > 2e-3
    print(what, "beyond 2e-3: %.4f of the flights, largest difference %.3e"
          % (float(beyond.double().mean()), float(d.max())))
    assert float(beyond.double().mean()) <= 0.03
    assert torch.equal(got["upright"][~beyond], f64["upright"][~beyond])
    return f64


def test_swingup_loop_twin_vs_the_restated_loop(tw):
    """256 swing-up starts, 30 steps, burn_in 10.  Measured: 95 % of the flights
    wrap within 30 steps; twin 0 % beyond 2e-3 (largest 5.5e-4), float32
    restatement 0 % (3.1e-4)."""
    s0, _ = R.swingup_case(F64)
    got = R.twin_closed_loop(tw, s0, DT, 10, 30, "swingup", 0.21, 10)
    check_swingup(got, "twin")


def _twin_behind_functional(tw, monkeypatch):
    """functional.cartpole_mpc_solve on CPU tensors: the host twin behind the
    same signature (tests only - the package itself never loads the twins)."""
    from apg_trajectory_tracking_amd import functional as F

    def stand_in(state0, dt, params, u0=None, horizon=10, iters=None, beta=None, alpha=None,
                 want_trace=False):
        if state0.dim() != 2 or state0.shape[1] != 4:
            raise ValueError("state0 [B,4] expected")
        return R.twin_solve(tw, state0, u0, dt, 10 if iters is None else iters,
                            horizon=horizon)
    monkeypatch.setattr(F, "cartpole_mpc_solve", stand_in)


def test_mpc_object_surface_and_warm_start(tw, monkeypatch):
    """`MPC(dynamics="cartpole").predict_actions(state)`: [4] numpy -> [1,1]
    numpy equal to row 0 of the batched call ([B,4] tensor -> [B,1] tensor); the
    warm start lives in the object, is shifted per call (call 2 = the closed
    loop's second action) and dropped by reset(); a wrong shape or horizon is a
    ValueError; the fixed wing is still refused by name."""
    from apg_trajectory_tracking_amd.controllers import MPC
    _twin_behind_functional(tw, monkeypatch)
    s0, loop = _short_loop(tw)
    B = s0.shape[0]
    batched = MPC(horizon=10, dt=DT, dynamics="cartpole", device="cpu")
    a = batched.predict_actions(s0)
    assert torch.is_tensor(a) and a.shape == (B, 1)
    assert batched.warm_start.shape == (B, 10, 1)
    single = MPC(horizon=10, dt=DT, dynamics="cartpole", device="cpu")
    a0 = single.predict_actions(s0[0].numpy())
    assert isinstance(a0, np.ndarray) and a0.shape == (1, 1)
    assert np.array_equal(a0[0], a[0].numpy())
    a2 = batched.predict_actions(loop["states"][:, 0])
    assert np.abs(N(a2[:, 0]) - N(loop["actions"][:, 1])).max() <= 1e-6
    batched.reset()
    assert batched.warm_start is None
    again = batched.predict_actions(s0)
    assert torch.equal(again, a)
    five = MPC(horizon=5, dt=DT, dynamics="cartpole", device="cpu")
    assert five.predict_actions(s0).shape == (B, 1) and five.warm_start.shape == (B, 5, 1)
    mod = MPC(horizon=10, dt=DT, dynamics="cartpole", modified_params=R.MISMATCH)
    assert mod.params.masspole == pytest.approx(0.2) and mod.params.length == pytest.approx(0.7)
    with pytest.raises(NotImplementedError, match="flightmare"):
        MPC(dynamics="fixed_wing")
    with pytest.raises(ValueError):
        MPC(horizon=7, dynamics="cartpole")
    with pytest.raises(ValueError):
        single.predict_actions(np.zeros(5))


def test_evaluator_routes_an_mpc_controller_to_the_mpc_closed_loop(tw, monkeypatch):
    """Evaluator's host logic with an MPC controller (no GPU: the host twin
    stands behind functional.cartpole_mpc_closed_loop): plant = the
    environment's parameters, model = the MPC's own; the draws, the returned
    dicts and return_success are the network controller's."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.evaluate_cartpole import CartPoleEnv, Evaluator
    seen = {}

    def stand_in(state0, dt, params, model_params=None, learnt=None, max_steps=250,
                 mode="balance", thresh_div=0.21, burn_in=50, want_trajectory=False,
                 **options):
        seen.update(plant=params.masspole, model=model_params.masspole, learnt=learnt,
                    options=options, starts=state0.clone())
        o = R.twin_closed_loop(tw, state0, dt, options["iters"], max_steps, mode, thresh_div,
                               burn_in, plant_params=R.MISMATCH, horizon=options["horizon"])
        return dict(steps=o["steps"].to(torch.int32), upright=o["upright"].to(torch.int32),
                    vel_sum=o["vel_sum"], vel_sq=o["vel_sq"], cost=o["cost"].t().contiguous(),
                    states=o["states"].permute(1, 2, 0).contiguous(),
                    actions=o["actions"].t().contiguous())
    monkeypatch.setattr(F, "cartpole_mpc_closed_loop", stand_in)
    np.random.seed(3)
    env = CartPoleEnv(CartpoleDynamics(R.MISMATCH), DT, thresh_div=0.3)
    ev = Evaluator(MPC(horizon=5, dt=DT, dynamics="cartpole", iters=4, device="cpu"), env)
    ev.initialize_straight = 0
    np.random.seed(4)
    res = ev.evaluate_in_environment(nr_iters=6, max_steps=12)
    after = np.random.rand()
    assert set(res) == {"mean_vel", "std_vel", "mean_stable", "std_stable"}
    assert seen["plant"] == pytest.approx(0.2) and seen["model"] == pytest.approx(0.1)
    assert seen["learnt"] is None
    assert seen["options"] == dict(horizon=5, iters=4, beta=None, alpha=None)
    assert ev.last_flights["cost"].shape == (12, 6)
    # the same draws, and the stream left where the network controller leaves it
    np.random.seed(4)
    starts = ev.balance_starts(6)
    assert np.random.rand() == after
    assert np.array_equal(starts, seen["starts"].numpy())
    success, velocities = ev.evaluate_in_environment(nr_iters=6, max_steps=12,
                                                     return_success=1)
    assert len(success) == 6 and len(velocities) == int(success.sum() + 6)
    sw = ev.evaluate_swingup(nr_iters=5, max_steps=8, burn_in_steps=2)
    assert set(sw) == {"mean_vel", "std_vel"} and env.state.shape == (4,)
    with pytest.raises(ValueError, match="dt"):
        Evaluator(MPC(horizon=10, dt=0.1, dynamics="cartpole", device="cpu"),
                  env).evaluate_swingup(nr_iters=1, max_steps=3)


def test_twin_argument_errors_and_abi(tw):
    from apg_trajectory_tracking_amd import _capi
    assert ctypes.sizeof(_capi.ApgCartpoleMpcOptions) == 12
    s0 = R.balance_starts(8)
    s = s0.t().contiguous()
    u, cost = torch.zeros(10, 8), torch.zeros(8)
    p = R.params()

    def call(H=10, opt=None, out=u):
        o = opt or R.options(1)
        return tw.apg_cartpole_mpc_solve_cpu(
            s.data_ptr(), None, DT, ctypes.byref(p), ctypes.byref(o), 8, H,
            None if out is None else out.data_ptr(), cost.data_ptr(), None)
    assert call() == 0
    assert call(out=None) == 0                      # NULL outputs drop their writes
    assert call(H=7) == -1 and b"H must be 5 or 10" in tw.apg_cpu_last_error_string()
    assert call(opt=_capi.ApgCartpoleMpcOptions(1, 1.5, 5e-4)) == -1
    assert call(opt=_capi.ApgCartpoleMpcOptions(-1, 0.5, 5e-4)) == -1
    assert call(opt=_capi.ApgCartpoleMpcOptions(1, 0.5, 0.0)) == -1


def test_horizon_five(tw):
    """H = 5 comes from the same template."""
    s0, _ = R.thirds(96, seed=2)
    z = torch.zeros(96, 5, 1)
    f64, f32 = R.solve(F64, s0, z, DT, 10), R.solve(F32, s0, z, DT, 10)
    check_solve(R.twin_solve(tw, s0, None, DT, 10, horizon=5), f32, f64, "twin H=5")


def test_kernels_keep_the_solver_in_registers():
    """The build's kernel_resources.json lists the two kernels in every
    instantiation (solve: H = 5, 10; closed loop: H = 5, 10 x analytic / learnt
    plant) without scratch and without spilled VGPRs."""
    res = kernel_names.resources()
    for name, count in (("cart_mpc_solve_kernel", 2), ("cart_mpc_closed_loop_kernel", 4)):
        found = kernel_names.instances(res, name)
        assert len(found) == count, (name, sorted(found))
        for k, v in found.items():
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
