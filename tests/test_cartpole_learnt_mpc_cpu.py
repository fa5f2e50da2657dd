"""The cart-pole shooting MPC that plans through the learnt simulator
(include/apg.h: apg_cartpole_learnt_mpc_solve, apg_cartpole_learnt_mpc_closed_loop)
through its host twins (include/apg_cpu_mpc.h) - the solver of
csrc/cartpole_mpc_math.h on its learnt model (CartMpcLearnt), compiled for the
CPU - against the float64 restatement of tests/cartpole_learnt_mpc_restatement.py
(model: the unwrapped oracle step on the module's six parameters plus the
residual, gradient: torch autograd), the float32 restatement as the yardstick
for rounding (conftest.assert_no_worse_than_fp32, its defaults).  Runs without
a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cartpole_learnt_mpc_restatement as L
import cartpole_mpc_restatement as R
import kernel_names
from test_cartpole_mpc_cpu import check_solve

DT = L.DT
F64, F32 = torch.float64, torch.float32
N = R.to_numpy


@pytest.fixture(scope="module")
def tw():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        from apg_trajectory_tracking_amd import build as b
        if not os.path.exists(b.LIB_CPU):
            pytest.fail("libapg_cpu.so is not built and there is no hipcc to build it")
    return L.twins()


def clamp_is_exercised(u64_full_range):
    """Void unless 10-90 % of the full-range unknowns sit on a bound in the
    float64 restatement after 20 iterations (measured: 21.2 %)."""
    on_bound = float(((u64_full_range <= -1.0) | (u64_full_range >= 1.0)).double().mean())
    print("full-range unknowns on a bound:", on_bound)
    assert 0.10 < on_bound < 0.90, on_bound


# ------------------------------------------------------------------ 1, 2: the solve
@pytest.mark.parametrize("iters", [1, 10, 20])
def test_solve_twin_under_the_fp64_arbiter(tw, iters):
    """The fitted module, R.thirds(256) from u = 0, H = 10: u, cost and every
    trace row.  Measured in the float64 restatement: mean cost near upright
    93.6 -> 5.35 (10 iterations) -> 5.04 (20), full range 1 134.8 -> 613.1 ->
    586.4, swing-up 588.1 -> 393.7 -> 372.9, no trajectory above its start cost.
    Worst error against float64 at 20 iterations: u twin 1.0e-6 / float32
    restatement 9.7e-7, cost (relative) 2.1e-7."""
    s0, parts, f64 = L.solve_case(F64)
    _, _, f32 = L.solve_case(F32)
    if iters == 20:
        clamp_is_exercised(f64[20]["u"][parts[1]])
    tr = f64[iters]["trace"]
    assert int((tr[-1] > tr[0]).sum()) == 0           # the rule descends on this model
    check_solve(L.twin_solve(tw, L.module(), s0, None, DT, iters), f32[iters], f64[iters],
                f"twin iters={iters}")


def test_horizon_five(tw):
    """H = 5 comes from the same template: 96 starts, 10 iterations."""
    s0, _, f64 = L.solve_case(F64, 96, 5, 2)
    _, _, f32 = L.solve_case(F32, 96, 5, 2)
    check_solve(L.twin_solve(tw, L.module(), s0, None, DT, 10, horizon=5), f32[10], f64[10],
                "twin H=5")


# ------------------------------------------------------------- 3: the zero residual
def zero_residual_is_the_analytic_solver(learnt_solve, analytic_solve):
    """A freshly constructed module with its three residual tensors zeroed: u and
    cost equal the analytic solver's on ApgCartpoleParams of the same six values
    within 1e-6 (cost: relative to the largest)."""
    s0, _ = R.thirds(256)
    got, want = learnt_solve(L.module("zero"), s0), analytic_solve(s0)
    du = np.abs(N(got["u"]) - N(want["u"])).max()
    dc = np.abs(N(got["cost"]) - N(want["cost"])).max() / N(want["cost"]).max()
    print("zero residual against the analytic solver: u %.3e, cost %.3e (relative)" % (du, dc))
    assert du <= 1e-6 and dc <= 1e-6


def test_a_zero_residual_is_the_analytic_solver(tw):
    m = L.module("zero")
    p = R.params()
    for k, want in (("max_force_mag", p.max_force_mag), ("masspole", p.masspole),
                    ("length", p.length), ("friction", p.friction),
                    ("total_mass", p.masspole + p.masscart),
                    ("polemass_length", p.masspole * p.length)):
        assert float(m.cfg[k].detach()) == pytest.approx(want, rel=1e-6), k
    zero_residual_is_the_analytic_solver(
        lambda mod, s0: L.twin_solve(tw, mod, s0, None, DT, 10),
        lambda s0: R.twin_solve(tw, s0, None, DT, 10))


# ------------------------------------------------- 4: unwrapped, residual on theta
def test_the_model_is_the_unwrapped_one_and_the_residual_reaches_theta(tw):
    """s = [0, 0, 3.1, 2], u = 0, iters 0: the angle crosses pi inside the
    horizon.  The twin's cost is the restatement's (measured 869.32), more than
    1.0 from the cost with the wrapped step (2 024.37), and apart from the
    restatement WITHOUT the residual's theta row (536.75: a gap of 332.6,
    asserted: a tenth of it, far above float32's rounding of a cost of 870:
    5e-5)."""
    s = torch.tensor([[0.0, 0.0, 3.1, 2.0]])
    z = torch.zeros(1, L.H, 1)
    m = L.module()
    got = float(L.twin_solve(tw, m, s, None, DT, 0)["trace"][0])
    want = float(L.cost(L.LearntModel(m, F64), s.double(), z.double(), DT))
    wrapped = float(L.cost(L.LearntModel(m, F64, wrapped=True), s.double(), z.double(), DT))
    no_row = float(L.cost(L.LearntModel(m, F64, theta_row=False), s.double(), z.double(), DT))
    print("cost at u = 0: twin %.5f, restatement %.5f, wrapped %.3f, without the residual's "
          "theta row %.5f" % (got, want, wrapped, no_row))
    assert abs(got - want) <= 1e-5 * want
    assert abs(got - wrapped) > 1.0
    gap = abs(want - no_row)
    assert gap > 100 * 6e-8 * want          # the row matters beyond float32 rounding
    assert abs(got - no_row) > 0.1 * gap


# ------------------------------------------------------------- 5, 6, 7: the loops
def check_learnt_loop(got, what):
    """`got`: plant and model both the fitted module, the 64 starts of the
    existing learnt-plant test, 40 steps, thresh_div 0.21, 10 iterations.  The
    reference itself meets the conditions: float32 against float64 has `steps`
    equal on 64 of 64 flights, largest state difference 6.3e-5, margin 0.0496."""
    f64 = L.loop_case(F64)
    early = int((f64["steps"] < L.LOOP_STEPS).sum())
    print(what, "float64 restatement: %d flights stop early, smallest distance of |theta| to "
          "thresh_div %.4f" % (early, f64["margin"]))
    assert f64["margin"] > 1e-3
    assert 0 < early < 64
    L.same_flights(got, L.loop_case(F32), what)


def test_balance_loop_twin_on_the_learnt_plant_with_the_learnt_model(tw):
    m = L.module()
    check_learnt_loop(L.twin_closed_loop(tw, L.loop_starts(), DT, 10, L.LOOP_STEPS, m, plant=m),
                      "twin")


def test_planning_with_the_adapted_model_pays(tw):
    """Both arms from the twins on the learnt plant; the nominal arm's `steps`
    are not compared elementwise (it grazes the threshold at 0.0010)."""
    m = L.module()
    learnt = L.twin_closed_loop(tw, L.loop_starts(), DT, 10, L.LOOP_STEPS, m, plant=m)
    nominal = L.twin_closed_loop(tw, L.loop_starts(), DT, 10, L.LOOP_STEPS, None, plant=m)
    L.pays(learnt, nominal, "twins")
    assert float((learnt["states"] - nominal["states"]).abs().max()) > 0.1


def neither_swapped_nor_aliased(fly):
    """fly(model, plant): model = fitted with plant = second (length 0.7, the
    residual halved) flies another path than the roles swapped, and than either
    module in both roles."""
    a, b = L.module(), L.module("second")
    ab, ba = fly(a, b)["states"], fly(b, a)["states"]
    d = float((ab - ba).abs().max())
    print("model/plant swapped: largest state difference %.4f" % d)
    assert d > 1e-3
    assert float((ab - fly(a, a)["states"]).abs().max()) > 1e-3
    assert float((ab - fly(b, b)["states"]).abs().max()) > 1e-3


def test_model_and_plant_are_neither_swapped_nor_aliased(tw):
    s0 = L.loop_starts()[16:32]
    neither_swapped_nor_aliased(
        lambda model, plant: L.twin_closed_loop(tw, s0, DT, 10, 12, model, plant=plant))
    # and an analytic plant under the learnt model is flown as such
    m = L.module()
    analytic = L.twin_closed_loop(tw, s0, DT, 10, 12, m, plant=None)
    learnt = L.twin_closed_loop(tw, s0, DT, 10, 12, m, plant=m)
    assert float((analytic["states"] - learnt["states"]).abs().max()) > 1e-3
    first = L.twin_solve(tw, m, s0, None, DT, 10)
    assert np.abs(N(first["u"][:, 0, 0]) - N(analytic["actions"][:, 0])).max() <= 1e-6


# ------------------------------------------------------------ 8: the MPC object
def _twin_behind_functional(tw, monkeypatch):
    """functional.cartpole_mpc_solve on CPU tensors: the host twin behind the
    same signature (tests only - the package itself never loads the twins)."""
    from apg_trajectory_tracking_amd import functional as F

    def stand_in(state0, dt, params, u0=None, horizon=10, iters=None, beta=None, alpha=None,
                 want_trace=False, learnt=None):
        assert learnt is not None and params is None
        return L.twin_solve(tw, learnt, state0, u0, dt, 10 if iters is None else iters,
                            horizon=horizon)
    monkeypatch.setattr(F, "cartpole_mpc_solve", stand_in)


def test_mpc_object_with_a_learnt_model(tw, monkeypatch):
    """`MPC(dynamics="cartpole", learnt_model=m).predict_actions(state)`: numpy
    [4] -> [1,1] equal to row 0 of the batched call; the warm start is shifted
    per call (call 2 = the closed loop's second action) and dropped by reset();
    `params` is None; what cannot be combined is refused."""
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    _twin_behind_functional(tw, monkeypatch)
    m = L.module()
    s0 = L.loop_starts()[16:28]
    loop = L.twin_closed_loop(tw, s0, DT, 10, 3, m, plant=m, mode="swingup")
    B = s0.shape[0]
    batched = MPC(horizon=10, dt=DT, dynamics="cartpole", device="cpu", learnt_model=m)
    assert batched.params is None and batched.learnt_model is m
    a = batched.predict_actions(s0)
    assert torch.is_tensor(a) and a.shape == (B, 1)
    assert batched.warm_start.shape == (B, 10, 1)
    assert np.abs(N(a[:, 0]) - N(loop["actions"][:, 0])).max() <= 1e-6
    single = MPC(horizon=10, dt=DT, dynamics="cartpole", device="cpu", learnt_model=m)
    a0 = single.predict_actions(s0[0].numpy())
    assert isinstance(a0, np.ndarray) and a0.shape == (1, 1)
    assert np.array_equal(a0[0], a[0].numpy())
    a2 = batched.predict_actions(loop["states"][:, 0])
    assert np.abs(N(a2[:, 0]) - N(loop["actions"][:, 1])).max() <= 1e-6
    batched.reset()
    assert batched.warm_start is None
    assert torch.equal(batched.predict_actions(s0), a)
    with pytest.raises(ValueError, match="modified_params"):
        MPC(dynamics="cartpole", dt=DT, learnt_model=m, modified_params={"length": 0.7})
    with pytest.raises(NotImplementedError, match="flightmare"):
        MPC(dynamics="cartpole", dt=DT, learnt_model=LearntDynamics())
    with pytest.raises(NotImplementedError, match="cartpole"):
        MPC(dynamics="flightmare", learnt_model=m)
    plain = MPC(dynamics="cartpole", dt=DT, device="cpu")
    assert plain.learnt_model is None and plain.params is not None


# --------------------------------------------------------- 9: the evaluator's routing
def test_evaluator_routes_a_learnt_model_to_the_new_closed_loop(tw, monkeypatch):
    """Evaluator(MPC(dynamics="cartpole", learnt_model=m), env): `model_learnt`
    is the MPC's module, `learnt` the environment's module or None with
    `params` for an analytic environment; the numpy draw stream is left where
    the network controller's evaluator leaves it (the host twin stands behind
    functional.cartpole_mpc_closed_loop)."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from apg_trajectory_tracking_amd.evaluate_cartpole import CartPoleEnv, Evaluator
    m, other = L.module(), L.module("second")
    seen = {}

    def stand_in(state0, dt, params, model_params=None, learnt=None, max_steps=250,
                 mode="balance", thresh_div=0.21, burn_in=50, want_trajectory=False,
                 model_learnt=None, **options):
        seen.update(params=params, model_params=model_params, learnt=learnt,
                    model_learnt=model_learnt, options=options, starts=state0.clone())
        o = L.twin_closed_loop(tw, state0, dt, options["iters"], max_steps, model_learnt,
                               plant=learnt, plant_params=R.MISMATCH, thresh_div=thresh_div,
                               mode=mode, burn_in=burn_in, horizon=options["horizon"])
        return dict(steps=o["steps"].to(torch.int32), upright=o["upright"].to(torch.int32),
                    vel_sum=o["vel_sum"], vel_sq=o["vel_sq"], cost=o["cost"].t().contiguous(),
                    states=o["states"].permute(1, 2, 0).contiguous(),
                    actions=o["actions"].t().contiguous())
    monkeypatch.setattr(F, "cartpole_mpc_closed_loop", stand_in)
    mpc = MPC(horizon=5, dt=DT, dynamics="cartpole", iters=4, device="cpu", learnt_model=m)
    np.random.seed(3)
    env = CartPoleEnv(CartpoleDynamics(R.MISMATCH), DT, thresh_div=0.3)
    ev = Evaluator(mpc, env)
    ev.initialize_straight = 0
    np.random.seed(4)
    res = ev.evaluate_in_environment(nr_iters=6, max_steps=12)
    after = np.random.rand()
    assert set(res) == {"mean_vel", "std_vel", "mean_stable", "std_stable"}
    assert seen["model_learnt"] is m and seen["learnt"] is None
    assert seen["params"] is env.dynamics.params and seen["model_params"] is None
    assert seen["options"] == dict(horizon=5, iters=4, beta=None, alpha=None)
    assert ev.last_flights["cost"].shape == (12, 6)
    # the same draws, and the stream left where the network controller leaves it
    np.random.seed(4)
    starts = ev.balance_starts(6)
    assert np.random.rand() == after
    assert np.array_equal(starts, seen["starts"].numpy())
    want = L.twin_closed_loop(tw, torch.from_numpy(starts), DT, 4, 12, m,
                              plant_params=R.MISMATCH, thresh_div=0.3, horizon=5)
    assert torch.equal(ev.last_flights["steps"].long(), want["steps"])
    # a learnt environment stays the plant, whichever module it is
    for plant in (m, other):
        ev = Evaluator(mpc, CartPoleEnv(plant, DT, thresh_div=0.3))
        ev.evaluate_in_environment(nr_iters=3, max_steps=4)
        assert seen["learnt"] is plant and seen["params"] is None
        assert seen["model_learnt"] is m


# ------------------------------------------------------------- 10: argument errors
def test_twin_argument_errors(tw):
    from apg_trajectory_tracking_amd import _capi
    s0 = R.balance_starts(8)
    s = s0.t().contiguous()
    u, cost = torch.zeros(10, 8), torch.zeros(8)
    hm = L.HostModel(L.module())
    ok = hm.struct
    err = tw.apg_cpu_last_error_string

    def without(*names):
        kw = {n: getattr(ok, n) for n, _ in _capi.ApgCartpoleLearnt._fields_}
        kw.update({n: None for n in names})
        return _capi.ApgCartpoleLearnt(**kw)

    def call(H=10, opt=None, out=u, model=ok):
        o = opt or R.options(1)
        return tw.apg_cartpole_learnt_mpc_solve_cpu(
            s.data_ptr(), None, DT, None if model is None else ctypes.byref(model),
            ctypes.byref(o), 8, H, None if out is None else out.data_ptr(), cost.data_ptr(),
            None)
    assert call() == 0
    assert call(out=None) == 0                      # NULL outputs drop their writes
    assert call(model=None) == -1 and b"model is NULL" in err()
    assert call(model=without("w1", "b1", "w2")) == -1 and b"w1 / b1 / w2" in err()
    assert call(model=without("b1")) == -1 and b"w1 / b1 / w2" in err()
    assert call(model=without("length")) == -1 and b"physical parameter" in err()
    assert call(H=7) == -1 and b"H must be 5 or 10" in err()
    assert call(opt=_capi.ApgCartpoleMpcOptions(1, 1.5, 5e-4)) == -1
    assert call(opt=_capi.ApgCartpoleMpcOptions(-1, 0.5, 5e-4)) == -1
    assert call(opt=_capi.ApgCartpoleMpcOptions(1, 0.5, 0.0)) == -1

    steps, upright = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    vs, vq = torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    p = R.params()

    def flight(T=3, mode=0, state0=s.data_ptr()):
        return _capi.ApgCartpoleFlight(
            state0=state0, max_steps=T, mode=mode, thresh_div=0.21, burn_in=0,
            steps=steps.data_ptr(), upright=upright.data_ptr(), vel_sum=vs.data_ptr(),
            vel_sq=vq.data_ptr(), states=None, actions=None)

    def loop(H=10, model=ok, plant=p, plant_learnt=None, B=8, T=3, mode=0, opt=None):
        return tw.apg_cartpole_learnt_mpc_closed_loop_cpu(
            ctypes.byref(flight(T, mode)), DT, None if plant is None else ctypes.byref(plant),
            None if plant_learnt is None else ctypes.byref(plant_learnt),
            None if model is None else ctypes.byref(model),
            ctypes.byref(opt or R.options(1)), B, H, None)
    assert loop() == 0 and int(steps.min()) >= 1
    assert loop(plant=None, plant_learnt=ok) == 0
    assert loop(model=None) == -1 and b"model is NULL" in err()
    assert loop(model=without("w1", "b1", "w2")) == -1 and b"w1 / b1 / w2" in err()
    assert loop(H=7) == -1 and b"H must be 5 or 10" in err()
    assert loop(plant=None) == -1 and b"plant is NULL" in err()
    assert loop(plant_learnt=without("w1", "b1", "w2")) == -1 and b"learnt plant" in err()
    assert loop(B=0) == -1 and loop(T=0) == -1 and loop(mode=2) == -1
    assert loop(opt=_capi.ApgCartpoleMpcOptions(1, 1.0, 5e-4)) == -1
    # the device entry points report the same errors before any HIP call
    lib = _capi.lib()
    o1 = R.options(1)
    assert lib.apg_cartpole_learnt_mpc_solve(1, None, DT, None, ctypes.byref(o1), 8, 10, None,
                                             None, None, None) == -1
    assert b"model is NULL" in lib.apg_last_error_string()
    assert lib.apg_cartpole_learnt_mpc_solve(1, None, DT, ctypes.byref(without("w2")),
                                             ctypes.byref(o1), 8, 10, None, None, None,
                                             None) == -1
    assert b"w1 / b1 / w2" in lib.apg_last_error_string()
    assert lib.apg_cartpole_learnt_mpc_solve(1, None, DT, ctypes.byref(ok), ctypes.byref(o1), 8,
                                             7, None, None, None, None) == -1
    assert b"H must be 5 or 10" in lib.apg_last_error_string()
    assert lib.apg_cartpole_learnt_mpc_closed_loop(
        ctypes.byref(flight(state0=1)), DT, None, None, ctypes.byref(ok), ctypes.byref(o1), 8,
        10, None, None) == -1
    assert b"plant is NULL" in lib.apg_last_error_string()


# ------------------------------------------------------------ 11: kernel resources
def test_kernels_keep_the_solver_in_registers():
    """The build's kernel_resources.json lists the two learnt-model kernels in
    every instantiation (solve: H = 5, 10; closed loop: H = 5, 10 x analytic /
    learnt plant) without scratch and without spilled VGPRs."""
    res = kernel_names.resources()
    for name, count in (("cart_mpc_learnt_solve_kernel", 2),
                        ("cart_mpc_learnt_closed_loop_kernel", 4)):
        found = kernel_names.instances(res, name)
        assert len(found) == count, (name, sorted(found))
        for k, v in found.items():
            print(k, v)
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
