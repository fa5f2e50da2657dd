"""The batched fixed-wing shooting MPC (include/apg.h: apg_wing_mpc_solve,
apg_wing_mpc_closed_loop) through its host twins (include/apg_cpu_wing_mpc.h) -
the per-lane headers csrc/wing_mpc_math.h and csrc/wing_flight_rule.h compiled
for the CPU - against the float64 restatement of the algorithm in
tests/wing_mpc_restatement.py (model: oracle.torch_port.WingOracle, gradient:
torch autograd), with the float32 restatement as the yardstick for rounding
(conftest.assert_no_worse_than_fp32, its defaults).  Runs without a GPU.  The
check_* helpers serve tests/test_gpu_wing_mpc.py with the kernel in the twin's
place."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kernel_names
import wing_mpc_restatement as R
from conftest import assert_no_worse_than_fp32, per_trajectory_err
from wing_flight_cases import GROUPS

DT = R.DT
F64, F32 = torch.float64, torch.float32
N = R.to_numpy
ITERS = (0, 1, 10, 20)


@pytest.fixture(scope="module")
def tw():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        from apg_trajectory_tracking_amd import build as b
        if not os.path.exists(b.LIB_CPU):
            pytest.fail("libapg_cpu.so is not built and there is no hipcc to build it")
    return R.twins()


# ------------------------------------------------------------------ the solve
def check_solve(got, f32, f64, what):
    """u, cost and every row of the trace under the fp64 arbiter; u in the box"""
    u = N(got["u"])
    assert u.shape == N(f64["u"]).shape
    assert u.min() >= 0.0 and u.max() <= 1.0
    assert_no_worse_than_fp32(u, N(f32["u"]), N(f64["u"]), what + " u")
    assert_no_worse_than_fp32(N(got["cost"])[:, None], N(f32["cost"])[:, None],
                              N(f64["cost"])[:, None], what + " cost")
    assert got["trace"].shape == f64["trace"].shape
    for i in range(f64["trace"].shape[0]):
        assert_no_worse_than_fp32(N(got["trace"][i])[:, None], N(f32["trace"][i])[:, None],
                                  N(f64["trace"][i])[:, None], f"{what} trace[{i}]")
    # the last row of the trace IS the returned cost
    assert np.array_equal(N(got["trace"][-1]), N(got["cost"]))


def check_the_inputs_test_something(f32, f64):
    """The conditions on the solve case, all on the restatement itself:
    the float32 restatement alone is under the 1e-4 bar on every trajectory at
    every iteration count (measured, B = 200, seed 3: worst u 1.8e-6 at 20
    iterations) - otherwise a kink decides and the inputs must change, not the
    bar; between 5 % and 60 % of the 20-iteration solution sit on the box
    (measured 32 %); no trajectory ends above its start cost (mean cost 86.0 at
    the start, 61.6 after 10 iterations, 61.3 after 20)."""
    for it in ITERS:
        e = per_trajectory_err(N(f32[it]["u"]), N(f64[it]["u"]))
        print("float32 restatement, %d iterations: worst u error %.2e" % (it, e.max()))
        assert e.max() < 1e-4, (it, e.max())
    u = f64[20]["u"]
    on_box = float(((u <= 0.0) | (u >= 1.0)).double().mean())
    print("unknowns on the box after 20 iterations: %.3f" % on_box)
    assert 0.05 < on_box < 0.60, on_box
    tr = f64[20]["trace"]
    assert int((tr[20] > tr[0]).sum()) == 0
    print("mean cost: start %.3f, 10 iterations %.3f, 20 iterations %.3f"
          % (float(tr[0].mean()), float(tr[10].mean()), float(tr[20].mean())))


def test_the_solve_case_tests_something():
    _, _, f64 = R.solve_case(F64)
    _, _, f32 = R.solve_case(F32)
    check_the_inputs_test_something(f32, f64)


@pytest.mark.parametrize("iters", ITERS)
def test_solve_twin_under_the_fp64_arbiter(tw, iters):
    """B = 200 starts of synthetic.wing_batch, the second half harder (side slip
    and vertical speed x 6, attitude x 4), from the cold start, H = 10."""
    s0, ref, f64 = R.solve_case(F64)
    _, _, f32 = R.solve_case(F32)
    check_solve(R.twin_solve(tw, s0, ref, None, DT, iters), f32[iters], f64[iters],
                f"twin iters={iters}")


def check_u0_semantics(solve, device="cpu"):
    """solve(state0, ref, u0, iters) -> dict(u, cost, ...) on tensors of `device`:
    u0 = None is the explicit cold start, the caller's tensor is left alone, a
    warm start changes the result."""
    s0, ref, _ = R.solve_case(F64)
    s0, ref = s0[:64].to(device), ref[:64].to(device)
    cold = solve(s0, ref, None, 10)
    start = R.cold_start(64).to(device)
    explicit = solve(s0, ref, start, 10)
    assert torch.equal(explicit["u"], cold["u"]) and torch.equal(explicit["cost"], cold["cost"])
    assert torch.equal(start.cpu(), R.cold_start(64))
    plan = cold["u"].clone()
    warm = solve(s0, ref, plan, 3)
    assert torch.equal(plan, cold["u"]) and not torch.equal(warm["u"], plan)
    assert float((warm["cost"] - cold["cost"]).abs().max()) > 0


def test_u0_semantics(tw):
    check_u0_semantics(lambda s0, ref, u0, iters: R.twin_solve(tw, s0, ref, u0, DT, iters))


# ------------------------------------------------------------ the closed loop
LOOP_GROUPS = GROUPS + (("seen_target", "seen", slice(12, 15)),)


def check_loop(got, case, what):
    """`got` ([B, ...] as the restatement lays it out) against the float64
    restatement of the whole loop; the float32 restatement as yardstick.  Void
    unless no flight of the float64 run comes within 1e-3 of a threshold."""
    f64, f32 = R.loop_cases(F64)[case], R.loop_cases(F32)[case]
    margin = float(f64["margin"].min())
    print(what, "float64 restatement: margin %.3e, failing flights %d, steps %d..%d"
          % (margin, int((f64["failures"] > 0).sum()), int(f64["steps"].min()),
             int(f64["steps"].max())))
    assert margin > 1e-3
    if case in ("nominal", "mismatch"):      # the flights are what they are meant to be:
        assert int(f64["steps"][32:40].max()) < int(f64["steps"][40:].min())   # lanes end early
        assert bool((f64["seen"][:8, -1, 12] == 30.0).all())                   # targets switch
    same_flights(got, f32, f64, what)
    return f64


def same_flights(got, f32, f64, what):
    """Every output of a closed loop, by name, against its restatement."""
    assert torch.equal(f32["steps"], f64["steps"])
    assert torch.equal(got["steps"].long(), f64["steps"])
    for k in ("div_pass", "div_fail"):
        assert torch.equal(got[k] >= 0, f64[k] >= 0), k
        assert torch.equal(got[k] < 0, f64[k] < 0), k
    for name, key, cols in LOOP_GROUPS:
        assert_no_worse_than_fp32(N(got[key][:, :, cols]), N(f32[key][:, :, cols]),
                                  N(f64[key][:, :, cols]), f"{what} {name}")
    for key in ("div_linear", "div_pass", "div_fail", "cost"):
        assert_no_worse_than_fp32(N(got[key]), N(f32[key]), N(f64[key]), f"{what} {key}")


def twin_loop(tw, case):
    st = R.LOOP_SETTINGS[case]
    return R.twin_closed_loop(tw, R.loop_targets(), DT, 10, R.LOOP_T, st["thresh_div"],
                              R.THRESH_STABLE, st["test_time"], plant_params=st["plant"])


def test_closed_loop_twin_vs_the_restated_loop(tw):
    """70 flights, 40 steps, targets at x = 20 with y, z in +-2; flights 0..7
    switch to a second target at x = 30, flights 32..39 end early (x = 5)."""
    f64 = check_loop(twin_loop(tw, "nominal"), "nominal", "twin nominal")
    assert int(f64["failures"].sum()) == 0


@pytest.mark.parametrize("case", ["break", "reset"])
def test_closed_loop_twin_with_failing_flights(tw, case):
    """thresh_div = 0.3: flights fail (measured: 26 of 70) - with test_time the
    flight ends there, without it the environment is reset onto the line while
    the solver goes on planning from the last simulated state."""
    f64 = check_loop(twin_loop(tw, case), case, f"twin {case}")
    assert int((f64["failures"] > 0).sum()) >= 1
    if case == "reset":        # a reset flight flies on, and may fail again
        assert int(f64["steps"].max()) == R.LOOP_T
        assert int(f64["failures"].max()) >= 2


def check_mismatch_differs(got, what):
    nominal = R.loop_cases(F64)["nominal"]
    d = float((got["drone"].double() - nominal["drone"]).abs().max())
    print(what, "largest difference from the nominal flight: %.3e" % d)
    assert d > 1e-3


def test_closed_loop_twin_model_mismatch(tw):
    """Plant {"mass": 1.3, "CL_alpha": 4.0}, model nominal: the logs follow the
    restated loop and differ from the nominal flight; with the roles swapped the
    flight is another one again."""
    got = twin_loop(tw, "mismatch")
    check_loop(got, "mismatch", "twin mismatch")
    check_mismatch_differs(got, "twin mismatch")
    swapped = R.twin_closed_loop(tw, R.loop_targets(), DT, 10, R.LOOP_T, 10.0,
                                 R.THRESH_STABLE, 0, model_params=R.MISMATCH)
    assert float((swapped["drone"] - got["drone"]).abs().max()) > 1e-3


# ------------------------------------------------------------- the MPC object
def _twin_behind_functional(tw, monkeypatch):
    """functional.wing_mpc_solve on CPU tensors: the host twin behind the same
    signature (tests only - the package itself never loads the twins)."""
    from apg_trajectory_tracking_amd import functional as F

    def stand_in(state0, ref, dt, params, u0=None, weights=None, iters=None, beta=None,
                 alpha_thrust=None, alpha_surface=None, want_trace=False):
        return R.twin_solve(tw, state0, ref, u0, dt, 10 if iters is None else iters)
    monkeypatch.setattr(F, "wing_mpc_solve", stand_in)


def check_mpc_object(loop, device):
    """`MPC(dynamics="fixed_wing_3D").predict_actions(state, target)`; loop: the
    first two steps of the closed loop on loop_targets() ([B, ...])."""
    from apg_trajectory_tracking_amd.controllers import MPC
    tg = R.loop_targets()[:, 0].to(device)
    B = tg.shape[0]
    s0 = torch.zeros(B, 12, device=device)
    s0[:, 3] = 11.5
    batched = MPC(horizon=10, dt=DT, dynamics="fixed_wing_3D", device=device)
    a = batched.predict_actions(s0, tg)
    assert torch.is_tensor(a) and a.shape == (B, 4)
    assert batched.warm_start.shape == (B, 10, 4)
    assert np.abs(N(a) - N(loop["drone"][:, 0, 12:])).max() <= 1e-6
    single = MPC(horizon=10, dt=DT, dynamics="fixed_wing_3D", device=device)
    a0 = single.predict_actions(s0[0].cpu().numpy(), tg[0].cpu().numpy())
    assert isinstance(a0, np.ndarray) and a0.shape == (1, 4)
    assert np.array_equal(a0[0], a[0].cpu().numpy())
    # the second call = the loop's second action: the warm start is shifted
    a2 = batched.predict_actions(loop["drone"][:, 0, :12].to(device), tg)
    assert np.abs(N(a2) - N(loop["drone"][:, 1, 12:])).max() <= 1e-6
    batched.reset()
    assert batched.warm_start is None
    assert torch.equal(batched.predict_actions(s0, tg), a)
    mod = MPC(horizon=10, dt=DT, dynamics="fixed_wing_3D", modified_params=R.MISMATCH)
    assert mod.params.mass == pytest.approx(1.3) and mod.params.CL_alpha == pytest.approx(4.0)
    with pytest.raises(ValueError):
        MPC(horizon=20, dt=DT, dynamics="fixed_wing_3D")
    with pytest.raises(ValueError):
        MPC(horizon=5, dt=DT, dynamics="fixed_wing_3D")
    for name in ("fixed_wing", "fixed_wing_2D", "simple_quad", "high_mpc"):
        with pytest.raises(NotImplementedError, match="flightmare"):
            MPC(dynamics=name)
    with pytest.raises(NotImplementedError):
        MPC(horizon=10, dt=DT, dynamics="fixed_wing_3D", learnt_model=object())
    with pytest.raises(ValueError):
        single.predict_actions(np.zeros(11), np.zeros(3))


def test_mpc_object_surface_and_warm_start(tw, monkeypatch):
    _twin_behind_functional(tw, monkeypatch)
    loop = R.twin_closed_loop(tw, R.loop_targets()[:, :1], DT, 10, 2, 10.0, R.THRESH_STABLE, 0)
    check_mpc_object(loop, "cpu")


# -------------------------------------------------------------- the evaluator
EVAL_SEED = 5


def check_evaluator(device):
    """`FixedWingEvaluator(MPC(...), FixedWingDynamics())`: run_eval(16,
    max_steps=120) under np.random.seed equals the statistics of the float64
    restatement on the same drawn targets; the numpy stream is left where the
    network controller's evaluator leaves it (one rand(nr_test, 2))."""
    from apg_trajectory_tracking_amd.controllers import MPC
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
        FixedWingDynamics, LearntFixedWingDynamics)
    from apg_trajectory_tracking_amd.evaluate_fixed_wing import FixedWingEvaluator
    targets, f64, want = R.eval_case(EVAL_SEED)
    print("float64 restatement: steps %d..%d, margin %.3e, mean target error %.4f"
          % (int(f64["steps"].min()), int(f64["steps"].max()), float(f64["margin"].min()),
             want.mean()))
    assert float(f64["margin"].min()) > 1e-3
    assert int(f64["steps"].max()) < 120        # every flight passes its target
    mpc = MPC(horizon=10, dt=DT, dynamics="fixed_wing_3D", device=device,
              modified_params={})
    ev = FixedWingEvaluator(mpc, FixedWingDynamics(), dt=DT)
    np.random.seed(EVAL_SEED)
    mean, std = ev.run_eval(16, max_steps=120, printout=False)
    after = np.random.rand()
    np.random.seed(EVAL_SEED)
    np.random.rand(16, 2)
    assert np.random.rand() == after
    assert np.isclose(mean, want.mean(), rtol=1e-3) and np.isclose(std, want.std(), rtol=1e-3)
    assert ev.last_flights["cost"].shape == (120, 16)
    assert torch.equal(ev.last_flights["steps"].cpu().long(), f64["steps"])
    np.random.seed(EVAL_SEED)
    dists = ev.run_eval(16, max_steps=120, printout=False, return_dists=True)
    np.testing.assert_allclose(dists, want, rtol=1e-3)
    # fly_to_point returns what it returns for a network controller
    div_target, div_linear = ev.fly_to_point(targets[0].numpy(), max_steps=120)
    n = int(f64["steps"][0])
    assert div_linear.shape == (n,) and len(div_target) == 1
    np.testing.assert_allclose(div_linear, N(f64["div_linear"][0, :n]), rtol=1e-3, atol=1e-5)
    traj = ev.fly_to_point(targets[:3].numpy(), max_steps=120, return_traj=True)
    assert [t.shape for t in traj] == [(int(s), 16) for s in f64["steps"][:3]]
    with pytest.raises(TypeError):
        FixedWingEvaluator(mpc, LearntFixedWingDynamics(), dt=DT)
    with pytest.raises(ValueError, match="dt"):
        FixedWingEvaluator(mpc, FixedWingDynamics(), dt=0.01).run_eval(2, max_steps=3)
    return ev


def test_evaluator_routes_an_mpc_controller_to_the_mpc_closed_loop(tw, monkeypatch):
    """The evaluator's host logic with an MPC controller (no GPU: the host twin
    stands behind functional.wing_mpc_closed_loop): plant = the environment's
    parameters, model = the MPC's own."""
    from apg_trajectory_tracking_amd import functional as F
    seen = {}

    def stand_in(targets, dt, params, model_params=None, state0=None, weights=None,
                 max_steps=1000, thresh_div=10.0, thresh_stable=0.8, test_time=0,
                 want_trajectory=False, **options):
        seen.update(plant=params.mass, model=model_params.mass, options=options)
        o = R.twin_closed_loop(tw, targets, dt, options["iters"], max_steps, thresh_div,
                               thresh_stable, test_time)
        out = {k: o[k].t().contiguous() for k in ("div_linear", "div_pass", "div_fail", "cost")}
        out["steps"] = o["steps"].to(torch.int32)
        if want_trajectory:
            out.update(drone=o["drone"].permute(1, 2, 0).contiguous(),
                       seen=o["seen"].permute(1, 2, 0).contiguous())
        return out
    monkeypatch.setattr(F, "wing_mpc_closed_loop", stand_in)
    check_evaluator("cpu")
    assert seen["plant"] == pytest.approx(1.01) and seen["model"] == pytest.approx(1.01)
    assert seen["options"] == dict(iters=10, beta=None, alpha_thrust=None, alpha_surface=None)


def test_every_field_of_the_flight_struct_is_the_one_it_is_named(tw):
    """ApgWingFlight through the twin on the smallest case whose outputs all
    differ from each other: B = 3, two targets, T = 4, test_time = 1, thresh_div
    = 0.3.  Flight 0 passes a first target at x = 1 after two steps and flies on
    to the second (an entry in div_pass only); flight 1's target lies 8 m to the
    side: flying off at 11.5 m/s along x it leaves the line by more than 0.3 at
    its second step and ends there (an entry in div_fail only, steps = 2); flight
    2 flies its four steps with neither.  Each output is held by name against the
    float64 restatement at the tolerances of the loop tests above; a same-typed
    neighbour swapped in the struct, in the ctypes mirror or in a forwarding layer
    fails one of them.  Flown again with drone / seen NULL, the other outputs
    keep their bits."""
    targets = torch.tensor([[[1.0, 0.05, 0.05], [30.0, 0.5, -0.5]],
                            [[20.0, 8.0, 0.0], [20.0, 8.0, 0.0]],
                            [[20.0, 0.5, 0.5], [20.0, 0.5, 0.5]]])
    flown = dict(iters=10, T=4, thresh_div=0.3, thresh_stable=R.THRESH_STABLE, test_time=1)
    with R.few_threads():
        f64, f32 = (R.closed_loop(dt, targets, DT, **flown) for dt in (F64, F32))
    print("float64 restatement: steps", f64["steps"].tolist(), "margin %.3e"
          % float(f64["margin"].min()))
    assert float(f64["margin"].min()) > 1e-3        # clear of every threshold
    assert f64["steps"].tolist() == [4, 2, 4]
    flown_rows = torch.arange(4)[None] < f64["steps"][:, None]      # (rows not flown: zero)
    passed = ((f64["div_pass"] >= 0) & flown_rows).sum(1)
    failed = ((f64["div_fail"] >= 0) & flown_rows).sum(1)
    assert passed.tolist() == [1, 0, 0] and failed.tolist() == [0, 1, 0]
    assert bool((f64["seen"][0, -1, 12:] == targets[0, 1].double()).all())   # target switch
    got = R.twin_closed_loop(tw, targets, DT, **flown)
    same_flights(got, f32, f64, "flight struct")
    bare = R.twin_closed_loop(tw, targets, DT, want_trajectory=False, **flown)
    for k in ("div_linear", "div_pass", "div_fail", "steps", "cost"):
        assert torch.equal(bare[k], got[k]), k
    assert not bare["drone"].any() and not bare["seen"].any()


# ------------------------------------------------------------ ABI, resources
def test_twin_argument_errors_and_abi(tw):
    from apg_trajectory_tracking_amd import _capi, functional as F
    assert ctypes.sizeof(_capi.ApgWingMpcOptions) == 16
    B = 8
    s0, ref, _ = R.solve_case(F64)
    s = s0[:B].t().contiguous()
    r = ref[:B].permute(1, 2, 0).contiguous()
    u, cost = R.cold_start(B).permute(1, 2, 0).contiguous(), torch.zeros(B)
    p, w = R.params(), F.wing_loss_weights()
    err = lambda: tw.apg_cpu_last_error_string()

    def solve(H=10, opt=None, B=B, state=s, model=p):
        o = opt or R.options(1)
        return tw.apg_wing_mpc_solve_cpu(
            None if state is None else state.data_ptr(), r.data_ptr(), DT,
            None if model is None else ctypes.byref(model), ctypes.byref(w), ctypes.byref(o),
            B, H, u.data_ptr(), cost.data_ptr(), None)
    assert solve() == 0
    assert solve(B=0, state=None) == 0
    assert solve(state=None) == -1 and b"NULL buffer" in err()
    assert solve(model=None) == -1 and b"model / weights is NULL" in err()
    assert solve(B=-1) == -1 and b"B must be >= 0" in err()
    for H in (5, 7, 20):
        assert solve(H=H) == -1 and b"H must be 10" in err()
    assert solve(opt=_capi.ApgWingMpcOptions(-1, 0.5, 0.03, 0.03)) == -1 and b"iters" in err()
    assert solve(opt=_capi.ApgWingMpcOptions(100001, 0.5, 0.03, 0.03)) == -1 and b"iters" in err()
    assert solve(opt=_capi.ApgWingMpcOptions(1, 1.0, 0.03, 0.03)) == -1 and b"beta" in err()
    assert solve(opt=_capi.ApgWingMpcOptions(1, -0.1, 0.03, 0.03)) == -1 and b"beta" in err()
    assert solve(opt=_capi.ApgWingMpcOptions(1, 0.5, 0.0, 0.03)) == -1 and b"alpha" in err()
    assert solve(opt=_capi.ApgWingMpcOptions(1, 0.5, 0.03, -1.0)) == -1 and b"alpha" in err()

    tg = R.loop_targets()[:B].permute(1, 2, 0).contiguous()
    T = 3
    logs = [torch.zeros(T, B) for _ in range(3)]
    steps = torch.zeros(B, dtype=torch.int32)

    def loop(n=2, T=T, H=10, plant=p, steps=steps, B=B, flight=True):
        fl = _capi.ApgWingFlight(
            targets=tg.data_ptr(), state0=None, n_targets=n, max_steps=T, thresh_div=10.0,
            thresh_stable=0.8, test_time=0, div_linear=logs[0].data_ptr(),
            div_pass=logs[1].data_ptr(), div_fail=logs[2].data_ptr(),
            steps=None if steps is None else steps.data_ptr(), drone=None, seen=None)
        return tw.apg_wing_mpc_closed_loop_cpu(
            ctypes.byref(fl) if flight else None, DT,
            None if plant is None else ctypes.byref(plant), ctypes.byref(p), ctypes.byref(w),
            ctypes.byref(R.options(1)), B, H, None)
    assert loop() == 0 and steps.tolist() == [T] * B   # drone, seen, cost NULL: writes dropped
    assert loop(B=0) == 0
    assert loop(flight=False) == -1 and b"flight is NULL" in err()
    assert loop(n=0) == -1 and b"n_targets must be >= 1" in err()
    assert loop(T=0) == -1 and b"max_steps must be >= 1" in err()
    assert loop(H=5) == -1 and b"H must be 10" in err()
    assert loop(plant=None) == -1 and b"plant is NULL" in err()
    assert loop(steps=None) == -1 and b"NULL buffer" in err()


def test_kernels_keep_the_solver_out_of_scratch():
    """The build's kernel_resources.json lists both kernels (H = 10) without
    scratch and without spilled VGPRs; the stash is their 30 KB of LDS."""
    res = kernel_names.resources()
    for name in ("wing_mpc_solve_kernel", "wing_mpc_closed_loop_kernel"):
        found = kernel_names.instances(res, name)
        assert sorted(found) == ["ILi10E"], (name, sorted(found))
        for k, v in found.items():
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (name, k, v)
