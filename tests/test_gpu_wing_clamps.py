"""Every fixed-wing kernel where the alpha / beta clamps of csrc/wing_math.h are
active: the step kernels (AoS through FixedWingDynamics' autograd, SoA through
the C ABI), apg_wing_rollout_fwd_bwd in its literal-constant and table
instances, one and two trajectories per lane, at the checkpoint strides 1, 3 and
4, apg_wing_rollout_fwd, the learnt simulator's step, fused rollout and fused
fit, and the closed loop over the analytic and the learnt plant - on the inputs
of tests/wing_clamp_cases.py (both clamps, alone and together, switching along
the horizon, within 0.1 % of a bound on either side, u < 0 and u = +-0 for the
step kernels), judged as tests/test_wing_clamps_cpu.py judges the host build of
the same headers: the float64 oracle arbitrates, the float32 oracle is the
yardstick (conftest.assert_no_worse_than_fp32's factors, the 1e-4 bar per
trajectory).  Coverage of the clamps and the cap on trajectories set aside as
too near a kink are asserted with every reference; every test prints what it
measured (pytest -s).

Not tested: u = v = w = 0, which is NaN in the reference itself."""
import ctypes

import numpy as np
import pytest
import torch

import wing_clamp_cases as wc
from conftest import (assert_no_worse_than_fp32, assert_param_rows_no_worse_than_fp32,
                      load_golden, oracle_wing_closed_loop, per_trajectory_err,
                      wing_loop_policy)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def wing_pk():
    """Selects the fused rollout kernel for plane-layout batches
    (apg_wing_set_two_per_lane: 1 = two trajectories per lane whenever
    possible, 0 = never) and restores the shipped choice (2: by batch size)."""
    from apg_trajectory_tracking_amd import _capi

    def choose(mode):
        _capi.check(_capi.lib().apg_wing_set_two_per_lane(int(mode)),
                    "apg_wing_set_two_per_lane")
    yield choose
    choose(2)


def N(t):
    return t.detach().cpu().numpy()


def dynamics(tag):
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    return FixedWingDynamics(modified_params=dict(wc.PARAMS[tag]))


# ---------------------------------------------------------------------- step
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("tag", ["def", "mod"])
def test_step_kernels_and_jacobian(dev, tag, layout):
    """apg_wing_step_fwd / apg_wing_step_bwd on step_cases(), 12 copies with
    one-hot cotangents in one launch: next states per trajectory and every
    (output, input) column of the Jacobian; finite at u = +-0 and equal to the
    float64 oracle next to 0."""
    from apg_trajectory_tracking_amd import _capi
    dyn = dynamics(tag)

    def run_aos(s, a, cot):
        s = torch.from_numpy(s).to(dev).requires_grad_(True)
        a = torch.from_numpy(a).to(dev).requires_grad_(True)
        nxt = dyn(s, a, wc.DT)
        gs, ga = torch.autograd.grad(nxt, (s, a), torch.from_numpy(cot).to(dev))
        return N(nxt), N(gs), N(ga)

    def run_soa(s, a, cot):
        lib = _capi.lib()
        s, a, cot = (torch.from_numpy(x).to(dev).t().contiguous() for x in (s, a, cot))
        B = s.shape[1]
        nxt, gs, ga = torch.empty_like(s), torch.empty_like(s), torch.empty_like(a)
        st = torch.cuda.current_stream().cuda_stream
        _capi.check(lib.apg_wing_step_fwd(s.data_ptr(), a.data_ptr(), wc.DT,
                                          ctypes.byref(dyn.params), B, _capi.LAYOUT_SOA,
                                          nxt.data_ptr(), st), "apg_wing_step_fwd")
        _capi.check(lib.apg_wing_step_bwd(s.data_ptr(), a.data_ptr(), wc.DT,
                                          ctypes.byref(dyn.params), B, _capi.LAYOUT_SOA,
                                          cot.data_ptr(), gs.data_ptr(), ga.data_ptr(), st),
                    "apg_wing_step_bwd")
        return N(nxt.t()), N(gs.t()), N(ga.t())
    wc.check_step(run_aos if layout == "aos" else run_soa, tag, f"gpu step/{tag}/{layout}")


# ------------------------------------------------------------------- rollout
B_ROLL = 2050          # even, ragged against 64 and against 128


@pytest.mark.parametrize("layout", ["aos", "soa", "soa_two_per_lane"])
@pytest.mark.parametrize("H", [6, 13, 20])       # checkpoint strides 1, 3, 4
@pytest.mark.parametrize("tag", ["def", "mod"])  # literal-constant / table instances
def test_rollout_fwd_bwd(dev, wing_pk, tag, H, layout):
    """The reverse sweep re-integrates the states between two checkpoints: it
    must take the clamp branches the forward pass took.  Two per lane: the two
    trajectories of a lane share every packed instruction, each with its own
    mask."""
    from apg_trajectory_tracking_amd import functional as F
    assert (H + 5) // 6 == {6: 1, 13: 3, 20: 4}[H]
    ref = wc.rollout_reference(B_ROLL, H, tag)
    d = ref["d"]
    dyn = dynamics(tag)
    what = f"gpu rollout/{tag}/H{H}/{layout}"
    if layout == "soa_two_per_lane":
        wing_pk(1)
        layout = "soa"
        print(what, "lane pairs in mixed clamp state: %.3f" % wc.mixed_pairs(ref["pre"]))
    else:
        wing_pk(0)
    a = (d["state0"].to(dev), d["actions"].to(dev), d["ref"].to(dev))
    if layout == "soa":
        a = (a[0].t().contiguous(), a[1].permute(1, 2, 0).contiguous(),
             a[2].permute(1, 2, 0).contiguous())
    res = F.wing_rollout_fwd_bwd(*a, wc.DT, dyn.params, layout=layout, want_states=True)
    fwd = F.wing_rollout_fwd(a[0], a[1], wc.DT, dyn.params, layout=layout)
    st, ga, gs = res["states"], res["grad_actions"], res["grad_state0"]
    if layout == "soa":
        st, ga, gs, fwd = (st.permute(2, 0, 1), ga.permute(2, 0, 1), gs.t(),
                           fwd.permute(2, 0, 1))
    wc.check_rollout(dict(states=N(st), loss=res["loss"].item(), grad_actions=N(ga),
                          grad_state0=N(gs)), ref, what)
    wc.check_rollout(dict(states=N(fwd)), ref, what + " (apg_wing_rollout_fwd)",
                     states_only=True)


# ------------------------------------------------------------ learnt simulator
def module(which, dev):
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
        LearntFixedWingDynamics)
    dyn = LearntFixedWingDynamics()
    res = dyn.load_state_dict({k: torch.from_numpy(v)
                               for k, v in wc.learnt_weights(which).items()})
    assert not res.missing_keys and not res.unexpected_keys
    return dyn.to(dev)


@pytest.mark.parametrize("which", ["w", "steps"])
def test_learnt_step_kernels_and_jacobian(dev, which):
    """apg_wing_learnt_step_fwd / _bwd (the general-inertia table) on
    step_cases() - the near-bound rows, u < 0 and u = +-0 included - through
    the module's autograd, residual network and all."""
    dyn = module(which, dev)

    def run(s, a, cot):
        s = torch.from_numpy(s).to(dev).requires_grad_(True)
        a = torch.from_numpy(a).to(dev).requires_grad_(True)
        nxt = dyn(s, a, wc.DT)
        gs, ga = torch.autograd.grad(nxt, (s, a), torch.from_numpy(cot).to(dev))
        return N(nxt), N(gs), N(ga)
    wc.check_step(run, which, f"gpu learnt step cases/{which}")


@pytest.mark.parametrize("which", ["w", "steps"])
def test_learnt_step_and_every_parameter_gradient(dev, which):
    """LearntFixedWingDynamics forward and backward (apg_wing_learnt_step_fwd /
    _bwd) on the fit batch with the fit's cotangent: next state, dL/dstate and
    dL/daction per trajectory, grad_params[50] parameter by parameter relative
    to the summed magnitudes of the samples' gradients, the residual's rows."""
    ref = wc.fit_reference(which)
    f64, f32 = ref["step"]["f64"], ref["step"]["f32"]
    dyn = module(which, dev)
    s = ref["state"].to(dev).requires_grad_(True)
    a = ref["action"].to(dev).requires_grad_(True)
    nxt = dyn(s, a, wc.DT)
    (nxt * ref["cot32"].to(dev)).sum().backward()
    what = f"gpu learnt step/{which}"
    for name, got in (("pred", nxt), ("grad_state", s.grad), ("grad_action", a.grad)):
        got = N(got)
        assert np.all(np.isfinite(got)), name
        assert_no_worse_than_fp32(got, f32[name], f64[name], f"{what} {name}")
    g = {k: (None if p.grad is None else N(p.grad)) for k, p in dyn.named_parameters()}
    wc.assert_physical_no_worse_than_fp32(g, dict(ref["step"], scale=ref["scale"]), what)
    pick = lambda x: {k: np.asarray(x[k]) for k in wc.RESIDUAL}
    assert_param_rows_no_worse_than_fp32(pick(g), pick(f32["g"]), pick(f64["g"]), what)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("H", [10, 20])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_learnt_rollout(dev, which, H, layout):
    from apg_trajectory_tracking_amd import functional as F
    B = 258
    ref = wc.learnt_rollout_reference(which, B, H)
    d = ref["d"]
    dyn = module(which, dev)
    a = (d["state0"].to(dev), d["actions"].to(dev), d["ref"].to(dev))
    if layout == "soa":
        a = (a[0].t().contiguous(), a[1].permute(1, 2, 0).contiguous(),
             a[2].permute(1, 2, 0).contiguous())
    res = F.wing_learnt_rollout_fwd_bwd(dyn, *a, wc.DT, layout=layout, want_states=True)
    st, ga, gs = res["states"], res["grad_actions"], res["grad_state0"]
    if layout == "soa":
        st, ga, gs = st.permute(2, 0, 1), ga.permute(2, 0, 1), gs.t()
    wc.check_learnt_rollout(dict(states=N(st), loss=res["loss"].item(), grad_actions=N(ga),
                                 grad_state0=N(gs)), ref,
                            f"gpu learnt rollout/{which}/H{H}/{layout}")


@pytest.mark.parametrize("mode", ["params", "target"])
@pytest.mark.parametrize("which", ["w", "steps"])
def test_learnt_fit(dev, which, mode):
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import FixedWingDynamics
    ref = wc.fit_reference(which)
    dyn = module(which, dev)
    kw = (dict(eval_params=FixedWingDynamics(modified_params=wc.target_mod()).params)
          if mode == "params" else dict(target=torch.from_numpy(ref["target32"]).to(dev)))
    res = F.wing_learnt_fit_fwd_bwd(dyn, ref["state"].to(dev), ref["action"].to(dev), wc.DT,
                                    **kw)
    views = F.wing_learnt_fit_grad_views(dyn, res["grad"])
    g = {name: N(v) for (name, _), v in zip(dyn.named_parameters(), views)}
    wc.check_fit(dict(loss=float(res["loss"].item()), g=g), ref, mode,
              f"gpu fit/{which}/{mode}")


# ---------------------------------------------------------------- closed loop
@pytest.mark.parametrize("plant", ["analytic", "learnt"])
def test_closed_loop_three_steps(dev, plant):
    """apg_wing_mlp_closed_loop from clamp_batch start states: three steps,
    thresholds so wide that no flight resets or ends; the drone states per
    trajectory against the oracle's loop at 1e-4.  The clamp states are read
    off the states the oracle's policy saw."""
    from apg_trajectory_tracking_amd import functional as F
    from oracle import torch_port as tp
    B, T = 300, 3
    g = load_golden("wing_closed_loop.npz")
    net = wing_loop_policy(dev)
    state0 = wc.clamp_batch(B, 1, wc.DT, seed=B)["state0"]
    gen = torch.Generator().manual_seed(31)
    targets = torch.zeros(B, 2, 3)
    targets[:, :, 0] = torch.tensor([30., 60.]) + 6 * torch.rand(B, 2, generator=gen) - 3
    targets[:, :, 1:] = 8 * torch.rand(B, 2, 2, generator=gen) - 4
    kw = dict(data_dt=float(g["data_dt"]), data_horizon=int(g["data_horizon"]),
              max_steps=T, thresh_div=1e3, thresh_stable=10.0, test_time=0,
              want_trajectory=True)
    dyn = dynamics("def")
    learnt = oracle = None
    if plant == "learnt":
        gl = load_golden("wing_closed_loop_learnt.npz")
        w = {k[len("dyn."):]: gl[k] for k in gl.files if k.startswith("dyn.")}
        from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
            LearntFixedWingDynamics)
        learnt = LearntFixedWingDynamics()
        learnt.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        learnt = learnt.to(dev)
        oracle = tp.LearntWingOracle(w, dtype=torch.float32)
    out = F.wing_mlp_closed_loop(net, targets.to(dev), float(g["dt"]), dyn.params,
                                 g["mean"].tolist(), g["std"].tolist(),
                                 state0=state0.to(dev), learnt=learnt, **kw)
    with torch.no_grad():
        ref = oracle_wing_closed_loop(net, targets, float(g["dt"]), None, g["mean"], g["std"],
                                      state0=state0, learnt=oracle, **kw)
    assert torch.all(ref["steps"] == T) and not bool((ref["div_fail"] >= 0).any())
    assert torch.all(out["steps"].cpu() == T)
    pre = ref["seen"].numpy()[:, :12].transpose(2, 0, 1)
    keep = wc.assert_coverage(pre, f"closed loop/{plant}")
    got = N(out["drone"])[:, :12].transpose(2, 0, 1)
    want = ref["drone"].numpy()[:, :12].transpose(2, 0, 1)
    assert np.all(np.isfinite(N(out["drone"])))
    e = per_trajectory_err(got[keep], want[keep])
    print(f"closed loop/{plant}: per-trajectory worst %.3g, median %.3g" % (
        e.max(), np.median(e)))
    assert e.max() < wc.BAR
