"""The conditions tests/quad_loss_cases.py promises about its inputs, held with
the float64 oracle, and the host twins (apg_quad_rollout_fwd_bwd_cpu,
apg_quad_mpc_solve_cpu) under non-default loss weights.  Runs without a GPU.

The conditions are what makes the GPU files (test_gpu_quad_loss_weights.py,
test_gpu_quad_learnt_rollout.py) able to fail:
  * under `balanced` every weighted term is 10-40 % of the loss of every batch
    a kernel is run on - none hides below a bar;
  * exchanging av and rates (`swapped`) moves the float64 loss and every
    compared gradient by at least 100 x the bar the GPU test applies;
  * at most 6 % of the trajectories of a learnt case sit on a ReLU kink and are
    set aside from the gradient comparisons;
  * the float32 oracle itself meets 1e-4 per trajectory on everything kept."""
import numpy as np
import pytest
import torch

import quad_loss_cases as C
import quad_mpc_restatement as R
import test_cpu_twins as T
from conftest import per_trajectory_err, rel_err
from test_cpu_twins import tw  # noqa: F401
from test_quad_mpc_cpu import check_solve

F64, F32 = torch.float64, torch.float32
ROLLOUT_BATCHES = [(200, 5), (200, 7), (200, 10), (200, 23), (67, 10)]
LOSS_BAR, GRAD_BAR = 1e-5, 1e-4        # the GPU tests' bars


def _print(what, **kw):
    print(what, {k: (np.asarray(v).round(4).tolist() if np.ndim(v) else float("%.3g" % v))
                 for k, v in kw.items()})


def _moved(a, b):
    """Largest per-trajectory distance of a from b (per_trajectory_err)."""
    return float(per_trajectory_err(a, b).max())


# ------------------------------------------------------ shares and the swap
@pytest.mark.parametrize("B,H", ROLLOUT_BATCHES)
def test_rollout_batches_balanced_shares_and_swap_margin(B, H):
    w = C.balanced(C.rollout_key(B, H))
    bal = C.rollout_oracle(B, H, w)
    s = C.check_balanced(bal["terms"], w)
    swp = C.rollout_oracle(B, H, C.swapped(w))
    d_loss = abs(swp["loss"] - bal["loss"]) / bal["loss"]
    d_ga = _moved(swp["grad_actions"], bal["grad_actions"])
    d_gs = _moved(swp["grad_state0"], bal["grad_state0"])
    d_part = float((np.abs(swp["partials"] - bal["partials"]) / bal["partials"]).min())
    _print(f"B={B} H={H}", unit_terms=bal["terms"].sum(0), shares=s, swap_loss=d_loss,
           swap_grad_actions=d_ga, swap_grad_state0=d_gs, swap_partials_min=d_part)
    assert d_loss >= 100 * LOSS_BAR and d_part >= 100 * LOSS_BAR
    assert d_ga >= 100 * GRAD_BAR and d_gs >= 100 * GRAD_BAR
    # the loss kernel's dL/dstates: the av columns of every state row scale with
    # w.av alone - exchanging the two weights moves them by |rates / av - 1|
    assert abs(w[3] / w[2] - 1) >= 100 * GRAD_BAR


@pytest.mark.parametrize("H", [7, 23])
def test_packed_reference_rows_velocity_column_margin(H):
    """The LDS kernel with packed [pos, vel] rows (ref_cols = 6) must read the
    velocity at column 3.  Reading column 6 (where [pos, euler, vel] rows keep
    it) lands on the NEXT row's position in the AoS tensor: the float64 loss
    under the one-hot vel set and under `balanced` then moves by far more than
    100 x the bar, so the GPU test sees it."""
    B = 200
    s0, a, ref = C.rollout_batch(B, H)
    flat = torch.cat((C.packed_ref(ref).double().reshape(-1), torch.zeros(6, dtype=F64)))
    at = (torch.arange(B * H) * 6 + 6)[:, None] + torch.arange(3)[None]
    wrong = C.packed_ref(ref).double().clone()
    wrong[:, :, 3:6] = flat[at].reshape(B, H, 3)
    states = torch.from_numpy(C.rollout_oracle(B, H, C.DEFAULT)["states"])
    for w in (C.ONE_HOT["vel"], C.balanced(C.rollout_key(B, H))):
        fn = C.weighted_quad_mpc_loss(w)
        good = float(fn(states, C.packed_ref(ref).double(), a.double()))
        bad = float(fn(states, wrong, a.double()))
        print(f"H={H} vel column 6 for 3 moves the loss by", abs(bad - good) / good)
        assert abs(bad - good) / good >= 100 * LOSS_BAR


def test_learnt_weight_case_balanced_shares_and_swap_margin():
    w = C.balanced(C.learnt_key("golden", 10))
    bal = C.learnt_oracle("golden", 200, 10, w)
    s = C.check_balanced(bal["terms"], w)
    swp = C.learnt_oracle("golden", 200, 10, C.swapped(w))
    d_loss = abs(swp["loss"] - bal["loss"]) / bal["loss"]
    d_ga = _moved(swp["grad_actions"], bal["grad_actions"])
    d_gs = _moved(swp["grad_state0"], bal["grad_state0"])
    _print("learnt golden H=10", shares=s, swap_loss=d_loss, swap_grad_actions=d_ga,
           swap_grad_state0=d_gs)
    assert d_loss >= 100 * LOSS_BAR and d_ga >= 100 * GRAD_BAR and d_gs >= 100 * GRAD_BAR


@pytest.mark.parametrize("kind", C.POLICY_KINDS)
def test_policy_batches_balanced_shares_and_swap_margin(kind):
    """With the policy's OWN actions (float64 policy + oracle unroll)."""
    w = C.balanced(C.policy_key(kind))
    bal = C.policy_oracle(kind, w)
    s = C.check_balanced(bal["terms"], w)
    swp = C.policy_oracle(kind, C.swapped(w))
    d_loss = abs(swp["loss"] - bal["loss"]) / abs(bal["loss"])
    d = {k: rel_err(swp["grads"][k], g) for k, g in bal["grads"].items()}
    _print(f"policy {kind}", shares=s, swap_loss=d_loss, swap_grads_min=min(d.values()))
    assert d_loss >= 100 * LOSS_BAR
    assert min(d.values()) >= 100 * GRAD_BAR, d


def test_mpc_case_balanced_shares_and_swap_margin():
    """Shares at the actions the float64 restatement returns under `balanced`."""
    w = C.balanced("mpc")
    bal = C.mpc_restated(w)
    s = C.check_balanced(C.mpc_terms(bal["u"]), w)
    swp = C.mpc_restated(C.swapped(w))
    d_u = _moved(R.to_numpy(swp["u"]), R.to_numpy(bal["u"]))
    d_cost = _moved(R.to_numpy(swp["cost"])[:, None], R.to_numpy(bal["cost"])[:, None])
    trace = R.to_numpy(bal["trace"]).mean(1)
    _print("mpc", shares=s, swap_u=d_u, swap_cost=d_cost, mean_cost_per_iteration=trace)
    assert trace[-1] < 0.7 * trace[0]          # (the rule still descends under these weights)
    assert d_u >= 100 * GRAD_BAR and d_cost >= 100 * GRAD_BAR


# ------------------------------------------------ the learnt cases' oracle
@pytest.mark.parametrize("which,H", C.LEARNT_CASES)
def test_learnt_cases_kink_share_and_float32_oracle(which, H):
    """Measured at B = 1003: kink share 5.5 % (steps, H = 48), <= 2.8 % at H =
    21 / 22, <= 1.1 % at H <= 10; the float32 oracle's worst kept trajectory
    2.1e-5 (dL/dstate0, steps, H = 48)."""
    f64 = C.learnt_oracle(which, C.LEARNT_B, H)
    f32 = C.learnt_oracle(which, C.LEARNT_B, H, C.DEFAULT, F32)
    share = float(f64["kink"].mean())
    keep = ~f64["kink"]
    e = dict(states=per_trajectory_err(f32["states"], f64["states"]).max(),
             grad_actions=per_trajectory_err(f32["grad_actions"][keep],
                                             f64["grad_actions"][keep]).max(),
             grad_state0=per_trajectory_err(f32["grad_state0"][keep],
                                            f64["grad_state0"][keep]).max())
    _print(f"{which} H={H}", kink_share=share, **e)
    assert share <= C.MAX_KINK_SHARE
    assert np.isfinite(f32["states"]).all() and max(e.values()) < 1e-4, e
    assert abs(f32["loss"] - f64["loss"]) < 1e-5 * f64["loss"]


# ------------------------------------------- the host twins under the weights
def _tensor_err(got, want):
    """conftest.rel_err; an identically zero float64 tensor must be met exactly."""
    if not np.asarray(want).any():
        assert not np.asarray(got).any(), "must be exactly zero"
        return 0.0
    return rel_err(got, want)


@pytest.mark.parametrize("wname", list(C.NAMES) + ["balanced"])
@pytest.mark.parametrize("H", [5, 10, 7])
@pytest.mark.parametrize("layout", [T.AOS, T.SOA])
def test_rollout_twin_under_the_weight_sets(tw, layout, H, wname):
    """apg_quad_rollout_fwd_bwd_cpu against the float64 oracle with the weighted
    loss, at the bars tests/test_cpu_twins.py applies at the defaults (1e-5 of
    the tensor's scale for states and both gradients, 1e-5 for the loss)."""
    B = 200
    w = C.weight_sets(C.rollout_key(B, H))[wname]
    want = C.rollout_oracle(B, H, w)
    s0, a, ref = (t.numpy() for t in C.rollout_batch(B, H))
    got = T._quad_rollout(tw, s0, a, ref, C.ROLLOUT_DT, C.MOD, layout,
                          weights=C.capi_weights(w))
    assert rel_err(got["states"], want["states"]) < 1e-5
    assert abs(got["loss"] - want["loss"]) < 1e-5 * want["loss"]
    assert _tensor_err(got["ga"], want["grad_actions"]) < 1e-5
    assert _tensor_err(got["gs"], want["grad_state0"]) < 1e-5
    assert got["partials"].shape == want["partials"].shape
    assert np.abs(got["partials"] - want["partials"]).max() < 1e-5 * want["partials"].max()
    assert abs(got["partials"].sum() - got["loss"]) <= 1e-6 * abs(got["loss"])


@pytest.fixture(scope="module")
def mpc_tw():
    return R.twins()


@pytest.mark.parametrize("wname", list(C.NAMES) + ["balanced"])
def test_mpc_twin_under_the_weight_sets(mpc_tw, wname):
    """apg_quad_mpc_solve_cpu against the restatement with the same weights,
    under the arbiter of tests/test_quad_mpc_cpu.py (check_solve)."""
    w = C.weight_sets("mpc")[wname]
    s0, ref, u0 = C.mpc_inputs()
    got = R.twin_solve(mpc_tw, s0, ref, u0, C.MPC_DT, C.MPC_ITERS, weights=w)
    check_solve(got, C.mpc_restated(w, F32), C.mpc_restated(w, F64), f"twin {wname}")
