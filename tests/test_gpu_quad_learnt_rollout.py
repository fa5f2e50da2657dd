"""The fused rollout through the learnt quadrotor simulator on the GPU
(csrc/quad.hip: apg_quad_learnt_rollout_fwd_bwd, quad_learnt_rollout_kernel -
H x (4 x 4 action transform + Flightmare step + the 16 -> 64 -> 12 residual) +
quad_mpc_loss + the reverse sweep in one launch) against
oracle.torch_port.LearntQuadOracle in float64, per trajectory, the float32
oracle being the yardstick for rounding (conftest.assert_no_worse_than_fp32 with
its default factors); across the 64 KB step of its dynamic LDS stash (H = 21 /
22) up to APG_MAX_HORIZON = 48; small and ragged batches; optional outputs;
canaries behind every output; live weights under a captured graph.

Cases, inputs and the ReLU-kink rule: tests/quad_loss_cases.py (conditions held
by tests/test_quad_loss_cases_cpu.py).  test_gpu_trainers.py's
test_learnt_rollout_kernel_matches_autograd_unroll pins the kernel to the
MODULE's forward; this file pins it to float64."""
import numpy as np
import pytest
import torch

import quad_loss_cases as C
from conftest import assert_no_worse_than_fp32, per_trajectory_err, rel_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
KEYS = ("loss", "loss_partials", "grad_actions", "grad_state0", "states")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def device_inputs(B, H, layout, ref_cols, dev):
    from apg_trajectory_tracking_amd import synthetic as sy
    s0, a, ref = C.learnt_batch(B, H)
    if ref_cols == 6:
        ref = C.packed_ref(ref)
    if layout == "soa":
        s0, a, ref = sy.to_soa_state(s0), sy.to_soa_seq(a), sy.to_soa_seq(ref)
    return s0.to(dev), a.to(dev), ref.to(dev)


def fused(dyn, args, layout, **kw):
    from apg_trajectory_tracking_amd import functional as F
    kw.setdefault("want_states", True)
    return F.quad_learnt_rollout_fwd_bwd(dyn, *args, C.learnt_dt(), layout=layout, **kw)


def as_aos(res, layout):
    """-> dict of float64 numpy arrays in the oracle's shapes."""
    from apg_trajectory_tracking_amd import synthetic as sy
    seq = sy.from_soa_seq if layout == "soa" else (lambda t: t)
    vec = sy.from_soa_state if layout == "soa" else (lambda t: t)
    n = lambda t: t.detach().double().cpu().numpy()
    return dict(loss=float(res["loss"]), partials=n(res["loss_partials"]),
                states=n(seq(res["states"])), grad_actions=n(seq(res["grad_actions"])),
                grad_state0=n(vec(res["grad_state0"])))


def measure(dev, which, H, layout, ref_cols):
    """One arbiter case at B = 1003 -> (device result, float32 oracle, float64
    oracle, rows kept for the gradient comparisons, tag)."""
    B = C.LEARNT_B
    f64 = C.learnt_oracle(which, B, H)        # (packed reference rows: the same numbers)
    f32 = C.learnt_oracle(which, B, H, C.DEFAULT, F32)
    got = as_aos(fused(C.learnt_module(which, dev),
                       device_inputs(B, H, layout, ref_cols, dev), layout), layout)
    return got, f32, f64, ~f64["kink"], f"{which}/H{H}/{layout}/ref{ref_cols}"


def arbiter_case(dev, which, H, layout, ref_cols):
    got, f32, f64, keep, tag = measure(dev, which, H, layout, ref_cols)
    assert np.isfinite(got["states"]).all() and np.isfinite(got["grad_actions"]).all()
    assert_no_worse_than_fp32(got["states"], f32["states"], f64["states"], tag + " states")
    for k in ("grad_actions", "grad_state0"):
        assert_no_worse_than_fp32(got[k][keep], f32[k][keep], f64[k][keep], f"{tag} {k}")
    # the loss: every wave's partial, dead lanes of the last wave adding nothing
    parts = got["partials"]
    assert parts.shape == ((C.LEARNT_B + 63) // 64,)
    e_parts = float((np.abs(parts - f64["partials"]) / f64["partials"]).max())
    e_loss = abs(got["loss"] - f64["loss"]) / f64["loss"]
    print(tag, "loss", float("%.3g" % e_loss), "partials", float("%.3g" % e_parts))
    assert e_loss < 1e-5 and e_parts < 1e-5
    assert abs(got["loss"] - parts.sum()) < 1e-6 * parts.sum()


ARBITER = ([(w, H, lay, 9) for w, H in C.LEARNT_CASES for lay in ("aos", "soa")]
           + [(w, H, lay, 6) for w in ("golden", "steps") for H in (10, 22)
              for lay in ("aos", "soa")])


@pytest.mark.parametrize("which,H,layout,ref_cols", ARBITER)
def test_kernel_under_the_fp64_arbiter(dev, which, H, layout, ref_cols):
    """B = 1003 (16 workgroups, a ragged last wave).  H = 21: the last horizon
    whose stash fits 64 KB of LDS, H = 22 the first beyond (hipFuncSetAttribute),
    H = 48 the largest (144 KB).  States over all trajectories, dL/dactions and
    dL/dstate0 over those off a ReLU kink (quad_loss_cases.learnt_oracle_run)."""
    arbiter_case(dev, which, H, layout, ref_cols)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("which,H", [("steps", 10), ("steps", 22), ("strong", 5)])
def test_small_batches_are_rows_of_the_large_one(dev, which, H, layout):
    """B = 1 and B = 67 (a ragged second wave) are the first rows of the B =
    1003 inputs: a lane's arithmetic does not depend on the batch - every
    output row equals the large run's bit for bit, and is within 1e-4 per
    trajectory of float64."""
    dyn = C.learnt_module(which, dev)
    big = as_aos(fused(dyn, device_inputs(C.LEARNT_B, H, layout, 9, dev), layout), layout)
    f64 = C.learnt_oracle(which, C.LEARNT_B, H)
    for B in (1, 67):
        got = as_aos(fused(dyn, device_inputs(B, H, layout, 9, dev), layout), layout)
        keep = ~f64["kink"][:B]
        for k in ("states", "grad_actions", "grad_state0"):
            assert np.array_equal(got[k], big[k][:B]), (k, B)
            rows = slice(None) if k == "states" else keep
            e = per_trajectory_err(got[k][rows], f64[k][:B][rows])
            assert e.size == 0 or e.max() < 1e-4, (k, B, e.max())
        assert got["partials"].shape == ((B + 63) // 64,)
        if B >= 64:         # (a full first wave: the same 64 lanes, the same sum)
            assert got["partials"][0] == big["partials"][0]
        want_loss = f64["per_traj"][:B].sum()
        assert abs(got["loss"] - want_loss) < 1e-5 * want_loss


def test_optional_outputs_and_empty_batch(dev):
    B, H = 67, 10
    dyn = C.learnt_module("steps", dev)
    for layout in ("aos", "soa"):
        args = device_inputs(B, H, layout, 9, dev)
        full = fused(dyn, args, layout)
        bare = fused(dyn, args, layout, want_grad_state0=False, want_states=False)
        assert bare["grad_state0"] is None and bare["states"] is None
        assert torch.equal(bare["grad_actions"], full["grad_actions"])
        assert torch.equal(bare["loss"], full["loss"])
        assert torch.equal(bare["loss_partials"], full["loss_partials"])
    s0, a, ref = device_inputs(B, H, "aos", 9, dev)
    empty = fused(dyn, (s0[:0], a[:0], ref[:0]), "aos")
    assert float(empty["loss"]) == 0.0


@pytest.mark.parametrize("H", [10, 22])
@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_nothing_is_written_behind_an_output(dev, layout, H):
    """Every output handed in through `out=` as the head of a longer buffer
    filled with a sentinel (B = 67: 61 dead lanes in the second wave): the
    floats behind stay untouched, the outputs equal the plain call's bits."""
    B, pad, sentinel = 67, 4096, 7.0
    dyn = C.learnt_module("steps", dev)
    args = device_inputs(B, H, layout, 9, dev)
    plain = fused(dyn, args, layout)
    bufs, out = {}, {}
    for k in KEYS:
        n = plain[k].numel()
        bufs[k] = torch.full((n + pad,), sentinel, device=dev)
        out[k] = bufs[k][:n].view(plain[k].shape)
    res = fused(dyn, args, layout, out=out)
    for k in KEYS:
        assert res[k].data_ptr() == bufs[k].data_ptr(), k
        assert torch.all(bufs[k][plain[k].numel():] == sentinel), k
        assert torch.equal(res[k], plain[k]), k


def _oracle_of_module(dyn, B, H):
    weights = {k: v.detach().cpu().numpy() for k, v in dyn.state_dict().items()}
    return C.learnt_oracle_run(weights, B, H)


def test_live_weights_under_a_captured_graph(dev):
    """One call captured with `out=` (a linear chain of launches); then
    linear_state_2.weight and linear_at change IN PLACE and the replay equals a
    fresh float64 oracle built from the new values - the kernel reads the
    module's tensors when it runs, not when it was captured."""
    B, H = 67, 10
    for layout in ("aos", "soa"):
        dyn = C.learnt_module("steps", dev)
        args = device_inputs(B, H, layout, 9, dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = {k: v.clone() for k, v in fused(dyn, args, layout).items()}
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fused(dyn, args, layout, out=out)
        graph.replay()
        torch.cuda.synchronize()
        first = as_aos(out, layout)
        before = _oracle_of_module(dyn, B, H)
        g = torch.Generator().manual_seed(9)
        with torch.no_grad():
            dyn.linear_state_2.weight.mul_(3.0)
            dyn.linear_at.add_(0.1 * torch.randn(4, 4, generator=g).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        second = as_aos(out, layout)
        after = _oracle_of_module(dyn, B, H)
        for got, want, when in ((first, before, "before"), (second, after, "after")):
            keep = ~want["kink"]
            assert abs(got["loss"] - want["loss"]) < 1e-5 * want["loss"], when
            for k in ("states", "grad_actions", "grad_state0"):
                rows = slice(None) if k == "states" else keep
                e = per_trajectory_err(got[k][rows], want[k][rows]).max()
                assert e < 1e-4, (layout, when, k, e)
        moved = {k: rel_err(second[k], first[k]) for k in ("states", "grad_actions",
                                                            "grad_state0")}
        print("the change moved", layout, moved)
        assert min(moved.values()) > 1e-2, moved
