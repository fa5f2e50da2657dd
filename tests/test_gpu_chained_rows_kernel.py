"""The chained instantiation of quad_rollout_rows_kernel on the GPU: launches
of a two-lane chain (RolloutPlan(loss_mode="deferred"), packed layout) run a
kernel of their own - dL/dactions rows are written during the reverse sweep
instead of after it - and must give, bit for bit, what the eager entry point
(the serial instantiation) gives on the same tensors, and meet the float64
oracle at the packed rollout's tolerance.  Nothing is timed."""
import pytest
import torch

import chained_rows_cases as cc
from conftest import rel_err

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 5]     # launches of a chain
ROTATIONS = [2, 3]         # plans in rotation: 3 gives the cross-lane edge, a
#                            chain longer than the rotation relaunches a plan
#                            (the stand-alone reduction)
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def side(dev):
    return torch.cuda.Stream(device=dev)


def _packed(d, dev):
    from apg_trajectory_tracking_amd import synthetic as sy
    ref6 = torch.cat((d["ref"][:, :, :3], d["ref"][:, :, 6:9]), 2)
    return (sy.to_packed_state(d["state0"]).to(dev), sy.to_packed_seq(d["actions"]).to(dev),
            sy.to_packed_seq(ref6).to(dev))


OUTS = ("grad_actions", "grad_state0", "states")


def _run_case(kind, B, H, want_gs, want_st, dev, side):
    from apg_trajectory_tracking_amd import functional as F, synthetic as sy
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    dyn = FlightmareDynamics()
    kw = dict(layout="packed", want_grad_state0=want_gs, want_states=want_st)
    data = [_packed(cc.inputs(kind, B, H, p), dev) for p in range(cc.NPLANS)]
    want = [F.quad_rollout_fwd_bwd(*t, cc.DT, dyn.params, **kw) for t in data]
    torch.cuda.synchronize()
    # the eager entry point itself against the float64 oracle (once per case)
    for p, w in enumerate(want):
        o = cc.oracle64(kind, B, H, p)
        errs = {"grad_actions": rel_err(sy.from_packed_seq(w["grad_actions"]).cpu().numpy(),
                                        o["grad_actions"]),
                "loss": abs(w["loss"].item() - o["loss"]) / abs(o["loss"])}
        if want_gs:
            errs["grad_state0"] = rel_err(
                sy.from_packed_state(w["grad_state0"]).cpu().numpy(), o["grad_state0"])
        if want_st:
            errs["states"] = rel_err(sy.from_packed_seq(w["states"]).cpu().numpy(),
                                     o["states"])
            assert torch.isfinite(w["states"]).all()
        print("eager vs float64", kind, B, H, want_gs, want_st, p, errs)
        assert max(errs.values()) < cc.TOL, (p, errs)
    with torch.cuda.stream(side):
        plans = [F.RolloutPlan("quad", *(x.clone() for x in t), cc.DT, dyn.params,
                               loss_mode="deferred", **kw) for t in data]
    torch.cuda.synchronize()
    for p in plans:
        assert (p.out["grad_state0"] is not None) == want_gs
        assert (p.out.get("states") is not None) == want_st
    for nplans in ROTATIONS:
        for length in LENGTHS:
            for p in plans:
                p.out["loss"].fill_(-1.0)
                for k in OUTS:
                    if p.out.get(k) is not None:
                        p.out[k].fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                prev = None
                for i in range(length):
                    plans[i % nplans].launch(after=prev)
                    prev = plans[i % nplans]
                prev.flush()
            torch.cuda.synchronize()
            for i in range(min(length, nplans)):
                got, w, o = plans[i].out, want[i], cc.oracle64(kind, B, H, i)
                what = (kind, B, H, want_gs, want_st, nplans, length, i)
                for k in OUTS:
                    if w.get(k) is None:
                        assert got.get(k) is None, (k, what)
                    else:
                        assert torch.equal(got[k], w[k]), (k, what)
                wl = w["loss"].item()
                assert abs(got["loss"].item() - wl) <= 1e-6 * abs(wl), what
                # the chain's own outputs against the float64 oracle
                assert abs(got["loss"].item() - o["loss"]) / abs(o["loss"]) < cc.TOL, what
                assert rel_err(sy.from_packed_seq(got["grad_actions"]).cpu().numpy(),
                               o["grad_actions"]) < cc.TOL, what
                if want_gs:
                    assert rel_err(sy.from_packed_state(got["grad_state0"]).cpu().numpy(),
                                   o["grad_state0"]) < cc.TOL, what
                if want_st:
                    assert rel_err(sy.from_packed_seq(got["states"]).cpu().numpy(),
                                   o["states"]) < cc.TOL, what


POLY = [(B, H, gs, st) for H in cc.HORIZONS for B in cc.BATCHES for gs, st in FLAGS]


@pytest.mark.parametrize("B,H,want_gs,want_st", POLY,
                         ids=[f"B{B}-H{H}-gs{int(g)}-st{int(s)}" for B, H, g, s in POLY])
def test_chained_launches_equal_the_eager_entry_point_bit_for_bit(
        dev, side, B, H, want_gs, want_st):
    _run_case("poly", B, H, want_gs, want_st, dev, side)


@pytest.mark.parametrize("H", cc.HORIZONS)
@pytest.mark.parametrize("kind", ["large", "zero"])
def test_chained_launches_at_large_and_at_zero_attitudes(dev, side, kind, H):
    """large: initial attitudes spread up to |angle| ~ 1e4 rad, where sin / cos
    need the two-word range reduction (a schedule that computes them again in
    the reverse sweep must round alike at both sites); zero: attitudes exactly
    0."""
    _run_case(kind, cc.SPECIAL_B, H, True, True, dev, side)
