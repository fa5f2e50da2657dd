"""Every batched closed-loop quadrotor kernel (mlp_closed_loop_kernel<false|true>,
lstm_closed_loop_kernel<false|true>) on every case of tests/quad_flight_cases.py,
held flight by flight and step by step against the float64 restatement run
with the kernel's own decisions (quad_flight_cases.check): per-flight arbiter
on drone / actions / start_states / div, 2e-4 on the divergences, every decision
against float64, flight ends, nothing written beyond them.  The conditions that
make these cases able to fail are held in tests/test_quad_flight_cases_cpu.py.
Then the C ABI with each optional output NULL and guarded NaN buffers, and the
independence of a flight from the batch it flies in.

The first case of this file caught mlp_closed_loop_kernel differing from launch
to launch in waves 4..7 of a workgroup (actions up to 3.3e-6 off, 11 x the
float32 restatement's error on the states): the assembly statement of
split_pair (csrc/policy_mfma16.h) next to the matrix instructions; the
closed-loop kernels split without it now (closed-loop section)."""
import ctypes

import numpy as np
import pytest
import torch

import quad_flight_cases as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("name", list(Q.CASES))
def test_every_flight_step_by_step_against_float64(dev, name, kind):
    case = Q.CASES[name]
    out = Q.run_kernel(case, kind, dev)
    Q.check(case, kind, Q.kernel_log(out), blank=0.0)
    short = Q.run_kernel(case, kind, dev, want_trajectory=False)
    assert set(short) == {"div", "steps"}
    assert _same_bits(short["div"], out["div"]) and torch.equal(short["steps"], out["steps"])


# ------------------------------------------------------------------- C ABI
GUARD, EXTRA = 2, 2        # guard planes before / after; rows allocated beyond T
COLS = dict(div=1, drone=12, actions=4, start_states=12)
STEPS_FILL = -7


def _abi_flight(case, kind, dev, skip=None):
    """apg_quad_mlp_closed_loop / apg_quad_lstm_closed_loop on NaN-filled
    buffers with guard planes around them and EXTRA rows beyond T; `skip`: the
    optional output handed over as NULL.  -> {name: whole buffer}, steps buffer."""
    from apg_trajectory_tracking_amd import _capi, functional as F
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    _, net, lstm, _, dyn = Q.device_fixtures(str(dev))
    B, L, _ = case.traj.shape
    T = Q.case_T(case)
    tr = case.traj.float().permute(1, 2, 0).contiguous().to(dev)
    rows = {k: (T + EXTRA + (k == "drone")) * c for k, c in COLS.items()}
    full = {k: torch.full((GUARD + rows[k] + GUARD, B), float("nan"), device=dev)
            for k in COLS if k != skip}
    steps = torch.full((GUARD + 1 + GUARD, B), STEPS_FILL, dtype=torch.int32, device=dev)
    at = lambda k: full[k][GUARD:].data_ptr() if k in full else None
    flight = _capi.ApgQuadFlight(tr.data_ptr(), L, case.max_steps, case.thresh_div,
                                 case.thresh_stable, case.test_time, at("div"),
                                 steps[GUARD:].data_ptr(), at("drone"), at("actions"),
                                 at("start_states"))
    learnt = dyn if kind.endswith("learnt") else None
    env, _keep = F._learnt_env(learnt)
    params = dyn.params if learnt is not None else FlightmareDynamics().params
    lib, stream = _capi.lib(), _capi.stream_of(tr)
    if kind.startswith("lstm"):
        pw = dict(conv_w=lstm.conv_ref.weight, conv_b=lstm.conv_ref.bias,
                  w_ih=lstm.lstm.weight_ih, w_hh=lstm.lstm.weight_hh,
                  b_ih=lstm.lstm.bias_ih, b_hh=lstm.lstm.bias_hh,
                  w_out=lstm.fc_out.weight, b_out=lstm.fc_out.bias)
        pw = {k: v.detach().float().contiguous() for k, v in pw.items()}
        pol = _capi.ApgLstmPolicy(**{k: v.data_ptr() for k, v in pw.items()})
        h0, c0 = F.to_soa(case.h0.to(dev)), F.to_soa(case.c0.to(dev))
        ws = torch.zeros(lib.apg_quad_lstm_workspace_floats(), device=dev)
        code = lib.apg_quad_lstm_closed_loop(
            ctypes.byref(flight), h0.data_ptr(), c0.data_ptr(), Q.DT, ctypes.byref(params),
            env, ctypes.byref(pol), B, 10, ws.data_ptr(), stream)
    else:
        pol, pw = F._mlp_policy(net)
        ws = torch.zeros(lib.apg_quad_mlp_workspace_floats(), device=dev)
        code = lib.apg_quad_mlp_closed_loop(
            ctypes.byref(flight), Q.DT, ctypes.byref(params), env, ctypes.byref(pol), B, 10,
            ws.data_ptr(), stream)
    _capi.check(code, kind)
    torch.cuda.synchronize(dev)
    return full, steps


def _abi_log(case, full, steps):
    """The guarded buffers' views as a flight-leading log, after the guards and
    the rows beyond T were found untouched."""
    T = Q.case_T(case)
    log = {}
    for k, buf in full.items():
        used = (T + (k == "drone")) * COLS[k]
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + used:]).all(), \
            (k, "wrote outside its view")
        view = buf[GUARD:GUARD + used].view(-1, COLS[k], buf.shape[1])
        log[k] = view.permute(2, 0, 1).cpu().numpy()
    if "div" in log:
        log["div"] = log["div"][:, :, 0]
    assert (steps[:GUARD] == STEPS_FILL).all() and (steps[GUARD + 1:] == STEPS_FILL).all(), \
        "steps: wrote outside its view"
    log["steps"] = steps[GUARD].cpu().numpy().astype(np.int64)
    return log


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("name", ["B129-L24-steps25-mixed-tt1", "B257-L24-steps25-mixed-tt0",
                                  "B70-L12-steps19-mixed-tt1"])
def test_c_abi_optional_outputs_and_guarded_buffers(dev, name, kind):
    """Entries after a flight's end, rows beyond T and the guard planes keep
    their NaN (check: blank = NaN); an optional output that is NULL changes no
    bit of the others."""
    case = Q.CASES[name]
    whole = _abi_flight(case, kind, dev)
    Q.check(case, kind, _abi_log(case, *whole), blank=float("nan"))
    for skip in ("drone", "actions", "start_states"):
        full, steps = _abi_flight(case, kind, dev, skip=skip)
        _abi_log(case, full, steps)
        assert set(full) == set(COLS) - {skip}
        for k, buf in full.items():
            assert _same_bits(buf, whole[0][k]), (skip, k)
        assert torch.equal(steps, whole[1]), skip


# ------------------------------------------------------- batch composition
@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("name", [Q.FLAGSHIP, "B300-L40-steps41-mixed-tt1"])
def test_a_flight_does_not_depend_on_the_batch_around_it(dev, name, kind):
    """The B = 300 mixed case flown again with the flights permuted: every
    flight's log is bit-identical (a flight is one column of every matrix
    product, the reset a per-lane select)."""
    case = Q.CASES[name]
    B = case.traj.shape[0]
    order = torch.randperm(B, generator=torch.Generator().manual_seed(12))
    assert (order // 32 != torch.arange(B) // 32).float().mean() > 0.8   # other waves
    out, moved = Q.run_kernel(case, kind, dev), Q.run_kernel(case, kind, dev, order=order)
    o = order.to(dev)
    for k in ("div", "steps", "drone", "actions", "start_states"):
        a, b = moved[k], out[k][..., o]
        if k == "steps":
            assert torch.equal(a, b)
        else:
            differ = (a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32))
            assert not differ.any(), (k, int(differ.sum()), float((a - b).abs().max()))
