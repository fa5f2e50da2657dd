"""The batched closed-loop fixed-wing kernels (wing_closed_loop_kernel<false|true>)
on every case of tests/wing_flight_cases.py, held flight by flight and step by
step against the float64 restatement run with the kernel's own decisions
(wing_flight_cases.check): per-flight arbiter on position / velocity / attitude /
rates / actions / what the policy saw, each on its own scale; 2e-4 on the
distances; every pass and failure decision against float64; flight ends; nothing
written beyond them.  The conditions that make these cases able to fail are held
in tests/test_wing_flight_cases_cpu.py.  Then what needs no tolerance: the same
bits from launch to launch, the independence of a flight from the batch it flies
in, and the C ABI with each optional output NULL and guarded NaN buffers.

What these tests found (one MI355X, 30 cases x 2 environments; DESIGN.md,
closed-loop section).  Both kernels gave the same bits at every launch and for
every flight whatever the batch around it, wrote nothing outside their outputs
and took no decision that float64 contradicts - but 9 of the 60 case x
environment pairs missed the arbiter's factor 4 on the body rates' own scale
(once on the attitude's), by up to 1.65 x the bound: worst flight 1.9e-5 against
the float32 restatement's 6.2e-6.  One step of the environment on the kernel's
own inputs showed where: the lateral position came out 3 x as far from float64
as float32 arithmetic puts it (rms 4.6e-8 m against 1.4e-8 m), everything else
as close.  The hardware sine and cosine are exact to 1.5e-7 absolutely, which
at a heading of a few hundredths of a radian is 3e-6 of the sine; the flight
steers by the direction to a target that is half a metre away on the step
before a pass, and the rates answer.  wing_closed_loop_kernel now takes the
attitude's sine and cosine in software (wing_step<true>, csrc/wing_math.h):
worst flight kernel | float32, rates 1.4e-5 | 6.4e-6 and 6.7e-6 | 6.2e-6
(learnt), attitude 6.0e-6 | 6.1e-6, actions 8.3e-6 | 9.7e-6; at most 0.96 of
the arbiter's bound; distances within 9.9e-6; 187 753 decisions observed, 59 of
them inside the 2e-4 band, none contradicting float64 outside it.  With
wing_step<false> in the kernel the nine cases fail again."""
import ctypes

import numpy as np
import pytest
import torch

import wing_flight_cases as W

pytestmark = pytest.mark.gpu

OUTPUTS = ("div_linear", "div_pass", "div_fail", "steps", "drone", "seen")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _differing(a, b):
    """Number of entries of two tensors that are not the same bits."""
    if a.shape != b.shape:
        return -1
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return int((a != b).sum())


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("name", W.NAMES)
def test_every_flight_step_by_step_against_float64(dev, name, kind):
    case = W.get(name, kind)
    out = W.run_kernel(case, kind, dev)
    W.check(case, kind, W.kernel_log(out), blank=0.0)
    short = W.run_kernel(case, kind, dev, want_trajectory=False)
    assert set(short) == {"div_linear", "div_pass", "div_fail", "steps"}
    for k in short:
        assert _differing(short[k], out[k]) == 0, k


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("name", [W.FLAGSHIP, W.FLAGSHIP_TT1])
def test_three_launches_give_the_same_bits(dev, name, kind):
    case = W.get(name, kind)
    first = W.run_kernel(case, kind, dev)
    for again in range(2):
        out = W.run_kernel(case, kind, dev)
        for k in OUTPUTS:
            n = _differing(out[k], first[k])
            assert n == 0, (k, again, n, float((out[k] - first[k]).abs().max()))


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("name", [W.FLAGSHIP, W.FLAGSHIP_TT1])
def test_a_flight_does_not_depend_on_the_batch_around_it(dev, name, kind):
    """The B = 300 mixed case flown again with the flights permuted: every
    flight's log is bit-identical (a flight is one column of every matrix
    product; target switch, break and reset are per lane)."""
    case = W.get(name, kind)
    B = case.targets.shape[0]
    order = torch.randperm(B, generator=torch.Generator().manual_seed(12))
    assert (order // 32 != torch.arange(B) // 32).float().mean() > 0.8   # other waves
    out, moved = W.run_kernel(case, kind, dev), W.run_kernel(case, kind, dev, order=order)
    o = order.to(dev)
    for k in OUTPUTS:
        n = _differing(moved[k], out[k][..., o])
        assert n == 0, (k, n, float((moved[k] - out[k][..., o]).abs().max()))


# ------------------------------------------------------------------- C ABI
GUARD, EXTRA = 2, 2        # guard planes before / after; rows allocated beyond T
COLS = dict(div_linear=1, div_pass=1, div_fail=1, drone=16, seen=15)
STEPS_FILL = -7


def _abi_flight(case, kind, dev, skip=()):
    """apg_wing_mlp_closed_loop on NaN-filled buffers with guard planes around
    them and EXTRA rows beyond T; `skip`: the optional outputs handed over as
    NULL.  -> {name: whole buffer}, steps buffer."""
    from apg_trajectory_tracking_amd import _capi
    net, dyn = W.device_fixtures(str(dev))
    d = W.data()
    B, n_t, _ = case.targets.shape
    T = case.max_steps
    tg = case.targets.float().permute(1, 2, 0).contiguous().to(dev)
    s0 = None if case.state0 is None else case.state0.float().t().contiguous().to(dev)
    full = {k: torch.full((GUARD + (T + EXTRA) * c + GUARD, B), float("nan"), device=dev)
            for k, c in COLS.items() if k not in skip}
    steps = torch.full((GUARD + 1 + GUARD, B), STEPS_FILL, dtype=torch.int32, device=dev)
    at = lambda k: full[k][GUARD:].data_ptr() if k in full else None
    names = ("w_s", "b_s", "w_r", "b_r", "w_1", "b_1", "w_2", "b_2", "w_3", "b_3", "w_out",
             "b_out")
    vals = (net.states_in.weight, net.states_in.bias, net.ref_in.weight, net.ref_in.bias,
            net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias, net.fc3.weight,
            net.fc3.bias, net.fc_out.weight, net.fc_out.bias)
    pw = {k: v.detach().float().contiguous() for k, v in zip(names, vals)}
    pol = _capi.ApgWingPolicy(**{k: v.data_ptr() for k, v in pw.items()})
    f12 = ctypes.c_float * 12
    params, I9, model = W.analytic_params(case), None, None
    if kind == "wing_learnt":
        host = torch.cat((dyn._theta().detach().reshape(-1).float(),
                          dyn.I.detach().reshape(-1).float())).cpu().tolist()
        params, I9 = _capi.ApgWingParams(*host[:41]), (ctypes.c_float * 9)(*host[41:])
        res = [dyn.linear_state_1.weight, dyn.linear_state_1.bias, dyn.linear_state_2.weight,
               dyn.linear_state_2.bias]
        model = _capi.ApgLearntResidual(None, *[t.data_ptr() for t in res])
    lib = _capi.lib()
    ws = torch.zeros(lib.apg_wing_policy_workspace_floats(), device=dev)
    flight = _capi.ApgWingFlight(
        targets=tg.data_ptr(), state0=None if s0 is None else s0.data_ptr(), n_targets=n_t,
        max_steps=T, thresh_div=case.thresh_div, thresh_stable=case.thresh_stable,
        test_time=case.test_time, div_linear=at("div_linear"), div_pass=at("div_pass"),
        div_fail=at("div_fail"), steps=steps[GUARD:].data_ptr(), drone=at("drone"),
        seen=at("seen"))
    code = lib.apg_wing_mlp_closed_loop(
        ctypes.byref(flight), d["dt"], ctypes.byref(params),
        I9, None if model is None else ctypes.byref(model), ctypes.byref(pol),
        f12(*d["mean"].tolist()), f12(*d["std"].tolist()), d["data_dt"], d["data_horizon"], B,
        ws.data_ptr(), _capi.stream_of(tg))
    _capi.check(code, kind)
    torch.cuda.synchronize(dev)
    return full, steps


def _abi_log(case, full, steps):
    """The guarded buffers' views as a flight-leading log, after the guards and
    the rows beyond T were found untouched."""
    T = case.max_steps
    log = {}
    for k, buf in full.items():
        used = T * COLS[k]
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + used:]).all(), \
            (k, "wrote outside its view")
        view = buf[GUARD:GUARD + used].view(T, COLS[k], buf.shape[1])
        log[k] = view.permute(2, 0, 1).cpu().numpy()
        if COLS[k] == 1:
            log[k] = log[k][:, :, 0]
    assert (steps[:GUARD] == STEPS_FILL).all() and (steps[GUARD + 1:] == STEPS_FILL).all(), \
        "steps: wrote outside its view"
    log["steps"] = steps[GUARD].cpu().numpy().astype(np.int64)
    return log


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("name", [f"B33-n3-steps{W.T_FULL}-mixed-tt1",
                                  f"B257-n3-steps{W.T_FULL}-mixed-tt0", W.FLAGSHIP_TT1])
def test_c_abi_optional_outputs_and_guarded_buffers(dev, name, kind):
    """Entries after a flight's end, rows beyond T and the guard planes keep
    their NaN (check: blank = NaN); an optional output that is NULL changes no
    bit of the others."""
    case = W.get(name, kind)
    whole = _abi_flight(case, kind, dev)
    W.check(case, kind, _abi_log(case, *whole), blank=float("nan"))
    for skip in (("drone",), ("seen",), ("drone", "seen")):
        full, steps = _abi_flight(case, kind, dev, skip=skip)
        _abi_log(case, full, steps)
        assert set(full) == set(COLS) - set(skip)
        for k, buf in full.items():
            assert _differing(buf, whole[0][k]) == 0, (skip, k)
        assert torch.equal(steps, whole[1]), skip
