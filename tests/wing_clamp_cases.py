"""Inputs, references and judges for the fixed-wing clamp tests
(test_wing_clamps_cpu.py, test_gpu_wing_clamps.py).

Every fixed-wing kernel computes alpha = clamp(atan(w / u), +-10 deg) and
beta = clamp(atan(v / V), +-10 deg) through csrc/wing_math.h (atan_clamped with
its arithmetic `free` mask, rcp_nr_finite(u), a dead gradient where a clamp is
active).  The suite's other inputs hardly ever reach a clamp; the ones built
here sit on both sides of both bounds, cross them along a rollout, come within
0.1 % of them and include u <= 0.

A helper module, not a conftest: it holds no fixture and changes no setting.
References are computed once per case, shared between the tests and never
written to."""
import math

import numpy as np
import torch

from conftest import load_golden, per_trajectory_err

DT = 0.05
BAR = 1e-4                                   # BASELINE.json north_star, per trajectory
TAN_BOUND = math.tan(math.radians(10.0))     # the bound on w / u and v / V
WMOD = {"mass": 1.4, "I_xz": -0.01, "CL0": 0.3, "rho": 1.0}   # as test_gpu_parity
PARAMS = {"def": {}, "mod": WMOD}
RESIDUAL = ("linear_state_1.weight", "linear_state_1.bias",
            "linear_state_2.weight", "linear_state_2.bias")


# ---------------------------------------------------------------- inputs
def clamp_batch(B, H, dt, seed):
    """synthetic.wing_batch(B, H, dt, seed) with v, w of state0 rewritten so
    that r_a = w / u and r_b = v / V - the ratios whose arc tangents the
    reference clamps - are uniform on +-2.5 tan(10 deg); trajectories with
    b % 4 == 1 keep r_a, those with b % 4 == 2 keep r_b within +-0.5 tan(10 deg):
    each clamp is seen alone, with the other and not at all.  u, position,
    attitude, rates, actions and ref are wing_batch's."""
    from apg_trajectory_tracking_amd import synthetic
    d = synthetic.wing_batch(B, H, dt, seed)
    g = torch.Generator().manual_seed(7919 + seed)
    b = torch.arange(B)
    span_a = torch.where(b % 4 == 1, 0.5, 2.5).double() * TAN_BOUND
    span_b = torch.where(b % 4 == 2, 0.5, 2.5).double() * TAN_BOUND
    r_a = (2 * torch.rand(B, generator=g, dtype=torch.float64) - 1) * span_a
    r_b = (2 * torch.rand(B, generator=g, dtype=torch.float64) - 1) * span_b
    state0 = d["state0"].clone()
    u = state0[:, 3].double()
    w = r_a * u
    v = r_b * torch.sqrt((u * u + w * w) / (1 - r_b * r_b))   # v / V = r_b
    state0[:, 4], state0[:, 5] = v.float(), w.float()
    return dict(d, state0=state0)


def ratios(states):
    """(w / u, v / V), each in units of tan(10 deg), of states [..., 12]
    (float64 numpy): beyond +-1 the clamp is active."""
    s = np.asarray(states, np.float64)
    u, v, w = s[..., 3], s[..., 4], s[..., 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (w / u) / TAN_BOUND, (v / np.sqrt(u * u + v * v + w * w)) / TAN_BOUND


def pre_states(state0, states):
    """[B, H, 12]: the state every step of a rollout starts from."""
    s0 = np.asarray(state0, np.float64)[:, None]
    return np.concatenate((s0, np.asarray(states, np.float64)[:, :-1]), 1)


def near_kink(pre_states64, delta=1e-4):
    """Mask [B] of the trajectories with a pre-step state of the float64 oracle
    within `delta` (relative) of a clamp bound, for either angle: there float32
    arithmetic may legitimately take the other branch.  They are left out of
    the accuracy assertions (never out of the finiteness ones)."""
    pre = np.asarray(pre_states64, np.float64)
    pre = pre.reshape(pre.shape[0], -1, 12)
    ra, rb = ratios(pre)
    return ((np.abs(np.abs(ra) - 1) < delta) | (np.abs(np.abs(rb) - 1) < delta)).any(1)


def clamp_stats(pre_states64):
    """Shares of steps with an active alpha / beta clamp, of trajectories with
    any clamp, and of trajectories whose alpha clamp is active on some steps
    and inactive on others."""
    pre = np.asarray(pre_states64, np.float64)
    pre = pre.reshape(pre.shape[0], -1, 12)
    ra, rb = ratios(pre)
    ca, cb = np.abs(ra) > 1, np.abs(rb) > 1
    return dict(alpha_steps=float(ca.mean()), beta_steps=float(cb.mean()),
                any_clamp=float((ca | cb).any(1).mean()),
                alpha_partial=float((ca.any(1) & ~ca.all(1)).mean()),
                beta_partial=float((cb.any(1) & ~cb.all(1)).mean()))


def assert_coverage(pre_states64, what, rollout=True):
    """The conditions every clamp test states about its own input: at most 1 %
    of the batch excluded as near a kink; at least 5 % of the steps clamped for
    each angle; for rollouts at least 20 % of the trajectories with the alpha
    clamp on some steps but not all.  Returns the mask of KEPT trajectories."""
    skip = near_kink(pre_states64)
    st = clamp_stats(pre_states64)
    print(what, "clamp coverage:", {k: round(v, 4) for k, v in st.items()},
          "near a kink: %d of %d" % (skip.sum(), len(skip)))
    assert skip.mean() <= 0.01, (what, skip.mean())
    assert st["alpha_steps"] >= 0.05 and st["beta_steps"] >= 0.05, (what, st)
    if rollout:
        assert st["alpha_partial"] >= 0.20, (what, st)
    return ~skip


# explicit single-step rows --------------------------------------------------
N_RANDOM = 232          # clamp_batch part of step_cases()


def step_cases():
    """dict(state [N,12], action [N,4], ref_state [N,12], zero_u [N] bool): the
    clamp_batch(N_RANDOM, 1) states followed by explicit rows -
      * |r_a| and |r_b| at (1 +- 1e-2) and (1 +- 1e-3) x the bound, both signs,
        each angle alone (the other ratio at 0.3 x the bound): 32 rows;
      * u ~ -12 in the four clamp states: 4 rows;
      * u = +0.0 and u = -0.0 with w = +-3: 4 rows.  `ref_state` carries
        u = +-1e-9 there (zero_u marks them): the reference's own gradient at
        u = 0 is NaN (0 x inf), the kernels' contract is alpha = +-bound with a
        dead gradient, which is what the reference computes next to 0.
    u = v = w = 0 is NaN in the reference itself and is not a case."""
    d = clamp_batch(N_RANDOM, 1, DT, seed=77)
    state, action = d["state0"].double(), d["actions"][:, 0].double()
    g = torch.Generator().manual_seed(78)
    rows = []

    def row(u, r_a, r_b):
        s = torch.zeros(12, dtype=torch.float64)
        s[6:12] = 0.05 * torch.randn(6, generator=g, dtype=torch.float64)
        w = r_a * TAN_BOUND * u
        s[3], s[5] = u, w
        rb = r_b * TAN_BOUND
        s[4] = rb * math.sqrt((u * u + w * w) / (1 - rb * rb))
        rows.append(s)
    for f in (1 - 1e-2, 1 - 1e-3, 1 + 1e-3, 1 + 1e-2):
        for sign in (1.0, -1.0):
            for u in (11.3, 12.2):
                row(u, sign * f, 0.3)
                row(u, -0.3, sign * f)
    for r_a, r_b in ((0.4, -0.5), (1.8, 0.5), (-0.4, 1.7), (-2.1, -1.6)):
        row(-12.0, r_a, r_b)
    extra = torch.stack(rows)
    zero = torch.zeros(4, 12, dtype=torch.float64)
    zero[:, 6:12] = 0.05 * torch.randn(4, 6, generator=g, dtype=torch.float64)
    zero[:, 3] = torch.tensor([0.0, -0.0, 0.0, -0.0], dtype=torch.float64)
    zero[:, 5] = torch.tensor([3.0, 3.0, -3.0, -3.0], dtype=torch.float64)
    zero[:, 4] = torch.tensor([0.2, -2.0, 1.5, -0.3], dtype=torch.float64)
    state = torch.cat((state, extra, zero)).float()
    n_extra = extra.shape[0] + 4
    action = torch.cat((action, torch.rand(n_extra, 4, generator=g,
                                           dtype=torch.float64))).float()
    zero_u = torch.zeros(state.shape[0], dtype=torch.bool)
    zero_u[-4:] = True
    ref_state = state.clone()
    ref_state[-4:, 3] = torch.tensor([1e-9, -1e-9, 1e-9, -1e-9])
    assert torch.equal(torch.signbit(state[-4:, 3]),
                       torch.tensor([False, True, False, True]))
    return dict(state=state, action=action, ref_state=ref_state, zero_u=zero_u.numpy())


# ------------------------------------------------------ column-wise Jacobian
def stack_one_hot(state, action):
    """The case set 12 times with the 12 one-hot cotangents of the next state:
    one backward call then yields d next / d (state, action) for every sample.
    -> state [12 N, 12], action [12 N, 4], cot [12 N, 12] (copy j: e_j)."""
    N = state.shape[0]
    cot = torch.zeros(12, N, 12, dtype=state.dtype)
    for j in range(12):
        cot[j, :, j] = 1
    return state.repeat(12, 1), action.repeat(12, 1), cot.reshape(12 * N, 12)


def unstack_jacobian(grad_state, grad_action):
    """[12 N, 12], [12 N, 4] of a stack_one_hot batch -> J [N, 12, 16]:
    J[b, o, i] = d next_o / d (state, action)_i of sample b."""
    gs = np.asarray(grad_state, np.float64).reshape(12, -1, 12)
    ga = np.asarray(grad_action, np.float64).reshape(12, -1, 4)
    return np.concatenate((gs, ga), 2).transpose(1, 0, 2)


def column_errors(J, J64):
    """err[o, i] = max_b |J - J64| / max_b |J64| for every (output, input)
    column; a column that is zero in float64 is compared absolutely."""
    scale = np.abs(J64).max(0)
    return np.abs(J - J64).max(0) / np.where(scale > 0, scale, 1.0)


def assert_columns_no_worse_than_fp32(dev, f32, f64, what):
    """conftest.assert_no_worse_than_fp32 with its defaults, the 192 (output,
    input) columns of a step Jacobian [N, 12, 16] in the place of trajectories:
    its error measure is then max_b |J - J64| / max_b |J64| per column, and a
    column that is zero in float64 has to be zero.  Each side's own worst
    column is compared, as there.  Also prints the worst column and the largest
    column-by-column ratio (with the function's floor under the float32 error).
    Measured on the MI355X: 2.4e-6 in columns (6, 10), d phi' / d q = dt sin(phi)
    tan(theta), and (4, 7), d v' / d theta = -dt g sin(phi) sin(theta) - both
    second order in attitude angles of at most 0.15 rad, where the hardware
    sin / cos pair is accurate to 1.5e-7 ABSOLUTELY (csrc/apg_device.h) and libm
    relatively; the float32 oracle's worst column: 1.3e-6 with the default,
    5.7e-7 with the modified parameters; the host build: 1.3e-6 / 5.5e-7
    (DESIGN.md 3.3)."""
    from conftest import assert_no_worse_than_fp32
    e_dev, e_f32 = column_errors(dev, f64), column_errors(f32, f64)
    o, i = np.unravel_index(np.argmax(e_dev), e_dev.shape)
    ratio = e_dev / np.maximum(e_f32, 1e-6)
    ro, ri = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("per column:", dict(what=what, worst_dev=float("%.3g" % e_dev.max()),
                              worst_column=(int(o), int(i)),
                              worst_f32=float("%.3g" % e_f32.max()),
                              worst_ratio=float("%.3g" % ratio.max()),
                              worst_ratio_column=(int(ro), int(ri))))
    assert np.all(np.isfinite(dev)), what
    cols = lambda J: np.asarray(J).transpose(1, 2, 0).reshape(12 * 16, -1)
    return assert_no_worse_than_fp32(cols(dev), cols(f32), cols(f64), what)


def assert_close_per_trajectory(got, want, what, bar=BAR):
    e = per_trajectory_err(got, want)
    print(what, "per-trajectory worst %.3g" % e.max())
    assert np.all(np.isfinite(np.asarray(got))) and e.max() < bar, (what, e.max())
    return e


# -------------------------------------------------------- analytic references
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _np(t, dtype=np.float32):
    return np.ascontiguousarray(t.numpy() if torch.is_tensor(t) else t, dtype)


def step_reference(tag):
    """Next state and Jacobian [N, 12, 16] of step_cases() in float64 and
    float32 (u = +-1e-9 in place of +-0), and the kept rows.  `tag` def / mod:
    the analytic step by the C oracle; w / steps: LearntWingOracle on that
    recorded weight set, by autograd."""
    def make():
        c = step_cases()
        S, A, cot = stack_one_hot(c["ref_state"], c["action"])
        out = dict(cases=c)
        for name, dt_ in (("f64", np.float64), ("f32", np.float32)):
            if tag in PARAMS:
                from oracle import c_oracle as co
                nxt = co.wing_step(_np(c["ref_state"]), _np(c["action"]), DT, PARAMS[tag],
                                   dtype=dt_)
                gs, ga = co.wing_step_vjp(_np(S), _np(A), DT, _np(cot), PARAMS[tag],
                                          dtype=dt_)
            else:
                from oracle import torch_port as tp
                dtype = torch.float64 if dt_ == np.float64 else torch.float32
                ora = tp.LearntWingOracle(learnt_weights(tag), dtype=dtype)
                s = S.clone().to(dtype).requires_grad_(True)
                a = A.clone().to(dtype).requires_grad_(True)
                nxt = ora(s, a, DT)
                gs, ga = (g.numpy() for g in torch.autograd.grad(nxt, (s, a), cot.to(dtype)))
                nxt = nxt.detach().numpy()[:c["state"].shape[0]]
            assert np.all(np.isfinite(nxt)) and np.all(np.isfinite(gs)), (tag, name)
            out["next_" + name] = nxt
            out["J_" + name] = unstack_jacobian(gs, ga)
        out["keep"] = assert_coverage(_np(c["ref_state"], np.float64)[:, None],
                                      "step cases", rollout=False)
        ra, rb = ratios(_np(c["ref_state"], np.float64))
        assert (np.abs(np.abs(ra) - 1) < 2e-3).sum() >= 8      # the near-bound rows
        assert (np.abs(np.abs(rb) - 1) < 2e-3).sum() >= 8
        assert (c["ref_state"][:, 3] < -1).sum() >= 4
        assert out["keep"][-40:].all()     # no explicit row is itself within delta
        return out
    return _cached(("step", tag), make)


def check_step(run, tag, what):
    """`run(state, action, cot or None) -> (next, grad_state, grad_action)` on
    float32 arrays: the next states per trajectory and per component, every
    (output, input) column of the Jacobian, from one stacked batch of one-hot
    cotangents; `tag`: see step_reference."""
    ref = step_reference(tag)
    c, keep = ref["cases"], ref["keep"]
    from conftest import assert_no_worse_than_fp32
    S, A, cot = stack_one_hot(c["state"], c["action"])
    nxt, gs, ga = run(S.numpy(), A.numpy(), cot.numpy())
    N = c["state"].shape[0]
    nxt = np.asarray(nxt).reshape(12, N, 12)
    assert np.array_equal(nxt[0], nxt[11])
    J = unstack_jacobian(gs, ga)
    assert np.all(np.isfinite(nxt)) and np.all(np.isfinite(J)), what
    assert_no_worse_than_fp32(nxt[0][keep], ref["next_f32"][keep], ref["next_f64"][keep],
                              what + " next")
    assert_no_worse_than_fp32(nxt[0][keep].T, ref["next_f32"][keep].T, ref["next_f64"][keep].T,
                              what + " next, per column")
    assert_columns_no_worse_than_fp32(J[keep], ref["J_f32"][keep], ref["J_f64"][keep],
                                      what + " Jacobian")
    # u = +-0: alpha = +-bound with a dead gradient, as the reference next to 0
    z = c["zero_u"]
    assert z.sum() == 4
    assert_close_per_trajectory(nxt[0][z], ref["next_f64"][z], what + " next at u = +-0")
    assert_close_per_trajectory(J[z][:, :, :12], ref["J_f64"][z][:, :, :12],
                                what + " d/dstate at u = +-0")
    assert_close_per_trajectory(J[z][:, :, 12:], ref["J_f64"][z][:, :, 12:],
                                what + " d/daction at u = +-0")


def rollout_reference(B, H, tag, seed=None):
    """clamp_batch(B, H) and its rollout by the C oracle: f64 / f32 =
    (states, loss, dL/dactions, dL/dstate0); `keep`: trajectories away from a
    kink, with the coverage conditions asserted."""
    def make():
        from oracle import c_oracle as co
        d = clamp_batch(B, H, DT, seed=H + B if seed is None else seed)
        args = (_np(d["state0"]), _np(d["actions"]), _np(d["ref"]), DT)
        f64 = co.wing_rollout_fwd_bwd(*args, modified_params=PARAMS[tag], dtype=np.float64)
        f32 = co.wing_rollout_fwd_bwd(*args, modified_params=PARAMS[tag], dtype=np.float32)
        assert all(np.all(np.isfinite(x)) for x in (f64[0], f64[2], f64[3]))
        pre = pre_states(args[0], f64[0])
        keep = assert_coverage(pre, f"rollout B{B} H{H} {tag}")
        return dict(d=d, f64=f64, f32=f32, pre=pre, keep=keep)
    return _cached(("rollout", B, H, tag, seed), make)


def check_rollout(got, ref, what, states_only=False):
    """`got`: dict(states, loss, grad_actions, grad_state0) in the AoS shapes.
    Everything finite on every trajectory; on the kept ones states, dL/dactions
    and dL/dstate0 no worse than the float32 oracle against the float64 one
    (conftest.assert_no_worse_than_fp32, its defaults), the loss at 1e-4."""
    from conftest import assert_no_worse_than_fp32
    keep, f64, f32 = ref["keep"], ref["f64"], ref["f32"]
    names = (("states", 0),) if states_only else (
        ("states", 0), ("grad_actions", 2), ("grad_state0", 3))
    stats = {}
    for name, i in names:
        x = np.asarray(got[name])
        assert x.shape == f64[i].shape, (what, name, x.shape)
        assert np.all(np.isfinite(x)), (what, name)
        stats[name] = assert_no_worse_than_fp32(x[keep], f32[i][keep], f64[i][keep],
                                                f"{what} {name}")
    if not states_only:
        e = abs(float(got["loss"]) - f64[1]) / abs(f64[1])
        print(what, "loss error %.3g" % e)
        assert e < BAR, (what, e)
    return stats


def mixed_pairs(pre_states64):
    """Share of the lane pairs (2 i, 2 i + 1) of the two-per-lane kernel whose
    two trajectories are in different clamp states on at least one step."""
    pre = np.asarray(pre_states64, np.float64)
    ra, rb = ratios(pre[:pre.shape[0] // 2 * 2])
    ca, cb = np.abs(ra) > 1, np.abs(rb) > 1
    mixed = (ca[0::2] != ca[1::2]) | (cb[0::2] != cb[1::2])
    return float(mixed.any(1).mean())


# ---------------------------------------------------------- learnt references
SETS = {"w": "w.", "steps": "steps.w."}


def learnt_weights(which):
    """{reference state_dict name: float32 array} of a recorded weight set of
    learnt_wing.npz (`steps`: a general inertia matrix)."""
    g = load_golden("learnt_wing.npz")
    p = SETS[which]
    return {k[len(p):]: np.array(g[k]) for k in g.files if k.startswith(p)}


def target_mod():
    g = load_golden("learnt_wing.npz")
    return {kv.split("=")[0]: float(kv.split("=")[1]) for kv in g["target_mod"]}


def learnt_rollout_reference(which, B, H):
    """clamp_batch(B, H) through LearntWingOracle: f64 / f32 = dict(states,
    loss, grad_actions, grad_state0); `keep` and the coverage as above."""
    def make():
        from oracle import torch_port as tp
        d = clamp_batch(B, H, DT, seed=H + B)
        out = dict(d=d)
        for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            ora = tp.LearntWingOracle(learnt_weights(which), dtype=dtype)
            s0 = d["state0"].clone().to(dtype).requires_grad_(True)
            a = d["actions"].clone().to(dtype).requires_grad_(True)
            states, cur = [], s0
            for k in range(H):
                cur = ora(cur, a[:, k], DT)
                states.append(cur)
            states = torch.stack(states, dim=1)
            loss = tp.fixed_wing_mpc_loss(states, d["ref"].to(dtype), a)
            loss.backward()
            out[name] = dict(states=states.detach().numpy(), loss=float(loss.detach()),
                             grad_actions=a.grad.numpy(), grad_state0=s0.grad.numpy())
        assert all(np.all(np.isfinite(v)) for v in out["f64"].values())
        out["pre"] = pre_states(d["state0"].numpy(), out["f64"]["states"])
        out["keep"] = assert_coverage(out["pre"], f"learnt rollout {which} B{B} H{H}")
        return out
    return _cached(("learnt_rollout", which, B, H), make)


def check_learnt_rollout(got, ref, what):
    from conftest import assert_no_worse_than_fp32
    keep = ref["keep"]
    stats = {}
    for name in ("states", "grad_actions", "grad_state0"):
        x = np.asarray(got[name])
        assert np.all(np.isfinite(x)), (what, name)
        stats[name] = assert_no_worse_than_fp32(
            x[keep], ref["f32"][name][keep], ref["f64"][name][keep], f"{what} {name}")
    e = abs(float(got["loss"]) - ref["f64"]["loss"]) / abs(ref["f64"]["loss"])
    print(what, "loss error %.3g" % e)
    assert e < BAR, (what, e)
    return stats


FIT_B = 321


def fit_batch():
    d = clamp_batch(FIT_B, 1, DT, seed=40 + FIT_B)
    return d["state0"], d["actions"][:, 0].contiguous()


def fit_reference(which):
    """The simulator-fit loss sum (pred - target)^2 on fit_batch() by autograd
    through LearntWingOracle.  Two target modes:
      `params`: target = the analytic step on target_mod(), in the oracle's own
                precision (the kernel computes it in float32 from eval_params);
      `target`: target = that step's float32 result, handed over as a tensor.
    Per mode f64 / f32 = dict(loss, g {name: gradient or None}, grad_state,
    grad_action, pred); `scale` {physical name: sum_b |sample gradient|} from
    float64 (mode `params`) - a batch sum of signed float32 terms carries
    rounding proportional to the terms, not to what is left after they cancel
    (test_zero_residual_physical_gradients_are_the_step_reverses);
    `cot32` = 2 (pred - target) of mode `target` in float32, the cotangent the
    single-step tests feed; `step` f64 / f32: the gradients for exactly that
    cotangent."""
    def make():
        from oracle import torch_port as tp
        s, a = fit_batch()
        w = learnt_weights(which)
        with torch.no_grad():
            tgt64 = tp.WingOracle(target_mod(), dtype=torch.float64)(s, a, DT)
            tgt32 = tp.WingOracle(target_mod(), dtype=torch.float32)(s, a, DT)
        out = dict(state=s, action=a, target32=tgt32.numpy())

        def run(dtype, tgt, cot=None):
            ora = tp.LearntWingOracle(w, dtype=dtype)
            sx = s.clone().to(dtype).requires_grad_(True)
            ax = a.clone().to(dtype).requires_grad_(True)
            pred = ora(sx, ax, DT)
            loss = (torch.sum((pred - tgt.to(dtype))**2) if cot is None
                    else torch.sum(pred * cot.to(dtype)))
            loss.backward()
            return dict(loss=float(loss.detach()), pred=pred.detach().numpy(),
                        grad_state=sx.grad.numpy(), grad_action=ax.grad.numpy(),
                        g={k: (None if p.grad is None else p.grad.numpy())
                           for k, p in ora.p.items()})
        out["params"] = dict(f64=run(torch.float64, tgt64), f32=run(torch.float32, tgt32))
        out["target"] = dict(f64=run(torch.float64, tgt32), f32=run(torch.float32, tgt32))
        cot32 = torch.from_numpy(
            2 * (out["target"]["f64"]["pred"] - tgt32.double().numpy())).float()
        out["cot32"] = cot32
        out["step"] = dict(f64=run(torch.float64, None, cot32),
                           f32=run(torch.float32, None, cot32))
        # per-sample magnitudes of the physical gradients
        ora = tp.LearntWingOracle(w, dtype=torch.float64)
        physical = [k for k in w if k not in RESIDUAL]
        scale = {k: np.zeros(np.asarray(w[k]).shape) for k in physical}
        for b in range(FIT_B):
            for p in ora.p.values():
                p.grad = None
            pred = ora(s[b:b + 1].double(), a[b:b + 1].double(), DT)
            torch.sum((pred - tgt64[b:b + 1])**2).backward()
            for k in physical:
                if ora.p[k].grad is not None:
                    scale[k] += np.abs(ora.p[k].grad.numpy())
        out["scale"] = scale
        out["keep"] = assert_coverage(s.double().numpy()[:, None], f"fit batch {which}",
                                      rollout=False)
        # a batch SUM cannot set a sample aside: the input holds none near a kink
        assert out["keep"].all()
        return out
    return _cached(("fit", which), make)


def physical_errors(got, want, scale):
    """{name: max |got - want| / max sum_b |sample gradient|} over the physical
    parameters; one without a gradient (cfg.g) must be exactly zero."""
    errs = {}
    for k, sc in scale.items():
        if want[k] is None or not np.any(sc):
            assert got[k] is None or not np.any(got[k]), k
            continue
        g = np.asarray(got[k], np.float64).reshape(sc.shape)
        errs[k] = float(np.abs(g - want[k]).max() / sc.max())
    return errs


def assert_physical_no_worse_than_fp32(dev, ref, what, worst_factor=4.0, floor=1e-6,
                                       bar=BAR):
    """Each physical parameter's batch-summed gradient on the scale of
    physical_errors: within the 1e-4 bar and within conftest's bound on a single
    worst value, `worst_factor` x float32 autograd's error + `floor`.
    `ref`: dict(f64, f32) of fit_reference (their `g`), plus its `scale`."""
    e_dev = physical_errors(dev, ref["f64"]["g"], ref["scale"])
    e_f32 = physical_errors(ref["f32"]["g"], ref["f64"]["g"], ref["scale"])
    k = max(e_dev, key=e_dev.get)
    print(what, "physical gradients / summed magnitudes: worst %.3g (%s), float32 "
          "autograd worst %.3g; relative to the sum itself %.3g" % (
              e_dev[k], k, max(e_f32.values()),
              np.abs(np.asarray(dev[k], np.float64).reshape(-1)
                     - np.asarray(ref["f64"]["g"][k]).reshape(-1)).max()
              / np.abs(ref["f64"]["g"][k]).max()))
    for n, e in e_dev.items():
        assert np.isfinite(e) and e < bar, (what, n, e)
        assert e <= worst_factor * e_f32[n] + floor, (what, n, e, e_f32[n])
    return e_dev


def check_fit(res, ref, mode, what):
    """`res`: dict(loss, g {name: gradient}) of one fit step; `ref`:
    wing_clamp_cases.fit_reference(which)."""
    from conftest import assert_param_rows_no_worse_than_fp32
    m = ref[mode]
    e = abs(res["loss"] - m["f64"]["loss"]) / m["f64"]["loss"]
    print(what, "loss error %.3g" % e)
    assert e < BAR
    assert all(np.all(np.isfinite(v)) for v in res["g"].values())
    assert_physical_no_worse_than_fp32(res["g"], dict(m, scale=ref["scale"]), what)
    pick = lambda g: {k: np.asarray(g[k]) for k in RESIDUAL}
    assert_param_rows_no_worse_than_fp32(pick(res["g"]), pick(m["f32"]["g"]),
                                         pick(m["f64"]["g"]), what)
