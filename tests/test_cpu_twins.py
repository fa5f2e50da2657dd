"""libapg_cpu.so (include/apg_cpu.h): the host twins of the dynamics entry
points - the kernels' per-trajectory headers compiled for the host behind the
signatures of apg.h minus the stream.  Pinned here to the golden
vectors the reference produced (tests/golden/make_golden.py), in every layout,
and - on a GPU - to the device entry points on the same inputs.  The Python
package must never load this library (it is not a fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden, rel_err

AOS, SOA, PACKED = 1, 0, 2
MOD = {"translational_drag": [.1, .2, .3], "rotational_drag": [.01, .02, .03],
       "mass": 1.0}
WING_MOD = {"mass": 1.4, "I_xz": -0.01, "CL0": 0.3, "rho": 1.0}
_F = ctypes.c_float


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@pytest.fixture(scope="module")
def tw():
    from apg_trajectory_tracking_amd import build as b
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(b.LIB_CPU):
        pytest.skip("no hipcc to compile the host twins")
    lib = ctypes.CDLL(b.build_cpu())
    lib.apg_cpu_last_error_string.restype = ctypes.c_char_p
    return lib


# ---- layout changes (numpy): per-trajectory vectors [B, S], sequences [B, H, C]
def vec_to(a, layout):
    a = _f(a)
    if layout == AOS:
        return a
    if layout == SOA:
        return _f(a.T)
    B, S = a.shape
    return _f(a.reshape(B, S // 4, 4).transpose(1, 0, 2))          # [S/4][B][4]


def vec_from(a, layout, B, S):
    if layout == AOS:
        return a.reshape(B, S)
    if layout == SOA:
        return a.reshape(S, B).T
    return a.reshape(S // 4, B, 4).transpose(1, 0, 2).reshape(B, S)


def seq_to(a, layout):
    a = _f(a)
    if layout == AOS:
        return a
    if layout == SOA:
        return _f(a.transpose(1, 2, 0))                            # [H][C][B]
    return _f(a.transpose(1, 0, 2))                                # [H][B][C]


def seq_from(a, layout, B, H, C):
    if layout == AOS:
        return a.reshape(B, H, C)
    if layout == SOA:
        return a.reshape(H, C, B).transpose(2, 0, 1)
    return a.reshape(H, B, C).transpose(1, 0, 2)


def states_from(a, layout, B, H, S):
    if layout == PACKED:                                           # [H][S/4][B][4]
        return a.reshape(H, S // 4, B, 4).transpose(2, 0, 1, 3).reshape(B, H, S)
    return seq_from(a, layout, B, H, S)


def _quad_params(mp):
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    return FlightmareDynamics(modified_params=mp).params


def _wing_params(mp):
    from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
        FixedWingDynamics)
    return FixedWingDynamics(modified_params=mp).params


def test_every_declared_twin_is_exported_and_has_a_device_original(tw):
    """include/apg_cpu.h: each `..._cpu` symbol resolves, and its name minus
    the suffix is an entry point of apg.h whose parameter list it repeats minus
    the trailing stream."""
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    cpu = open(os.path.join(REPO, "include", "apg_cpu.h")).read()
    gpu = open(os.path.join(REPO, "include", "apg.h")).read()
    decls = re.findall(r"\bint\s+(apg_\w+_cpu)\s*\(([^;]*?)\)\s*;", cpu, re.S)
    assert len(decls) == 12
    for name, args in decls:
        assert hasattr(tw, name), name
        m = re.search(r"\bint\s+" + name[:-4] + r"\s*\(([^;]*?)\)\s*;", gpu, re.S)
        assert m, name
        dev_args = norm(m.group(1))
        assert dev_args.endswith(", apg_stream_t stream"), name
        assert norm(args) == dev_args[:-len(", apg_stream_t stream")], name
    assert tw.apg_cpu_version() >= 1


def test_the_package_never_loads_the_twins():
    pkg = os.path.join(REPO, "apg_trajectory_tracking_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f != "build.py":
                src = open(os.path.join(root, f)).read()
                assert "apg_cpu" not in src and "_cpu(" not in src, f
    # and the library stands alone: no HIP runtime behind it
    import subprocess
    from apg_trajectory_tracking_amd import build as b
    if os.path.exists(b.LIB_CPU):
        deps = subprocess.run(["ldd", b.LIB_CPU], capture_output=True, text=True).stdout
        assert "amdhip" not in deps and "hsa-runtime" not in deps, deps


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("tag,mp", [("def", {}), ("mod", MOD)])
@pytest.mark.parametrize("dt", [0.05, 0.1])
def test_quad_step_twins_vs_golden(tw, tag, mp, dt, layout):
    g = load_golden("quad_step.npz")
    key = f"{tag}_dt{int(round(dt * 100)):03d}"
    par = _quad_params(mp)
    s, a = vec_to(g["state"], layout), vec_to(g["action"], layout)
    B = g["state"].shape[0]
    nxt = np.empty_like(s)
    assert tw.apg_quad_step_fwd_cpu(_p(s), _p(a), _F(dt), ctypes.byref(par), B, layout,
                                    _p(nxt)) == 0
    assert rel_err(vec_from(nxt, layout, B, 12), g[key + "_next"]) < 2e-6
    for i, c in enumerate(g["cot"]):
        gs, ga = np.empty_like(s), np.empty_like(a)
        assert tw.apg_quad_step_bwd_cpu(_p(s), _p(a), _F(dt), ctypes.byref(par), B, layout,
                                        _p(vec_to(c, layout)), _p(gs), _p(ga)) == 0
        assert rel_err(vec_from(gs, layout, B, 12), g[key + "_gstate"][i]) < 1e-5
        assert rel_err(vec_from(ga, layout, B, 4), g[key + "_gaction"][i]) < 1e-5
    # either output may be skipped
    gs = np.empty_like(s)
    assert tw.apg_quad_step_bwd_cpu(_p(s), _p(a), _F(dt), ctypes.byref(par), B, layout,
                                    _p(vec_to(g["cot"][0], layout)), _p(gs), None) == 0
    assert rel_err(vec_from(gs, layout, B, 12), g[key + "_gstate"][0]) < 1e-5
    # the reference's own known answer (quad_dynamics_flightmare.py __main__)
    s1, a1 = _f(g["ka_state"]), _f(g["ka_action"])
    n1 = np.empty_like(s1)
    assert tw.apg_quad_step_fwd_cpu(_p(s1), _p(a1), _F(float(g["ka_dt"])),
                                    ctypes.byref(_quad_params({})), 1, AOS, _p(n1)) == 0
    assert rel_err(n1, g["ka_next"]) < 2e-6


def _quad_rollout(tw, s0, act, ref, dt, mp, layout, want_states=True, deferred=None,
                  weights=None):
    """weights: an ApgQuadLossWeights (default: the reference's five)."""
    from apg_trajectory_tracking_amd import functional as F
    B, H = act.shape[:2]
    if layout == PACKED:
        ref = ref[:, :, [0, 1, 2, 6, 7, 8]]
    s, a, r = vec_to(s0, layout), seq_to(act, layout), seq_to(ref, layout)
    part = np.full((B + 63) // 64, np.nan, np.float32)
    loss = np.full(1, np.nan, np.float32)
    ga, gs = np.empty_like(a), np.empty_like(s)
    st = np.empty(B * H * 12, np.float32) if want_states else None
    w = weights or F.quad_loss_weights()
    rc = tw.apg_quad_rollout_fwd_bwd_cpu(
        _p(s), _p(a), _p(r), ref.shape[2], _F(dt), ctypes.byref(_quad_params(mp)),
        ctypes.byref(w), B, H, layout, _p(part), _p(loss), _p(ga), _p(gs), _p(st),
        deferred)
    assert rc == 0, tw.apg_cpu_last_error_string()
    return dict(states=None if st is None else states_from(st, layout, B, H, 12),
                loss=float(loss[0]), partials=part,
                ga=seq_from(ga, layout, B, H, 4), gs=vec_from(gs, layout, B, 12))


@pytest.mark.parametrize("layout", [AOS, SOA, PACKED])
@pytest.mark.parametrize("tag,mp", [("def", {}), ("mod", MOD)])
def test_quad_rollout_twin_vs_golden(tw, tag, mp, layout):
    g = load_golden("quad_rollout.npz")
    r = _quad_rollout(tw, g["state0"], g["actions"], g["ref"], float(g["dt"]), mp, layout)
    assert rel_err(r["states"], g[tag + "_states"]) < 1e-5
    assert abs(r["loss"] - g[tag + "_loss"]) / g[tag + "_loss"] < 1e-5
    assert rel_err(r["ga"], g[tag + "_gactions"]) < 1e-5
    assert rel_err(r["gs"], g[tag + "_gstate0"]) < 1e-5
    assert abs(r["partials"].sum() - r["loss"]) <= 1e-6 * abs(r["loss"])


@pytest.mark.parametrize("layout", [AOS, SOA, PACKED])
def test_quad_rollout_twin_h5_ragged_batch_and_deferred_loss(tw, layout):
    """H = 5 on a batch of 37 (one partial), then the same call reducing an
    EARLIER launch's partials (ApgDeferredLoss) as the device entry does."""
    from apg_trajectory_tracking_amd import _capi
    g = load_golden("quad_rollout.npz")
    r = _quad_rollout(tw, g["h5_state0"], g["h5_actions"], g["h5_ref"], float(g["h5_dt"]),
                      {}, layout, want_states=False)
    assert r["states"] is None and r["partials"].shape == (1,)
    assert abs(r["loss"] - g["h5_loss"]) / g["h5_loss"] < 1e-5
    assert rel_err(r["ga"], g["h5_gactions"]) < 1e-5
    assert rel_err(r["gs"], g["h5_gstate0"]) < 1e-5
    prev = np.array([1.5, 2.25, -0.75], np.float32)
    prev_loss = np.zeros(1, np.float32)
    d = _capi.ApgDeferredLoss(prev_partials=prev.ctypes.data, prev_count=3,
                              prev_loss=prev_loss.ctypes.data)
    _quad_rollout(tw, g["h5_state0"], g["h5_actions"], g["h5_ref"], float(g["h5_dt"]), {},
                  layout, want_states=False, deferred=ctypes.byref(d))
    assert prev_loss[0] == 3.0


def test_quad_rollout_fwd_twin_and_partials_per_64(tw):
    from apg_trajectory_tracking_amd import synthetic
    B, H, dt = 200, 10, 0.1
    d = synthetic.quad_polynomial_batch(B, H, dt, seed=5)
    s0, act, ref = (d[k].numpy() for k in ("state0", "actions", "ref"))
    full = _quad_rollout(tw, s0, act, ref, dt, MOD, SOA)
    assert full["partials"].shape == (4,) and np.isfinite(full["partials"]).all()
    # partial w = the 64 trajectories 64 w .. of the batch, on their own
    part1 = _quad_rollout(tw, s0[64:128], act[64:128], ref[64:128], dt, MOD, AOS)
    assert abs(part1["loss"] - full["partials"][1]) <= 1e-6 * abs(part1["loss"])
    for layout in (AOS, SOA):
        st = np.empty(B * H * 12, np.float32)
        assert tw.apg_quad_rollout_fwd_cpu(
            _p(vec_to(s0, layout)), _p(seq_to(act, layout)), _F(dt),
            ctypes.byref(_quad_params(MOD)), B, H, layout, _p(st)) == 0
        assert np.array_equal(seq_from(st, layout, B, H, 12), full["states"])


@pytest.mark.parametrize("layout", [AOS, SOA])
@pytest.mark.parametrize("tag,mp", [("def", {}), ("mod", WING_MOD)])
def test_wing_twins_vs_golden(tw, tag, mp, layout):
    from apg_trajectory_tracking_amd import functional as F
    g = load_golden("wing.npz")
    par = _wing_params(mp)
    B = g["step_state"].shape[0]
    s, a = vec_to(g["step_state"], layout), vec_to(g["step_action"], layout)
    nxt = np.empty_like(s)
    assert tw.apg_wing_step_fwd_cpu(_p(s), _p(a), _F(0.05), ctypes.byref(par), B, layout,
                                    _p(nxt)) == 0
    assert rel_err(vec_from(nxt, layout, B, 12), g[f"step_{tag}_next"]) < 2e-6
    for i, c in enumerate(g["step_cot"]):
        gs, ga = np.empty_like(s), np.empty_like(a)
        assert tw.apg_wing_step_bwd_cpu(_p(s), _p(a), _F(0.05), ctypes.byref(par), B, layout,
                                        _p(vec_to(c, layout)), _p(gs), _p(ga)) == 0
        assert rel_err(vec_from(gs, layout, B, 12), g[f"step_{tag}_gstate"][i]) < 1e-5
        assert rel_err(vec_from(ga, layout, B, 4), g[f"step_{tag}_gaction"][i]) < 1e-5
    if tag != "def":
        return
    w = F.wing_loss_weights()
    for H in (20, 10):
        p = f"h{H}_"
        s0, act, ref = (vec_to(g[p + "state0"], layout), seq_to(g[p + "actions"], layout),
                        seq_to(g[p + "ref"], layout))
        B = g[p + "state0"].shape[0]
        part, loss = np.empty(1, np.float32), np.empty(1, np.float32)
        ga, gs = np.empty_like(act), np.empty_like(s0)
        st = np.empty(B * H * 12, np.float32)
        assert tw.apg_wing_rollout_fwd_bwd_cpu(
            _p(s0), _p(act), _p(ref), _F(0.05), ctypes.byref(par), ctypes.byref(w), B, H,
            layout, _p(part), _p(loss), _p(ga), _p(gs), _p(st), None) == 0
        assert rel_err(seq_from(st, layout, B, H, 12), g[p + "states"]) < 1e-5
        assert abs(loss[0] - g[p + "loss"]) / g[p + "loss"] < 1e-5
        assert rel_err(seq_from(ga, layout, B, H, 4), g[p + "gactions"]) < 2e-5
        assert rel_err(vec_from(gs, layout, B, 12), g[p + "gstate0"]) < 2e-5
        st2 = np.empty_like(st)
        assert tw.apg_wing_rollout_fwd_cpu(_p(s0), _p(act), _F(0.05), ctypes.byref(par), B,
                                           H, layout, _p(st2)) == 0
        assert np.array_equal(st2, st)


@pytest.mark.parametrize("layout", [AOS, SOA])
def test_cartpole_twins_vs_golden(tw, layout):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    g = load_golden("cartpole.npz")
    par = CartpoleDynamics().params
    s1, a1 = _f(g["ka_state"]), _f(g["ka_action"])
    n1 = np.empty_like(s1)
    assert tw.apg_cartpole_step_fwd_cpu(_p(s1), _p(a1), _F(0.02), ctypes.byref(par), 1, AOS,
                                        _p(n1)) == 0
    assert rel_err(n1, g["ka_next"]) < 2e-6
    B, H = g["actions"].shape[:2]
    s, a = vec_to(g["state0"], layout), _f(g["actions"][:, 0, 0])
    nxt, gs, ga = np.empty_like(s), np.empty_like(s), np.empty_like(a)
    assert tw.apg_cartpole_step_fwd_cpu(_p(s), _p(a), _F(0.02), ctypes.byref(par), B, layout,
                                        _p(nxt)) == 0
    assert rel_err(vec_from(nxt, layout, B, 4), g["step_next"]) < 2e-6
    assert tw.apg_cartpole_step_bwd_cpu(_p(s), _p(a), _F(0.02), ctypes.byref(par), B, layout,
                                        _p(vec_to(g["step_cot"], layout)), _p(gs),
                                        _p(ga)) == 0
    assert rel_err(vec_from(gs, layout, B, 4), g["step_gstate"]) < 1e-5
    assert rel_err(ga, g["step_gaction"][:, 0]) < 1e-5
    act = seq_to(g["actions"], layout)
    part, loss = np.empty(1, np.float32), np.empty(1, np.float32)
    gact, gs0 = np.empty_like(act), np.empty_like(s)
    st = np.empty(B * H * 4, np.float32)
    assert tw.apg_cartpole_rollout_fwd_bwd_cpu(
        _p(s), _p(act), _F(float(g["dt"])), ctypes.byref(par), B, H, layout, _p(part),
        _p(loss), _p(gact), _p(gs0), _p(st)) == 0
    assert rel_err(seq_from(st, layout, B, H, 4), g["states"]) < 1e-5
    assert abs(loss[0] - g["loss"]) / g["loss"] < 1e-5
    assert rel_err(seq_from(gact, layout, B, H, 1), g["gactions"]) < 1e-5
    assert rel_err(vec_from(gs0, layout, B, 4), g["gstate0"]) < 1e-5
    st2 = np.empty_like(st)
    assert tw.apg_cartpole_rollout_fwd_cpu(_p(s), _p(act), _F(float(g["dt"])),
                                           ctypes.byref(par), B, H, layout, _p(st2)) == 0
    assert np.array_equal(st2, st)


def test_twins_report_argument_errors_like_the_device_entries(tw):
    g = load_golden("quad_rollout.npz")
    from apg_trajectory_tracking_amd import functional as F
    par, w = _quad_params({}), F.quad_loss_weights()
    s, a, r = _f(g["state0"]), _f(g["actions"]), _f(g["ref"])
    out = np.empty_like(s)
    err = lambda: tw.apg_cpu_last_error_string()
    assert tw.apg_quad_step_fwd_cpu(_p(s), _p(a), _F(0.1), ctypes.byref(par), -1, AOS,
                                    _p(out)) == -1 and b"B must be >= 0" in err()
    assert tw.apg_quad_step_fwd_cpu(_p(s), _p(a), _F(0.1), ctypes.byref(par), 4, 7,
                                    _p(out)) == -1 and b"unknown layout" in err()
    assert tw.apg_quad_step_fwd_cpu(_p(s), _p(a), _F(0.1), None, 4, AOS,
                                    _p(out)) == -1 and b"params is NULL" in err()
    assert tw.apg_quad_step_fwd_cpu(_p(s), _p(a), _F(0.1), ctypes.byref(par), 4, PACKED,
                                    _p(out)) == -1      # packed: the fused rollout only
    part, ga = np.empty(1, np.float32), np.empty_like(a)

    def roll(H, layout, ref_cols=9, ref=r, grads=ga):
        return tw.apg_quad_rollout_fwd_bwd_cpu(
            _p(s), _p(a), _p(ref), ref_cols, _F(0.1), ctypes.byref(par), ctypes.byref(w),
            64, H, layout, _p(part), None, _p(grads), None, None, None)
    assert roll(0, AOS) == -1 and b"H must be in [1, 48]" in err()
    assert roll(49, AOS) == -1
    assert roll(10, AOS, ref_cols=5) == -1 and b"ref_cols" in err()
    assert roll(7, PACKED, ref_cols=6) == -1 and b"H must be 5 or 10" in err()
    assert roll(10, PACKED) == -1 and b"ref_cols = 6" in err()
    assert roll(10, AOS, ref=None) == -1 and roll(10, AOS, grads=None) == -1
    assert roll(10, AOS) == 0
    # B = 0: nothing to do, nothing touched
    assert tw.apg_quad_step_fwd_cpu(None, None, _F(0.1), ctypes.byref(par), 0, AOS,
                                    _p(out)) == 0


@pytest.mark.gpu
def test_twins_agree_with_the_device_entry_points():
    """Same inputs through libapg_hip.so on the GPU and libapg_cpu.so on the
    host (the same per-lane headers, two compilers): fp32 rounding apart."""
    import torch
    from apg_trajectory_tracking_amd import build as b, functional as F, synthetic
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    tw = ctypes.CDLL(b.build_cpu())
    dev = torch.device("cuda:0")
    B, H, dt = 3000, 10, 0.1
    d = synthetic.quad_polynomial_batch(B, H, dt, seed=8)
    s0, act, ref = (d[k] for k in ("state0", "actions", "ref"))
    par = _quad_params(MOD)
    res = F.quad_rollout_fwd_bwd(s0.to(dev), act.to(dev), ref.to(dev), dt, par,
                                 want_states=True)
    r = _quad_rollout(tw, s0.numpy(), act.numpy(), ref.numpy(), dt, MOD, AOS)
    N = lambda t: t.cpu().numpy()
    assert rel_err(r["states"], N(res["states"])) < 2e-6
    assert abs(r["loss"] - res["loss"].item()) / abs(r["loss"]) < 1e-6
    assert rel_err(r["ga"], N(res["grad_actions"])) < 5e-6
    assert rel_err(r["gs"], N(res["grad_state0"])) < 5e-6
    assert rel_err(r["partials"], N(res["loss_partials"])) < 1e-6
    # fixed wing, 20 steps
    wd = synthetic.wing_batch(B, 20, 0.05, seed=3) if hasattr(synthetic, "wing_batch") else None
    if wd is not None:
        wp = _wing_params({})
        ws0, wact, wref = (wd[k] for k in ("state0", "actions", "ref"))
        wres = F.wing_rollout_fwd_bwd(ws0.to(dev), wact.to(dev), wref.to(dev), 0.05, wp)
        part, loss = np.empty((B + 63) // 64, np.float32), np.empty(1, np.float32)
        ga, gs = np.empty((B, 20, 4), np.float32), np.empty((B, 12), np.float32)
        assert tw.apg_wing_rollout_fwd_bwd_cpu(
            _p(_f(ws0.numpy())), _p(_f(wact.numpy())), _p(_f(wref.numpy())), _F(0.05),
            ctypes.byref(wp), ctypes.byref(F.wing_loss_weights()), B, 20, AOS, _p(part),
            _p(loss), _p(ga), _p(gs), None, None) == 0
        assert abs(loss[0] - wres["loss"].item()) / abs(loss[0]) < 2e-6
        assert rel_err(ga, N(wres["grad_actions"])) < 2e-5
        assert rel_err(gs, N(wres["grad_state0"])) < 2e-5
    # cart-pole step
    g = load_golden("cartpole.npz")
    cp = CartpoleDynamics().params
    s, a = _f(g["state0"]), _f(g["actions"][:, 0])
    nxt = np.empty_like(s)
    assert tw.apg_cartpole_step_fwd_cpu(_p(s), _p(a), _F(0.02), ctypes.byref(cp),
                                        s.shape[0], AOS, _p(nxt)) == 0
    dn = F.cartpole_step(torch.from_numpy(s).to(dev), torch.from_numpy(a).to(dev), 0.02, cp)
    assert rel_err(nxt, N(dn)) < 1e-6
