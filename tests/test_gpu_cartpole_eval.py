"""The batched cart-pole closed-loop evaluation (apg_cartpole_mlp_closed_loop,
evaluate_cartpole.Evaluator) on the GPU: against the recordings of the REAL
Evaluator (G19), against the CPU restatement of tests/test_cartpole_eval_cpu.py
at a batch of many workgroups, the trainer's evaluation hook and training loop
(TrainCartpole.evaluate_model / train_control), and the device restatement of
construct_states (SyntheticCartpoleDataset.resample_data)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_cartpole_eval_cpu import (CASES, DT, case, case_net, check_against_case,
                                    closed_loop_cpu, construct_states_loop,
                                    golden_net)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", CASES)
def test_kernel_and_evaluator_vs_reference_recordings(dev, name):
    """(a) Every G19 case: the kernel on the recorded start states, and the
    Evaluator drawing them itself from the same numpy seed."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        CartpoleDynamics)
    from apg_trajectory_tracking_amd.evaluate_cartpole import (
        CartPoleEnv, CartpoleWrapper, Evaluator)
    g = load_golden("cartpole_closed_loop.npz")
    c = case(g, name)
    swing = int(c["swingup"])
    mp = {"masspole": float(c["masspole"]), "length": float(c["length"])}
    net = case_net(g, name).to(dev)
    dyn = CartpoleDynamics(mp)
    out = F.cartpole_mlp_closed_loop(
        net, torch.from_numpy(c["start"]).to(dev), DT, dyn.params, max_steps=250,
        mode="swingup" if swing else "balance", thresh_div=float(c["thresh_div"]),
        burn_in=int(c["burn_in"]), want_trajectory=True)
    # the untrained controller spins the pole (|theta_dot| up to 22 rad/s, the
    # angle wrapping round): the ulp-level differences between the device's
    # and the host's sin / cos / atan2 grow to 2.3e-4 of the angle's range
    # over 250 steps there (measured); the shipped controller's flights keep
    # the 1e-4 bound.  Steps and flags are compared exactly in every case.
    check_against_case(c, host(out),
                       state_tol=1e-3 if name == "swingup_untrained" else 1e-4)

    np.random.seed(int(c["seed"]))
    env = CartPoleEnv(dyn, DT, thresh_div=float(c["thresh_div"]))
    ev = Evaluator(CartpoleWrapper(net), env)
    ev.initialize_straight = int(c["straight"])
    n = len(c["steps"])
    if swing:
        res = ev.evaluate_swingup(nr_iters=n, max_steps=250)
    else:
        res = ev.evaluate_in_environment(nr_iters=n, max_steps=250)
    assert np.random.rand() == float(c["next_rand"])
    np.testing.assert_array_equal(ev.last_flights["steps"].cpu().numpy(), c["steps"])
    for k, v in res.items():
        assert abs(v - float(c[k])) <= 1e-4 * abs(float(c[k])), (k, v, c[k])
    if swing:
        np.testing.assert_allclose(env.state, c["env_state"], rtol=0,
                                   atol=1e-4 * np.abs(c["states"]).max())
    else:
        np.testing.assert_array_equal(env.state, c["env_state"])
    # return_success: the per-flight values
    np.random.seed(int(c["seed"]))
    env = CartPoleEnv(dyn, DT, thresh_div=float(c["thresh_div"]))
    ev = Evaluator(CartpoleWrapper(net), env)
    ev.initialize_straight = int(c["straight"])
    if swing:
        np.testing.assert_array_equal(
            ev.evaluate_swingup(nr_iters=n, return_success=1), c["upright"])
    else:
        success, velocities = ev.evaluate_in_environment(nr_iters=n, return_success=1)
        np.testing.assert_array_equal(success, c["success"])
        assert len(velocities) == int(c["steps"].sum())
        assert ev.evaluate_in_environment(nr_iters=0) == (0, 0, [])


def test_large_random_swingup_batch_vs_cpu_restatement(dev):
    """(b) B = 65 536 + 37 random swing-up flights (many workgroups, a ragged
    last wave) against the CPU restatement on a strided subset."""
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        CartpoleDynamics)
    g = load_golden("cartpole_closed_loop.npz")
    net = golden_net(g, "shipped")
    B, T = 65536 + 37, 250
    gen = torch.Generator().manual_seed(5)
    u = torch.rand(B, 4, generator=gen)
    s0 = (u * 2 - 1) * torch.tensor([2.4, 7.5, np.pi, 7.5])
    s0[:, 0] = 0
    s0[:, 1] *= .1
    s0[:, 3] *= .1
    sign = torch.where(torch.rand(B, generator=gen) > .5, -1.0, 1.0)
    s0[:, 2] = sign * (2.8 + torch.rand(B, generator=gen) * .3)
    out = host(F.cartpole_mlp_closed_loop(
        net.to(dev), s0.to(dev), DT, CartpoleDynamics().params, max_steps=T,
        mode="swingup", burn_in=100, want_trajectory=True))
    assert (out["steps"] == T).all()
    idx = np.unique(np.concatenate([np.arange(0, B, 251), np.arange(B - 37, B)]))
    assert len(idx) >= 256
    ref = closed_loop_cpu(golden_net(g, "shipped"), s0[idx], DT, {}, T, "swingup",
                          .21, 100)
    assert out["upright"][idx].tolist() == ref["upright"].tolist()
    got = out["states"][:, :, idx]
    want = ref["states"].numpy()
    scale = np.abs(want).max((0, 2))
    err = np.abs(got - want).max((0, 2))
    assert np.all(err <= 1e-4 * scale + 1e-6), (err, scale)
    np.testing.assert_allclose(out["vel_sum"][idx], ref["vel_sum"].numpy(), rtol=1e-4)


def cartpole_config(tmp_path, **kw):
    cfg = {"system": "cartpole", "delta_t": 0.05, "state_size": 4, "batch_size": 8,
           "nr_epochs": 3, "sample_in": "eval_env", "resample_every": 3,
           "thresh_div_start": 0.07, "thresh_div_step": 0.02, "thresh_div_end": 0.21,
           "l2_lambda": 0, "modified_params": {}, "horizon": 10, "action_dim": 1,
           "learning_rate_controller": 1e-9, "sample_data": 200, "suc_up_down": -1,
           "save_name": str(tmp_path / "cp")}
    cfg.update(kw)
    return cfg


def test_trainer_evaluate_model_and_train_control(dev, tmp_path, monkeypatch):
    """(c) TrainCartpole with the shipped controller: evaluate_model fills
    results_dict, runs the thresh_div ladder (0.07 -> 0.09 at epoch 0, -> 0.11
    at epoch 3), resamples at epoch 2 and checkpoints epochs > 0;
    train_control runs to finalize."""
    monkeypatch.chdir(tmp_path)
    from apg_trajectory_tracking_amd import train_cartpole as tc
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        CartpoleDynamics)
    g = load_golden("cartpole_closed_loop.npz")
    cfg = cartpole_config(tmp_path)
    tr = tc.TrainCartpole(CartpoleDynamics(), CartpoleDynamics(test_time=1), cfg)
    tr.initialize_model(golden_net(g, "shipped"), device=dev)
    assert cfg["thresh_div"] == 0.07
    before = tr.state_data.states.clone()
    ladder = []
    for epoch in range(4):
        res = tr.evaluate_model(epoch)
        ladder.append(round(cfg["thresh_div"], 6))
        assert res == (tr.results_dict["mean_vel"][-1], tr.results_dict["std_vel"][-1])
        if epoch == 1:
            assert torch.equal(tr.state_data.states, before)
        if epoch == 2:
            resampled = tr.state_data.states
            assert not torch.equal(resampled, before)
            assert torch.equal(tr.state_data.labels, resampled)
            assert resampled.shape == (200, 4)
            tr.run_epoch(train="controller")       # the loader sees the new rows
    assert ladder == [0.09, 0.09, 0.09, 0.11]
    assert tr.results_dict["evaluate_at"] == [0, 1, 2, 3]
    for k in ("mean_vel", "std_vel", "mean_stable", "std_stable"):
        assert len(tr.results_dict[k]) == 4
    assert tr.results_dict["mean_stable"][0] == 249.0      # balances throughout
    saved = sorted(os.listdir(tr.save_path))
    assert saved == ["model_cartpole1", "model_cartpole2", "model_cartpole3"]

    base = tmp_path / "base.pt"
    torch.save(golden_net(g, "shipped").state_dict(), base)
    cfg = cartpole_config(tmp_path, save_name=str(tmp_path / "tc"))
    trainer = tc.train_control(str(base), cfg, swingup=1, device=dev)
    assert cfg["learning_rate_controller"] == 1e-5
    assert trainer.results_dict["evaluate_at"] == [0, 1, 2]
    assert len(trainer.results_dict["loss_controller"]) == 3
    assert os.path.exists(os.path.join(trainer.save_path, "model_cartpole"))
    assert os.path.exists(os.path.join(trainer.save_path, "results.json"))


@pytest.mark.parametrize("num,thresh", [(400, .11), (333, .07)])
def test_resample_data_vs_cpu_loop(dev, num, thresh):
    """(d) construct_states on the device fed explicit draws equals the CPU
    loop; exactly num rows; every balancing run ends at its first state that
    is not upright."""
    from apg_trajectory_tracking_amd import dataset as ds
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import (
        CartpoleDynamics)
    d = ds.draw_cartpole_states(num, torch.Generator().manual_seed(num))
    got = ds.cartpole_states_from_draws({k: v.to(dev) for k, v in d.items()}, num,
                                        thresh, DT, CartpoleDynamics().params).cpu()
    want = construct_states_loop(d, num, thresh, DT)
    assert got.shape == want.shape == (num, 4)
    scale = want.abs().amax(0)
    assert ((got - want).abs().amax(0) <= 1e-4 * scale + 1e-6).all()
    # balancing part: a row outside the threshold is the last row of its run,
    # so the next row (if any) starts a new run near upright
    n_rand = d["rand_start"].shape[0] * ds.CARTPOLE_RANDOM_RUN
    tail = got[n_rand:]
    down = ~((tail[:, 2] > -thresh) & (tail[:, 2] < thresh))
    assert down.any()
    for i in torch.nonzero(down[:-1]).flatten().tolist():
        assert abs(float(tail[i + 1, 2])) < 0.05 + 0.5 * thresh

    data = ds.SyntheticCartpoleDataset(num, seed=1, device=dev)
    rows = data.states
    data.resample_data(num, thresh)
    assert data.states is rows and data.num_sampled_states == num
    assert torch.equal(data.states, data.labels)


# ------------------------------------------------ what needs no tolerance
# cart_closed_loop_kernel<false|true> (apg_cartpole_mlp_closed_loop,
# apg_cartpole_learnt_mlp_closed_loop) in both modes: the same bits from launch
# to launch, for an episode whatever batch it runs in, nothing written outside
# the outputs or after an episode's end, optional outputs that change nothing,
# and steps / upright / written rows that agree with each other.  (A per-episode
# float64 comparison is another matter: theta goes through atan2, a rounding
# at +-pi moves a value by 2 pi.)
BIT_T, BALANCE_THRESH = 40, 0.07
BIT_OUTPUTS = ("states", "actions", "steps", "upright", "vel_sum", "vel_sq")
BIT_CASES = [(env, mode, B) for env in ("analytic", "learnt") for mode in ("balance", "swingup")
             for B in (33, 129, 300)]


def _bit_start(mode, B):
    """Balance: near upright with the pole moving at up to 1.2 rad/s, so that with
    thresh_div = 0.07 the episodes end at different steps (about a fifth after
    one step, as many over the eight after it, the rest never); swing-up:
    hanging."""
    gen = torch.Generator().manual_seed(17 + B)
    u = lambda: 2 * torch.rand(B, generator=gen) - 1
    s0 = torch.stack((0.5 * u(), 1.0 * u(), 0.06 * u(), 1.2 * u()), 1)
    if mode == "swingup":
        s0[:, 2] = torch.where(u() > 0, 1.0, -1.0) * (2.8 + 0.3 * torch.rand(B, generator=gen))
    return s0


def _bit_fixtures(env, dev):
    from apg_trajectory_tracking_amd.dynamics.cartpole_dynamics import CartpoleDynamics
    from test_cartpole_learnt_cpu import fitted, g20
    net = golden_net(load_golden("cartpole_closed_loop.npz"), "shipped").to(dev)
    return net, CartpoleDynamics().params, (fitted(g20()).to(dev) if env == "learnt" else None)


def _bit_run(env, mode, s0, dev):
    from apg_trajectory_tracking_amd import functional as F
    net, params, learnt = _bit_fixtures(env, dev)
    return F.cartpole_mlp_closed_loop(net, s0.to(dev), DT, params, max_steps=BIT_T, mode=mode,
                                      thresh_div=BALANCE_THRESH, burn_in=10,
                                      want_trajectory=True, learnt=learnt)


def _differing(a, b):
    if a.shape != b.shape:
        return -1
    as_int = {torch.float32: torch.int32, torch.float64: torch.int64}.get(a.dtype)
    if as_int is not None:
        a, b = a.contiguous().view(as_int), b.contiguous().view(as_int)
    return int((a != b).sum())


@pytest.mark.parametrize("env,mode,B", BIT_CASES)
def test_closed_loop_bits_across_launches_and_batches(dev, env, mode, B):
    """Three launches give the same bits; a permuted batch gives every episode
    the same bits; in balance mode steps, upright and the rows written agree."""
    s0 = _bit_start(mode, B)
    first = _bit_run(env, mode, s0, dev)
    for again in range(2):
        out = _bit_run(env, mode, s0, dev)
        for k in BIT_OUTPUTS:
            assert _differing(out[k], first[k]) == 0, (k, again)
    order = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    moved, o = _bit_run(env, mode, s0[order], dev), order.to(dev)
    for k in BIT_OUTPUTS:
        assert _differing(moved[k], first[k][..., o]) == 0, k
    steps, upright = first["steps"].cpu().numpy(), first["upright"].cpu().numpy()
    if mode == "swingup":
        assert (steps == BIT_T).all()
        return
    assert len(set(steps.tolist())) > 3 and (steps == BIT_T).any() and (steps < BIT_T).any()
    states = first["states"].cpu().numpy()                      # [T,4,B]
    last = states[steps - 1, 2, np.arange(B)]                   # theta of the last written row
    outside = ~((-np.float32(BALANCE_THRESH) < last) & (last < np.float32(BALANCE_THRESH)))
    assert ((upright == 0) == outside).all()
    assert (upright[steps < BIT_T] == 0).all()


CART_GUARD, CART_EXTRA = 2, 2


def _cart_abi(env, mode, s0, dev, skip=()):
    """The C entry point on NaN-filled states / actions with guard planes around
    them and rows beyond T; `skip`: handed over as NULL."""
    import ctypes
    from apg_trajectory_tracking_amd import _capi, functional as F
    net, params, learnt = _bit_fixtures(env, dev)
    B, T = s0.shape[0], BIT_T
    pw = []
    for l in (net.fc0, net.fc1, net.fc2, net.fc3, net.fc_out):
        pw += [l.weight.detach().float().contiguous(), l.bias.detach().float().contiguous()]
    pol = _capi.ApgCartpolePolicy(*[t.data_ptr() for t in pw])
    soa = s0.float().t().contiguous().to(dev)
    cols = dict(states=4, actions=1)
    full = {k: torch.full((CART_GUARD + (T + CART_EXTRA) * c + CART_GUARD, B), float("nan"),
                          device=dev) for k, c in cols.items() if k not in skip}
    ints = {k: torch.full((CART_GUARD + 1 + CART_GUARD, B), -7, dtype=torch.int32, device=dev)
            for k in ("steps", "upright")}
    sums = {k: torch.full((CART_GUARD + 1 + CART_GUARD, B), float("nan"), dtype=torch.float64,
                          device=dev) for k in ("vel_sum", "vel_sq")}
    at = lambda k: full[k][CART_GUARD:].data_ptr() if k in full else None
    lib = _capi.lib()
    ws = torch.empty(lib.apg_cartpole_policy_workspace_floats(), device=dev)
    if learnt is None:
        name, model = "apg_cartpole_mlp_closed_loop", params
    else:
        name = "apg_cartpole_learnt_mlp_closed_loop"
        model = F._cartpole_learnt_model(F._cartpole_learnt_tensors(learnt))
    flight = _capi.ApgCartpoleFlight(
        state0=soa.data_ptr(), max_steps=T, mode=F.CARTPOLE_MODES[mode],
        thresh_div=BALANCE_THRESH, burn_in=10, steps=ints["steps"][CART_GUARD:].data_ptr(),
        upright=ints["upright"][CART_GUARD:].data_ptr(),
        vel_sum=sums["vel_sum"][CART_GUARD:].data_ptr(),
        vel_sq=sums["vel_sq"][CART_GUARD:].data_ptr(), states=at("states"),
        actions=at("actions"))
    _capi.check(getattr(lib, name)(
        ctypes.byref(flight), DT, ctypes.byref(model), ctypes.byref(pol), B, ws.data_ptr(),
        _capi.stream_of(soa)), name)
    torch.cuda.synchronize(dev)
    for k, buf in full.items():
        used = T * cols[k]
        assert torch.isnan(buf[:CART_GUARD]).all() and \
            torch.isnan(buf[CART_GUARD + used:]).all(), (k, "wrote outside its view")
    for k, buf in ints.items():
        assert (buf[:CART_GUARD] == -7).all() and (buf[CART_GUARD + 1:] == -7).all(), k
    for k, buf in sums.items():
        assert torch.isnan(buf[:CART_GUARD]).all() and torch.isnan(buf[CART_GUARD + 1:]).all(), k
    return {**full, **ints, **sums}


@pytest.mark.parametrize("env,mode,B", BIT_CASES)
def test_closed_loop_c_abi_guarded_buffers_and_optional_outputs(dev, env, mode, B):
    """Nothing is written outside the views or after an episode's end (rows k <
    steps are written, the rest keep their NaN); states and / or actions NULL
    change no other bit; the wrapper's call gives the same bits."""
    s0 = _bit_start(mode, B)
    whole = _cart_abi(env, mode, s0, dev)
    steps = whole["steps"][CART_GUARD]
    assert (whole["upright"][CART_GUARD] >= 0).all() and (steps >= 1).all()
    written = torch.arange(BIT_T, device=dev)[:, None] < steps[None, :]          # [T,B]
    states = whole["states"][CART_GUARD:CART_GUARD + 4 * BIT_T].view(BIT_T, 4, B)
    actions = whole["actions"][CART_GUARD:CART_GUARD + BIT_T]
    assert (torch.isnan(states) == ~written[:, None, :]).all()
    assert (torch.isnan(actions) == ~written).all()
    out = _bit_run(env, mode, s0, dev)
    assert _differing(torch.where(written[:, None, :], states, 0.0), out["states"]) == 0
    assert _differing(torch.where(written, actions, 0.0), out["actions"]) == 0
    for k in ("steps", "upright", "vel_sum", "vel_sq"):
        assert _differing(whole[k][CART_GUARD], out[k]) == 0, k
    for skip in (("states",), ("actions",), ("states", "actions")):
        part = _cart_abi(env, mode, s0, dev, skip=skip)
        assert set(part) == set(whole) - set(skip)
        for k, buf in part.items():
            assert _differing(buf, whole[k]) == 0, (skip, k)
