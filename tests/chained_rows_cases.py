"""Inputs and float64 oracle results shared by tests/test_chained_rows_kernel_cpu.py
and tests/test_gpu_chained_rows_kernel.py (no test in here): every input set is
made once, every oracle pass is computed once and handed out unchanged."""
import functools

import torch

DT = 0.1
BATCHES = [1, 64, 65, 64 * 3 + 17]   # a lone lane, a full wave, a wave with one
#                                      live lane, a ragged last wave
HORIZONS = [5, 10]
NPLANS = 3
KINDS = ("poly", "large", "zero")
SPECIAL_B = 64 * 3 + 17              # the batch of the `large` and `zero` inputs
TOL = 1e-4                           # tests/test_gpu_parity.py, packed rollout


def cases():
    """(kind, B, H) of every input set the GPU test launches."""
    out = [("poly", B, H) for H in HORIZONS for B in BATCHES]
    out += [(kind, SPECIAL_B, H) for kind in ("large", "zero") for H in HORIZONS]
    return out


@functools.lru_cache(maxsize=None)
def inputs(kind, B, H, plan):
    """float32 {state0 [B,12], actions [B,H,4], ref [B,H,9]} of plan `plan`.
    large: the first 64 trajectories start at attitudes spread uniformly over
    +-1e4 rad (where a one-word range reduction fails), the rest
    at tens of radians; zero: attitudes exactly 0."""
    from apg_trajectory_tracking_amd import synthetic as sy
    seed = 1000 * KINDS.index(kind) + 100 * H + 7 * plan + B
    d = sy.quad_polynomial_batch(B, H, DT, seed=seed)
    s0 = d["state0"].clone()
    actions = d["actions"].clone()
    if kind == "large":
        g = torch.Generator().manual_seed(seed + 1)
        s0[:, 3:6] = 30.0 * torch.randn(B, 3, generator=g)
        s0[:64, 3:6] = 1e4 * (2.0 * torch.rand(64, 3, generator=g) - 1.0)
        # float32 spaces attitudes near 1e4 rad 1e-3 rad apart: a rollout that
        # MOVES such an attitude rounds it by up to 5e-4 rad per step whoever
        # computes it, and the reference's own float32 arithmetic then misses
        # 1e-4 of the float64 result (measured here: 1.8e-4 / 2.7e-4 on the two
        # gradients).  These 64 trajectories therefore hold their attitude -
        # no body rates, rate commands at exactly 0.5 - so that the angles
        # every step's sin / cos see are the same numbers in float32 and
        # float64 and what is left is the evaluation of sin / cos itself (a
        # one-word range reduction is 1.2e-3 rad off at 1e4 rad: it still
        # fails).  The thrust command stays random.
        s0[:64, 9:12] = 0.0
        actions[:64, :, 1:4] = 0.5
    elif kind == "zero":
        s0[:, 3:6] = 0.0
    return dict(state0=s0, actions=actions, ref=d["ref"].clone())


def _oracle(kind, B, H, plan, dtype):
    from oracle import torch_port as tp
    d = {k: v.to(dtype) for k, v in inputs(kind, B, H, plan).items()}
    st, loss, ga, gs = tp.rollout_fwd_bwd(
        tp.QuadOracle(dtype=dtype), tp.quad_mpc_loss, d["state0"], d["actions"],
        d["ref"], DT)
    return dict(states=st.detach().numpy(), loss=float(loss), grad_actions=ga.numpy(),
                grad_state0=gs.numpy())


@functools.lru_cache(maxsize=None)
def oracle64(kind, B, H, plan):
    """states [B,H,12], loss, dL/dactions [B,H,4], dL/dstate0 [B,12] of the
    float64 restatement (oracle/torch_port.py)."""
    return _oracle(kind, B, H, plan, torch.float64)


def oracle32(kind, B, H, plan):
    return _oracle(kind, B, H, plan, torch.float32)
