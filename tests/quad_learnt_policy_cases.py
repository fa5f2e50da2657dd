"""The cases of the concurrent controller step through the learnt quadrotor
simulator (functional.quad_learnt_concurrent_policy_grads), shared by
tests/test_quad_learnt_policy_cpu.py - which holds their conditions on the float64
oracle alone - and tests/test_gpu_quad_learnt_policy.py.

  policy      torch.manual_seed(8); Net(15, 10, 9, 40, conv=1)
  pool        synthetic.quad_polynomial_batch(600, 10, learnt_dt(), seed=900)
  simulators  quad_loss_cases.learnt_weights(golden | steps | strong), each with
              linear_at += 0.1 randn(4, 4) (Generator().manual_seed(9)): the
              goldens' action transform is close to the identity, and a kernel
              that applied it transposed - or not at all - would stay inside the
              tolerance without it
  oracle      autograd over Net + tp.quad_state_features + tp.LearntQuadOracle +
              tp.quad_mpc_loss, every part of which is pinned to the reference's
              goldens elsewhere in the suite
  batches     the first B pool rows off a ReLU kink of the residual network
              (quad_loss_cases' rule, KINK = 1e-5, along the oracle's own unroll)

Not a test module (no test_ prefix)."""
import copy
import functools

import numpy as np
import torch

from oracle import torch_port as tp
from quad_loss_cases import KINK, LEARNT_INIT, MAX_KINK_SHARE, learnt_dt, learnt_weights

H, POOL = 10, 600
SIMS = ("golden", "steps", "strong")
SIZES = (1, 33, 257, 515)     # one lane pair | ragged 2nd wave | ragged 2nd workgroup | 3 workgroups
# the GPU bars (tests/test_gpu_in_sweep.py's) and what the float32 oracle must
# stay under for them to be reachable
LOSS_BAR, GRAD_BAR = 1e-5, 1e-4
MIN_MOVE = 1e-2               # what leaving out the residual / the transform must move


@functools.lru_cache(maxsize=None)
def policy():
    from apg_trajectory_tracking_amd.models.hutter_model import Net
    torch.manual_seed(8)
    return Net(15, H, 9, 4 * H, conv=1)


@functools.lru_cache(maxsize=None)
def pool():
    from apg_trajectory_tracking_amd import synthetic
    return synthetic.quad_polynomial_batch(POOL, H, learnt_dt(), seed=900)


def at_perturbation(seed=9):
    return (0.1 * torch.randn(4, 4, generator=torch.Generator().manual_seed(seed))).numpy()


def sim_weights(which, transform=True, residual=True):
    """The state_dict (numpy) of simulator `which`; transform False: without the
    linear_at perturbation; residual False: the residual's output layer zeroed."""
    w = {k: np.array(v, dtype=np.float32) for k, v in learnt_weights(which).items()}
    if transform:
        w["linear_at"] = (w["linear_at"] + at_perturbation()).astype(np.float32)
    if not residual:
        w["linear_state_2.weight"] = np.zeros_like(w["linear_state_2.weight"])
        w["linear_state_2.bias"] = np.zeros_like(w["linear_state_2.bias"])
    return w


def module(weights, dev):
    """A LearntDynamics carrying `weights` on `dev`."""
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_trained import LearntDynamics
    dyn = LearntDynamics(initial_params=dict(LEARNT_INIT))
    res = dyn.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in weights.items()})
    assert not res.missing_keys and not res.unexpected_keys
    return dyn.to(dev)


def oracle_run(weights, net, rows, dtype=torch.float64):
    """The step on pool rows `rows` in `dtype` -> dict(loss, grads {name: float64
    array}, actions [B,H,4], states [B,H,12], grad_actions [B,H,4], kink [B])."""
    d = pool()
    rows = torch.as_tensor(rows, dtype=torch.long)
    s0, in_ref, ref = (d[k][rows].to(dtype) for k in ("state0", "in_ref", "ref"))
    n = copy.deepcopy(net).to(dtype)
    ora = tp.LearntQuadOracle(weights, initial_params=dict(LEARNT_INIT), dtype=dtype)
    acts = torch.sigmoid(n(tp.quad_state_features(s0), in_ref)).reshape(-1, H, 4)
    acts.retain_grad()
    kink = torch.zeros(len(rows), dtype=torch.bool)
    cur, inter = s0, []
    for k in range(H):
        with torch.no_grad():
            x = torch.cat((cur, (ora.A @ acts[:, k].unsqueeze(2))[:, :, 0]), 1)
            z = x @ ora.w1.t() + ora.b1
            scale = ora.b1.abs() + x.abs() @ ora.w1.abs().t()
            kink.logical_or_((z.abs() < KINK * scale).any(1))
        cur = ora(cur, acts[:, k], learnt_dt())
        inter.append(cur)
    states = torch.stack(inter, 1)
    loss = tp.quad_mpc_loss(states, ref[:, :H], acts)
    loss.backward()
    f = lambda t: t.detach().double().numpy()
    return dict(loss=float(loss.detach()), actions=f(acts), states=f(states),
                grad_actions=f(acts.grad), kink=kink.numpy(),
                grads={k: f(p.grad) for k, p in n.named_parameters() if p.grad is not None})


@functools.lru_cache(maxsize=None)
def pool_kinks(which):
    """[POOL] bool: the pool rows on a kink under simulator `which`."""
    return oracle_run(sim_weights(which), policy(), range(POOL))["kink"]


def batch_rows(which, B, also=()):
    """The first B pool rows off a kink (`also`: further [POOL] kink masks - of a
    simulator the same batch is run through later)."""
    bad = pool_kinks(which).copy()
    for m in also:
        bad |= m
    rows = np.flatnonzero(~bad)[:B]
    assert len(rows) == B
    return rows


@functools.lru_cache(maxsize=None)
def oracle(which, B, dtype=torch.float64, transform=True, residual=True):
    """oracle_run of the batch (`which`, B) - the rows are those of the FULL
    simulator whatever `transform` / `residual` leave out."""
    return oracle_run(sim_weights(which, transform, residual), policy(), batch_rows(which, B),
                      dtype)


def batch(which, B, dev=None, ref_cols=9):
    """-> (rows, dict of the batch's float32 tensors: normed, state0, in_ref, ref)."""
    from quad_loss_cases import packed_ref
    d = pool()
    rows = batch_rows(which, B)
    r = torch.as_tensor(rows, dtype=torch.long)
    out = dict(state0=d["state0"][r], in_ref=d["in_ref"][r], ref=d["ref"][r][:, :H])
    out["normed"] = tp.quad_state_features(out["state0"])
    if ref_cols == 6:
        out["ref"] = packed_ref(out["ref"])
    out = {k: v.contiguous() for k, v in out.items()}
    if dev is not None:
        out = {k: v.to(dev) for k, v in out.items()}
    return rows, out


def moved(a, b):
    """{name: conftest.rel_err of gradient a against b}."""
    from conftest import rel_err
    return {k: rel_err(a[k], b[k]) for k in b}
