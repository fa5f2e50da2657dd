"""The two-lane deferred-loss launch chain on the GPU (include/apg.h "launch
chain", csrc/launch_chain.hip): chains of RolloutPlan launches give, after
flush(), exactly what the eager entry points give - launched eagerly, captured
with torch.cuda.graph and replayed on refilled inputs, an eager chain followed
by a captured one on the same stream, and with the results consumed on the
caller's stream right after flush() without a synchronize.  Nothing is timed."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CONFIGS = {                      # system, layout, H, dt
    "quad_packed_h10": ("quad", "packed", 10, 0.1),
    "quad_packed_h5": ("quad", "packed", 5, 0.1),
    "quad_soa_h10": ("quad", "soa", 10, 0.1),
    "wing_soa_h20": ("wing", "soa", 20, 0.05),
}
# a ragged last wave and four partials; 65 partials (more than one per lane of
# the reducing wave)
BATCHES = [64 * 3 + 17, 4096 + 17]
LENGTHS = [1, 2, 3, 4, 7]
NPLANS = [2, 3, 4]
MAX_PLANS = max(NPLANS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def side(dev):
    return torch.cuda.Stream(device=dev)


def _inputs(system, layout, B, H, dt, seed, dev):
    from apg_trajectory_tracking_amd import synthetic as sy
    if system == "wing":
        d = sy.wing_batch(B, H, dt, seed=seed)
        ref = d["ref"]
    else:
        d = sy.quad_polynomial_batch(B, H, dt, seed=seed)
        ref = d["ref"]
    if layout == "packed":
        ref6 = torch.cat((ref[:, :, :3], ref[:, :, 6:9]), 2)
        t = (sy.to_packed_state(d["state0"]), sy.to_packed_seq(d["actions"]),
             sy.to_packed_seq(ref6))
    else:
        t = (sy.to_soa_state(d["state0"]), sy.to_soa_seq(d["actions"]),
             sy.to_soa_seq(ref))
    return tuple(x.contiguous().to(dev) for x in t)


class Case:
    """MAX_PLANS plans of one configuration on the side stream, two versions
    of every plan's inputs and the eager results for both (computed once)."""

    def __init__(self, name, B, dev, side):
        from apg_trajectory_tracking_amd import functional as F
        system, layout, H, dt = CONFIGS[name]
        if system == "wing":
            from apg_trajectory_tracking_amd.dynamics.fixed_wing_dynamics import (
                FixedWingDynamics)
            dyn, eager = FixedWingDynamics(), F.wing_rollout_fwd_bwd
        else:
            from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
                FlightmareDynamics)
            dyn, eager = FlightmareDynamics(), F.quad_rollout_fwd_bwd
        self.dyn = dyn
        self.data = [[_inputs(system, layout, B, H, dt, 10 * v + p, dev)
                      for p in range(MAX_PLANS)] for v in range(2)]
        self.want = [[eager(*t, dt, dyn.params, layout=layout) for t in version]
                     for version in self.data]
        torch.cuda.synchronize()
        self.side = side
        with torch.cuda.stream(side):
            self.plans = [F.RolloutPlan(system, *(x.clone() for x in t), dt, dyn.params,
                                        layout=layout, loss_mode="deferred")
                          for t in self.data[0]]
        torch.cuda.synchronize()

    def refill(self, version, poison=True):
        for p, t in zip(self.plans, self.data[version]):
            for dst, src in zip(p.inputs, t):
                dst.copy_(src)
            if poison:
                p.out["loss"].fill_(-1.0)
                p.out["grad_actions"].fill_(float("nan"))
        torch.cuda.synchronize()

    def chain(self, length, nplans):
        prev = None
        for i in range(length):
            p = self.plans[i % nplans]
            p.launch(after=prev)
            prev = p
        prev.flush()

    def check(self, version, length, nplans, got=None):
        """the launched plans hold the eager results of `version`"""
        for i in range(min(length, nplans)):
            want = self.want[version][i]
            loss, ga = got[i] if got else (self.plans[i].out["loss"],
                                           self.plans[i].out["grad_actions"])
            wl = want["loss"].item()
            assert abs(loss.item() - wl) <= 1e-6 * abs(wl), (version, length, nplans, i)
            assert torch.equal(ga, want["grad_actions"]), (version, length, nplans, i)


_cases = {}


@pytest.fixture
def case(request, dev, side):
    key = request.param
    if key not in _cases:
        _cases[key] = Case(*key, dev, side)
    return _cases[key]


ALL = [(n, B) for n in CONFIGS for B in BATCHES]
IDS = [f"{n}-B{B}" for n, B in ALL]


@pytest.mark.parametrize("case", ALL, ids=IDS, indirect=True)
def test_eager_chains_match_the_eager_entry_points(case):
    """... also when the results are consumed on the caller's stream right
    after flush(), with no synchronize in between: the flush has joined the
    second lane."""
    for nplans in NPLANS:
        for length in LENGTHS:
            case.refill(0)
            with torch.cuda.stream(case.side):
                case.chain(length, nplans)
                got = [(p.out["loss"].clone(), p.out["grad_actions"].clone())
                       for p in case.plans]
            torch.cuda.synchronize()
            case.check(0, length, nplans, got)
            case.check(0, length, nplans)


@pytest.mark.parametrize("case", ALL, ids=IDS, indirect=True)
def test_captured_chains_replay_on_refilled_inputs(case):
    """An eager chain, then the same chain captured on the same stream and
    replayed twice with the inputs refilled in place between the replays."""
    for nplans in NPLANS:
        for length in LENGTHS:
            case.refill(0)
            with torch.cuda.stream(case.side):
                case.chain(length, nplans)
            torch.cuda.synchronize()
            case.check(0, length, nplans)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=case.side):
                case.chain(length, nplans)
            for version in (1, 0):
                case.refill(version)
                g.replay()
                torch.cuda.synchronize()
                case.check(version, length, nplans)
            del g


def test_empty_batch_through_the_chain(dev, side):
    from apg_trajectory_tracking_amd import functional as F
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    dyn = FlightmareDynamics()
    H = 10
    with torch.cuda.stream(side):
        plans = [F.RolloutPlan(
            "quad", torch.empty(12, 0, device=dev), torch.empty(H, 4, 0, device=dev),
            torch.empty(H, 9, 0, device=dev), 0.1, dyn.params, layout="soa",
            loss_mode="deferred") for _ in range(2)]
        for p in plans:
            p.out["loss"].fill_(-1.0)
        plans[0].launch()
        plans[1].launch(after=plans[0])
        plans[0].launch(after=plans[1])
        plans[0].flush()
    torch.cuda.synchronize()
    assert [p.out["loss"].item() for p in plans] == [0.0, 0.0]
    assert plans[0].out["grad_actions"].shape == (H, 4, 0)
