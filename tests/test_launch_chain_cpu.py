"""The bookkeeping of the two-lane launch chain (csrc/launch_chain.h) compiled
for the host (libapg_cpu.so, include/apg_cpu_launch_chain.h): which lane a
launch goes to, which earlier launch's loss its kernel reduces, which
cross-lane event edges it needs, and what the flush still owes.  The steps the
bookkeeping hands out are replayed on a model of two in-order streams with
events; the properties are asserted on that model.  No GPU, no timing."""
import ctypes
import os

import pytest

_P = ctypes.c_void_p


class Reduce(ctypes.Structure):
    _fields_ = [("partials", _P), ("count", ctypes.c_int), ("loss", _P)]


class Step(ctypes.Structure):
    _fields_ = [("lane", ctypes.c_int), ("fork", ctypes.c_int),
                ("pre_lane", ctypes.c_int), ("edge_from", ctypes.c_int),
                ("pre", Reduce), ("fold", Reduce)]


@pytest.fixture(scope="module")
def tw():
    from apg_trajectory_tracking_amd import build as b
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.path.exists(b.LIB_CPU):
        pytest.skip("no hipcc to compile the host twins")
    lib = ctypes.CDLL(b.build_cpu())
    lib.apg_cpu_chain_new.restype = _P
    lib.apg_cpu_chain_free.argtypes = [_P]
    lib.apg_cpu_chain_empty.argtypes = [_P]
    lib.apg_cpu_chain_launch.argtypes = [_P, _P, ctypes.c_int, _P, _P, ctypes.c_int,
                                         _P, ctypes.POINTER(Step)]
    lib.apg_cpu_chain_flush.argtypes = [
        _P, ctypes.POINTER(Reduce), ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(Reduce), ctypes.POINTER(ctypes.c_int), ctypes.c_int,
        ctypes.POINTER(ctypes.c_int)]
    return lib


# plan p: partials at 0x1000 * (p + 1), loss 0x100 above, p + 3 partials
def _partials(p):
    return 0x1000 * (p + 1)


def _loss(p):
    return _partials(p) + 0x100


def _count(p):
    return p + 3


class Model:
    """Two in-order lanes.  `seen[l][m]`: how many operations of lane m are
    known to have completed before the next operation of lane l starts."""

    def __init__(self):
        self.n = [0, 0]                      # operations enqueued per lane
        self.seen = [[0, 0], [0, 0]]
        self.owed = {}                       # plan -> (lane, position) of its unreduced launch
        self.last = {}                       # plan -> (lane, position, reduced at (lane, pos))
        self.reduced_at = {}                 # plan -> (lane, position) of the latest reduction
        self.launches = 0
        self.reductions = 0
        self.edges = 0
        self.lane1_forked = False

    def op(self, lane):
        self.seen[lane][lane] = self.n[lane]
        self.n[lane] += 1
        return self.n[lane] - 1

    def edge(self, src, dst):
        # record on src's tail, wait on dst: dst inherits all src knows
        know = list(self.seen[src])
        know[src] = self.n[src]
        self.seen[dst] = [max(a, b) for a, b in zip(self.seen[dst], know)]

    def ordered_before(self, lane_pos, lane):
        """operation (m, pos) completes before lane's next operation starts"""
        m, pos = lane_pos
        return m == lane or self.seen[lane][m] > pos

    def reduce(self, r, lane):
        plan = r.partials // 0x1000 - 1
        assert (r.partials, r.loss, r.count) == (_partials(plan), _loss(plan), _count(plan))
        assert plan in self.owed, f"plan {plan} reduced twice or before a launch"
        prod_lane, prod_pos = self.owed.pop(plan)
        assert prod_lane == lane, "a reduction runs on its producer's lane"
        pos = self.op(lane)
        assert pos > prod_pos
        self.reduced_at[plan] = (lane, pos)
        self.reductions += 1

    def step(self, s, plan):
        if self.launches == 0:
            assert s.fork and s.lane == 0
            self.n, self.seen = [0, 0], [[0, 0], [0, 0]]
        else:
            assert not s.fork
        if s.pre.loss:
            self.reduce(s.pre, s.pre_lane)
        else:
            assert s.pre_lane == -1
        if s.edge_from >= 0:
            assert s.edge_from == 1 - s.lane
            self.edge(s.edge_from, s.lane)
            self.edges += 1
        # the launch overwrites the plan's buffers: its earlier launch and that
        # launch's reduction are over, by lane order or by an edge
        assert plan not in self.owed, "partials overwritten before they were reduced"
        if plan in self.last:
            assert self.ordered_before(self.last[plan], s.lane)
            assert self.ordered_before(self.reduced_at[plan], s.lane)
        if s.fold.loss:
            assert s.fold.partials != _partials(plan)
            self.reduce(s.fold, s.lane)      # same kernel: position shared below
            self.n[s.lane] -= 1
        pos = self.op(s.lane)
        self.owed[plan] = (s.lane, pos)
        self.last[plan] = (s.lane, pos)
        self.launches += 1


def run_chain(tw, chain, plans, afters, model=None):
    """Launch `plans` (indices) with `afters` (index or None each); returns
    (model, steps)."""
    model = model or Model()
    steps = []
    for p, a in zip(plans, afters):
        s = Step()
        if a is None:
            tw.apg_cpu_chain_launch(chain, _partials(p), _count(p), _loss(p), None, 0,
                                    None, ctypes.byref(s))
        else:
            tw.apg_cpu_chain_launch(chain, _partials(p), _count(p), _loss(p),
                                    _partials(a), _count(a), _loss(a), ctypes.byref(s))
        model.step(s, p)
        steps.append(s)
    return model, steps


def flush(tw, chain, model):
    cap = 16
    r0, r1 = (Reduce * cap)(), (Reduce * cap)()
    n0, n1, join = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    tw.apg_cpu_chain_flush(chain, r0, ctypes.byref(n0), r1, ctypes.byref(n1), cap,
                           ctypes.byref(join))
    assert n0.value <= cap and n1.value <= cap
    for lane, (rs, n) in enumerate(((r0, n0.value), (r1, n1.value))):
        for i in range(n):
            model.reduce(rs[i], lane)
    assert not model.owed, "a loss is still owed after the flush"
    assert model.reductions == model.launches
    assert bool(join.value) == (model.n[1] > 0), "lane 1 is joined iff it was used"
    assert tw.apg_cpu_chain_empty(chain)
    return n0.value, n1.value


@pytest.mark.parametrize("nplans", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("length", range(1, 10))
def test_rotating_plans(tw, nplans, length):
    chain = tw.apg_cpu_chain_new()
    try:
        for _ in range(2):                   # the flushed chain is reusable
            assert tw.apg_cpu_chain_empty(chain)
            plans = [i % nplans for i in range(length)]
            if nplans == 1:                  # a plan cannot follow itself
                afters = [None] * length
            else:
                afters = [None] + plans[:-1]
            model, steps = run_chain(tw, chain, plans, afters)
            assert not tw.apg_cpu_chain_empty(chain)
            # consecutive launches alternate between the lanes
            assert [s.lane for s in steps] == [i % 2 for i in range(length)]
            if nplans in (2, 4):
                assert model.edges == 0      # what the speed-up rests on
            if nplans >= 3:
                # kernel i + 2 carries kernel i's reduction, nothing stands alone
                for i, s in enumerate(steps):
                    assert not s.pre.loss
                    if i >= 2:
                        assert s.fold.partials == _partials(plans[i - 2])
                    else:
                        assert not s.fold.loss
            if nplans % 2 == 1 and nplans > 1 and length > nplans:
                assert model.edges > 0       # the plan returns on the other lane
            n0, n1 = flush(tw, chain, model)
            if nplans > 1:                   # one pending reduction per lane at most
                assert n0 <= 1 and n1 <= 1
    finally:
        tw.apg_cpu_chain_free(chain)


@pytest.mark.parametrize("plans,afters", [
    ([0, 0], [None, None]),                      # relaunched at once, no `after`
    ([0, 1, 1], [None, 0, None]),
    ([0, 1, 0, 0, 1], [None, 0, 1, None, 0]),
    ([0, 1, 2, 2, 0, 1], [None, 0, 1, None, 2, 0]),
    ([0, 1, 2, 0, 0, 0, 1], [None, 0, 1, 2, None, None, 0]),
    ([0, 1, 2, 3, 1, 3, 0], [None, 0, 1, 2, 3, 1, 3]),   # out of rotation
    ([0, 1, 2], [3, 0, 1]),                      # `after` a plan of an earlier chain
    ([0, 1, 2, 3], [None, None, None, None]),    # nothing named: all owed at the flush
])
def test_relaunched_and_irregular_chains(tw, plans, afters):
    chain = tw.apg_cpu_chain_new()
    try:
        for _ in range(2):
            model = Model()
            if afters[0] is not None:        # produced before this chain began
                model.owed[afters[0]] = (0, -1)
                model.launches = 0
                model.reductions = -1
            model, steps = run_chain(tw, chain, plans, afters, model)
            for s, a in zip(steps[1:], afters[1:]):
                if a is not None:            # the lane `after` is not on
                    assert s.lane == 1 - model_lane(steps, plans, a, s)
            flush(tw, chain, model)
    finally:
        tw.apg_cpu_chain_free(chain)


def model_lane(steps, plans, plan, before):
    """lane of the latest launch of `plan` enqueued before step `before`"""
    lane = None
    for s, p in zip(steps, plans):
        if s is before:
            break
        if p == plan:
            lane = s.lane
    return lane
