"""Every block shape of csrc/planes_gemm.hip on the device, element by element
against float64: the 17 instances of the register-streaming kernel (alone and
through the grouped stream kernel's switch), the 10 of the LDS-tile kernel and
the segmented stream path, on the cases, operand families and bounds of
tests/planes_gemm_cases.py (tests/test_planes_gemm_cases_cpu.py shows on the
CPU that these bounds tell a lost bf16 product from a whole kernel); the
double-buffered loops of both kernels at 1 to 7 trips with a ragged last one;
bit-for-bit repeatability; and the rejected combinations.

Order: the shapes the full-size step tests already run come first.  Every test
prints what it measured (pytest -s); profiles/planes_gemm_elementwise.jsonl
records it (tools/planes_gemm_elementwise.py)."""
import numpy as np
import pytest
import torch

import planes_gemm_cases as pc

pytestmark = pytest.mark.gpu

CASES = pc.accepted_cases()
# <1,1>, <1,4>, <2,12>, <4,1>, <4,4>, <4,7> and the tile shapes <1,1>, <2,4> run in
# the suite's other tests: they go first
_KNOWN = {("stream", 1, 1), ("stream", 1, 4), ("stream", 2, 12), ("stream", 4, 1),
          ("stream", 4, 4), ("stream", 4, 7), ("segmented", 2, 1), ("tile", 1, 1),
          ("tile", 2, 4)}
ORDERED = sorted(CASES, key=lambda c: (pc.kind_of(c) not in _KNOWN, pc.kind_of(c)[0] == "tile"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def F():
    from apg_trajectory_tracking_amd import functional
    return functional


def _lib():
    from apg_trajectory_tracking_amd import _capi
    return _capi.lib()


def _check(c, family, err, bound, R, what=""):
    worst = float(err.max())
    m, j = np.unravel_index(int(err.argmax()), err.shape)
    print("%s %s %s: worst %.2f x 2^-24 at (%d, %d), bound %.0f (R = %g)" % (
        c.name, family, what, worst / pc.U, m, j, bound / pc.U, R))
    assert worst <= bound, (c.name, family, what, worst / pc.U, bound / pc.U, (m, j))


# ------------------------------------------- 1. every case, both families
@pytest.mark.parametrize("family", ["aligned", "decades"])
@pytest.mark.parametrize("c", ORDERED, ids=[c.name for c in ORDERED])
def test_every_case_elementwise(dev, F, c, family):
    """functional.planes_gemm on every case of the table.  aligned: every
    element of C and every row sum within 2^-20 of its own sum |a||b| (at most
    15 roundings by the choice of N and grid; a lost product is >= 2^-19); decades:
    within (4 + R) 2^-24.  The view's surroundings stay NaN, the view itself
    holds no NaN.  (Measured: profiles/planes_gemm_elementwise.jsonl.)"""
    N, wgs = pc.PLAN[family, pc.kind_of(c)[0]]
    err, C = pc.run_case(F, dev, c, family, N, wgs)
    bound, R = pc.bound_of(c, family, N, wgs or pc.default_wgs(_lib(), c))
    assert np.isfinite(C).all(), c.name
    _check(c, family, err, bound, R)


# ------------------------------------------------------- 2. loop depth
_BY_SHAPE = {}          # the case with the largest (M, J) of every shape
for _c in sorted(CASES, key=lambda c: (c.M, c.J)):
    _BY_SHAPE[pc.kind_of(_c)] = _c
STREAM_DEPTH = [_BY_SHAPE["stream", 1, 1], _BY_SHAPE["stream", 4, 7],
                _BY_SHAPE["stream", 2, 12], _BY_SHAPE["segmented", 2, 1]]


@pytest.mark.parametrize("wgs", [1, 2])
@pytest.mark.parametrize("c", STREAM_DEPTH, ids=[c.name for c in STREAM_DEPTH])
def test_stream_loop_depth(dev, F, c, wgs):
    """1 to 7 chunks per wave (63 for the segmented case): both exits of the
    double-buffered loop, ragged last chunks, segment boundaries inside a
    wave's stride.  Decades operands, the bound of the configuration's R."""
    trips = set()
    for N in (100, 130, 300, 777):
        err, C = pc.run_case(F, dev, c, "decades", N, wgs, seed=N)
        bound, R = pc.bound_of(c, "decades", N, wgs)
        trips.add(pc.stream_chunks_per_wave(N, c.S, wgs))
        _check(c, "decades", err, bound, R, "N %d, %d workgroups" % (N, wgs))
    if c.S == 1:
        assert trips == ({1, 2, 3, 7} if wgs == 1 else {1, 2, 4})


TILE_DEPTH = [_BY_SHAPE["tile", 1, 1], _BY_SHAPE["tile", 2, 4], _BY_SHAPE["tile", 1, 6],
              _BY_SHAPE["tile", 2, 1]]


@pytest.mark.parametrize("c", TILE_DEPTH, ids=[c.name for c in TILE_DEPTH])
def test_tile_loop_depth(dev, F, c):
    """One workgroup, 1 to 5 tiles per segment: both parities of the LDS ring,
    a ragged last tile, the tiles of the segments interleaved."""
    for N in (64, 128, 150, 256, 300):
        S = c.S
        assert pc.tile_tiles_per_wg(N, S, 1) == S * -(-N // 64)
        err, C = pc.run_case(F, dev, c, "decades", N, 1, seed=N)
        bound, R = pc.bound_of(c, "decades", N, 1)
        _check(c, "decades", err, bound, R, "N %d, one workgroup" % N)


# ------------------------------------------- 3. the grouped stream launch
@pytest.mark.parametrize("family", ["aligned", "decades"])
@pytest.mark.parametrize("call", [0, 1, 2])
def test_grouped_stream_launch_runs_every_shape(dev, F, call, family):
    """planes_gemm_multi with 5 or 6 plain products of short planes: ONE launch
    of planes_gemm_stream_grouped_kernel, whose switch restates the 17 shapes.
    Outputs are strided views pre-filled with NaN (a case of the switch that
    does nothing leaves its partials uninitialised or its output NaN), row sums
    go to their own vectors.  N = 100: four chunks, at most one per wave
    whatever share of the grid a product gets, so R = 10."""
    N = 100
    cs = pc.grouped_calls(CASES)[call]
    assert len(cs) >= 2 and N <= 262144
    ops = [pc.operands(c, family, N, seed=50 + i) for i, c in enumerate(cs)]
    ps = [pc.problem(F, dev, c, A, Bp, pad=(2, 1 + i, 4)) for i, (c, (A, Bp)) in
          enumerate(zip(cs, ops))]
    F.planes_gemm_multi([p["kw"] for p in ps])
    for c, (A, Bp), p in zip(cs, ops, ps):
        C = pc.result(c, p)
        assert np.isfinite(C).all(), c.name
        err = pc.elementwise_err(C, *pc.reference(c, A, Bp))
        bound, R = pc.bound_of(c, family, N, 1)
        assert R == 10
        _check(c, family, err, bound, R, "grouped")


# ------------------------------------------------------ 4. determinism
def test_results_repeat_bit_for_bit(dev, F):
    """The file states a fixed summation order: a stream product, an LDS-tile
    product and a grouped multi call give identical bits twice."""
    for c, N in ((_BY_SHAPE["stream", 4, 7], 777), (_BY_SHAPE["tile", 2, 4], 300),
                 (_BY_SHAPE["segmented", 2, 1], 300)):
        a = pc.run_case(F, dev, c, "decades", N, None, seed=3)[1]
        b = pc.run_case(F, dev, c, "decades", N, None, seed=3)[1]
        assert np.array_equal(a, b), c.name
    cs = pc.grouped_calls(CASES)[1]
    runs = []
    for _ in range(2):
        ps = [pc.problem(F, dev, c, *pc.operands(c, "decades", 500, seed=9)) for c in cs]
        F.planes_gemm_multi([p["kw"] for p in ps])
        runs.append([pc.result(c, p) for c, p in zip(cs, ps)])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------- 5. rejected combinations
@pytest.mark.parametrize("M,S,J,ones", pc.REJECTED)
def test_rejected_combinations_raise_and_write_nothing(dev, F, M, S, J, ones):
    A = torch.ones(M * S, 64, device=dev)
    Bp = torch.ones(J, 64, device=dev)
    out = torch.full((M, J + 1), 7.0, device=dev)
    bias = torch.full((M,), 7.0, device=dev)
    with pytest.raises(ValueError):
        pc.dispatch(M, S, J, ones)
    for b in (None, bias):
        with pytest.raises(ValueError):
            F.planes_gemm(A, M, S, Bp, F.make_bdesc(dev, range(J)), with_ones=ones,
                          out=out, bias_out=b)
    with pytest.raises(ValueError):
        ok = torch.full((16, 17), 7.0, device=dev)
        F.planes_gemm_multi([
            dict(A=A[:16], M=16, S=1, Bp=Bp, bdesc=F.make_bdesc(dev, range(16)), out=ok),
            dict(A=A, M=M, S=S, Bp=Bp, bdesc=F.make_bdesc(dev, range(J)), with_ones=ones,
                 out=out)])
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((bias == 7).all()) and bool((ok == 7).all())
