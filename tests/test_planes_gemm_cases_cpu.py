"""The case table, the restated dispatch and the bounds of
tests/planes_gemm_cases.py, checked without a GPU: the table reaches exactly
the block shapes csrc/planes_gemm.hip instantiates, the Python dispatch agrees
with the library's host functions, and the element-wise bounds of
tests/test_gpu_planes_gemm_shapes.py separate the kernel's arithmetic from the
same arithmetic with any one of its six products missing."""
import os
import re

import numpy as np
import pytest

import planes_gemm_cases as pc
from conftest import REPO

SOURCE = os.path.join(REPO, "apg_trajectory_tracking_amd", "csrc", "planes_gemm.hip")


@pytest.fixture(scope="module")
def cases():
    return pc.accepted_cases()


def _shapes(cases, kind):
    return {pc.kind_of(c)[1:] for c in cases if pc.kind_of(c)[0] == kind}


def test_table_reaches_exactly_the_instantiated_shapes(cases):
    """Every block shape the source instantiates - read from the source: the
    grouped stream kernel's switch, the stream and the LDS-tile launch tables -
    is reached, at both ends of its row and column range, with and without the
    ones column and bias_out; so are the segmented stream path (one case with
    two-level, per-column strides), the two places a row sum can land, LDS-tile
    cases with two-level strides and the rejected combinations."""
    src = open(SOURCE).read()
    grouped = {(int(a), int(b)) for a, b in re.findall(r"APG_STREAM_CASE\((\d+), (\d+)\)", src)}
    tile = {(int(a), int(b)) for a, b in re.findall(r"return launch<(\d+), (\d+)>", src)}
    nbs = {int(n) for n in re.findall(r"launch_stream<MB, (\d+)>", src)}
    assert grouped == pc.STREAM_SHAPES and len(grouped) == 17
    assert tile == pc.TILE_SHAPES and len(tile) == 10
    assert nbs == set(pc.STREAM_NBS)
    assert _shapes(cases, "stream") == pc.STREAM_SHAPES
    assert _shapes(cases, "tile") == pc.TILE_SHAPES
    # both ends of every range, all three states of the ones column per kernel
    for mb, nb in pc.STREAM_SHAPES:
        mine = [c for c in cases if pc.kind_of(c) == ("stream", mb, nb)]
        assert {c.M for c in mine} >= set(pc._M_ENDS[mb]), (mb, nb)
        lo, hi = pc._J_ENDS[nb]
        # both ends exactly; the top J of the last block as a live row WITHOUT
        # the ones column, and next to it where the argument rule admits that
        assert {lo, hi} <= {c.J for c in mine}, (mb, nb)
        top = [c for c in mine if c.M == pc._M_ENDS[mb][1] and c.J >= hi - 1]
        if pc.check_problem(pc._M_ENDS[mb][1], 1, hi, True):
            assert {(c.J, c.ones) for c in top} == {(hi, False), (hi - 1, True)}, (mb, nb)
    # the ones column is tied to no end of a range
    low = {c.J for c in cases if c.S == 1 and c.ones} & {lo for lo, _ in pc._J_ENDS.values()}
    assert len(low) >= 3, low
    for MB, NB in pc.TILE_SHAPES:
        jt = {c.J + c.ones for c in cases if pc.kind_of(c) == ("tile", MB, NB)}
        assert 32 * NB in jt and max(32 * (NB - 1) + 1, 17) in jt, (MB, NB)
    assert {c.M for c in cases if pc.kind_of(c)[0] == "tile"} >= {32, 33, 64}
    for kind in ("stream", "tile"):
        states = {(c.ones, c.bias) for c in cases if pc.kind_of(c)[0] == kind}
        assert states == {(False, False), (True, False), (True, True)}, kind
    ones_col = {(c.J, c.bias) for c in cases if c.S == 1 and c.ones and c.M == 16}
    assert ones_col >= {(15, False), (15, True), (16, False), (16, True)}
    seg = [c for c in cases if pc.kind_of(c)[0] == "segmented"]
    assert {(c.M, c.S, c.J) for c in seg} == {(20, 10, 3), (64, 3, 15)}
    assert any(c.sdiv > 1 and len(set(c.s1)) > 1 and len(set(c.s2)) > 1 for c in seg)
    assert sum(c.sdiv > 1 for c in cases if pc.kind_of(c)[0] == "tile") >= 1
    assert all(c.S >= 2 and c.J >= 16 for c in cases if pc.kind_of(c)[0] == "tile")
    rej = set(pc.REJECTED)
    assert {(33, 1, 129, False), (64, 1, 128, True)} <= rej
    assert any(J + ones == 193 for _, _, J, ones in rej)
    for M, S, J, ones in rej:
        with pytest.raises(ValueError):
            pc.dispatch(M, S, J, ones)
    # descriptors stay inside B, names are unique (they label the parametrised tests)
    assert len({c.name for c in cases}) == len(cases)
    assert all(min(c.offs) >= 0 and pc.b_planes(c) <= 400 for c in cases)


def test_dispatch_agrees_with_the_library():
    """apg_planes_gemm_workspace_floats and apg_planes_gemm_default_wgs for
    every (M, J, ones) against the restated dispatch; the rejected combinations
    return APG_ERR_ARG with a message before anything touches a device."""
    from apg_trajectory_tracking_amd import _capi
    lib = _capi.lib()
    for M in range(1, pc.MAX_M + 1):
        for J in range(1, pc.MAX_JT + 1):
            for ones in (0, 1):
                got = lib.apg_planes_gemm_workspace_floats(M, J, ones, 1)
                assert got == pc.workspace_floats(M, J, ones, 1), (M, J, ones)
    assert lib.apg_planes_gemm_workspace_floats(33, 70, 1, 5) == 5 * pc.workspace_floats(33, 70, 1, 1)
    # the kernel choice shows in the default grid: the smallest stream shape
    # gets four workgroups per CU, every other stream shape one
    one = lib.apg_planes_gemm_default_wgs(64, 1, 112, 0)
    for M, S, J in ((1, 1, 16), (16, 5, 15), (17, 1, 16), (16, 1, 17), (64, 3, 15)):
        k, mb, nb = pc.dispatch(M, S, J, 0)
        assert k == "stream"
        assert lib.apg_planes_gemm_default_wgs(M, S, J, 0) == one * (4 if mb + nb <= 2 else 1)
    # real host buffers, and the message of the RANGE rule: a product the rule
    # let through by mistake would fail here, before the assertion on the
    # return value could hide that a launch had been tried
    for M, S, J, ones in pc.REJECTED:
        assert pc.check_problem(M, S, J, ones)
        A = np.zeros((M * S, 64), np.float32)
        Bp = np.zeros((J, 64), np.float32)
        desc = np.zeros((3, J), np.int32)
        desc[0] = np.arange(J)
        C = np.zeros((M, J + 1), np.float32)
        ws = np.zeros(pc.workspace_floats(M, J, ones, 1), np.float32)
        rc = lib.apg_planes_gemm(A.ctypes.data, M, S, Bp.ctypes.data, desc.ctypes.data, J, 1,
                                 int(ones), J, 64, ws.ctypes.data, 1, C.ctypes.data, J + 1,
                                 None, None)
        msg = lib.apg_last_error_string()
        assert rc == -1 and b"apg_planes_gemm: need 1 <= M <= 64, J + ones <= 192" in msg, (
            M, S, J, ones, rc, msg)
        assert not C.any()


def _aligned(c):
    N = pc.PLAN["aligned", pc.kind_of(c)[0]][0]
    A, Bp = pc.operands(c, "aligned", N)
    return A, Bp, pc.reference(c, A, Bp)


def test_aligned_constants():
    pool = pc.aligned_pool()
    h, m, l = pc.split3(pool)
    assert len(np.unique(pool)) == len(pool) >= pc.MAX_M + 400
    assert (pool >= 1).all() and (pool < 2).all()
    assert (m >= pc.M_MIN * pool).all() and (l >= pc.L_MIN * pool).all()
    assert pc.M_MIN >= 0.71 * 2.0 ** -9 and pc.L_MIN >= 0.5 * 2.0 ** -17
    print("aligned pool: %d of 200000 draws (1 in %.1f)" % (len(pool), 2e5 / len(pool)))
    assert 2e5 / len(pool) < 60


def test_six_products_reach_fp32_rounding_on_every_aligned_case(cases):
    """The kernel's arithmetic with exact sums: element-wise error < 2^-22 on
    every element of every aligned case (measured: 0.21 2^-22)."""
    worst = 0.0
    for c in cases:
        A, Bp, (ref, sab) = _aligned(c)
        assert A.dtype == np.float32 and ref.shape == (c.M, c.J + c.ones)
        e = pc.elementwise_err(pc.emulate(c, A, Bp), ref, sab)
        worst = max(worst, e.max())
        assert e.max() < 2.0 ** -22, (c.name, e.max() * 2.0 ** 22)
    print("six products, aligned: worst %.3f x 2^-22" % (worst * 2.0 ** 22))
    assert worst < 0.25 * 2.0 ** -22     # what the GPU bound's count starts from


def test_every_missing_product_moves_every_aligned_element(cases):
    """Without any one of the six products EVERY element of C (the row sums do
    not come from the products) is off by >= 2^-19 - twice the GPU bound of
    2^-20: that bound tells a kernel with a lost product from a whole one."""
    least = np.inf
    for c in cases:
        A, Bp, (ref, sab) = _aligned(c)
        for k in range(6):
            e = pc.elementwise_err(pc.emulate(c, A, Bp, drop=k), ref, sab)[:, :c.J]
            least = min(least, e.min())
            assert e.min() >= pc.DROP_ONE_MIN, (c.name, pc.PRODUCTS[k], e.min() * 2.0 ** 22)
    print("drop one, aligned: least %.3f x 2^-22" % (least * 2.0 ** 22))
    assert pc.ALIGNED_BOUND <= 0.75 * pc.DROP_ONE_MIN


def test_decades_bound_sees_a_missing_middle_product(cases):
    """Decades operands: the full emulation stays under 2^-22 on every case
    (so under every decades bound, 4 + R roundings); without a product of
    weight 2^-8 - (m, h) or (h, m) - the bound of the all-cases test fails, and
    conftest.rel_err's 1e-5 of the largest entry would not have seen the rows
    that are small."""
    for c in cases:
        N = pc.PLAN["decades", pc.kind_of(c)[0]][0]
        A, Bp = pc.operands(c, "decades", N)
        ref, sab = pc.reference(c, A, Bp)
        assert np.isfinite(ref).all() and (sab > 0).all()
        e = pc.elementwise_err(pc.emulate(c, A, Bp), ref, sab)
        assert e.max() <= 2.0 ** -22, (c.name, e.max() * 2.0 ** 24)
    c = next(c for c in cases if (c.M, c.J) == (64, 112))
    A, Bp = pc.operands(c, "decades", 100)
    ref, sab = pc.reference(c, A, Bp)
    bound = pc.decades_bound(pc.stream_roundings(100, 1, 256))
    assert bound == 14 * pc.U
    for k in (3, 4):
        e = pc.elementwise_err(pc.emulate(c, A, Bp, drop=k), ref, sab)
        assert e.max() > 50 * bound, (k, e.max())
    rows = np.abs(ref).max(1)
    assert rows.max() / rows.min() > 1e12          # what "decades" means


def test_rounding_counts():
    """R of the configurations the GPU tests use."""
    assert pc.stream_roundings(100, 1, 1) == 10 and pc.stream_roundings(96, 1, 256) == 10
    assert [pc.stream_chunks_per_wave(n, 1, 1) for n in (100, 130, 300, 777)] == [1, 2, 3, 7]
    assert [pc.stream_chunks_per_wave(n, 1, 2) for n in (100, 130, 300, 777)] == [1, 1, 2, 4]
    assert pc.stream_chunks_per_wave(777, 10, 1) == 63
    assert [pc.tile_tiles_per_wg(n, 2, 1) for n in (64, 128, 150, 256, 300)] == [2, 4, 6, 8, 10]
    assert pc.tile_tiles_per_wg(200, 2, 512) == 1 and pc.tile_tiles_per_wg(200, 6, 1024) == 1
    assert pc.tile_roundings(200, 2, 512) == 20
    assert pc.tile_aligned_roundings(64, 2, 512) == 12.5 <= pc.ALIGNED_MAX_R
    assert pc.tile_aligned_roundings(8, 6, 1024) == 4.5 + 4
    assert pc.stream_roundings(100, 1, 1) + 0.85 + 0.15 <= pc.ALIGNED_BOUND / pc.U
