"""Cases, operands, references and bounds for the block-shape tests of
csrc/planes_gemm.hip (test_planes_gemm_cases_cpu.py, test_gpu_planes_gemm_shapes.py).

The file builds 17 instances of the register-streaming kernel
(planes_gemm_stream_kernel<MB, NB>, restated as a `switch` in the grouped
stream kernel) and 10 of the LDS-tile kernel (planes_gemm_kernel<MB, NB>).  The
table here reaches every one of them with tiny products, at both ends of its
row and column range, and judges the result ELEMENT BY ELEMENT:

    elementwise_err = |C - ref64| / (|A| @ |B|^T)

against a bound counted in fp32 roundings.  conftest.rel_err (largest error
over the tensor's largest entry, < 1e-5) passes a stream kernel that has lost
any one of its three low bf16 products; this measure does not (the aligned
operand family below makes every one of the six products worth >= 2^-19 of
EVERY element).

A helper module, not a conftest: it holds no fixture and changes no setting.
Nothing here needs a GPU; run_case() takes the device from its caller."""
import collections
import math

import numpy as np

# ------------------------------------------------ the dispatch, restated
MAX_M, MAX_JT = 64, 192
STREAM_MBS, STREAM_NBS = (1, 2, 4), (1, 2, 4, 7, 8, 12)
STREAM_SHAPES = frozenset((mb, nb) for mb in STREAM_MBS for nb in STREAM_NBS
                          if (mb, nb) != (4, 12))                     # 17
TILE_SHAPES = frozenset([(1, nb) for nb in range(1, 7)]
                        + [(2, nb) for nb in range(1, 5)])            # 10


def use_stream(S, J):
    """Plain products, and segmented ones with fewer than 16 B rows."""
    return S == 1 or J < 16


def stream_mb(M):
    b = (M + 15) // 16
    return 1 if b <= 1 else 2 if b <= 2 else 4


def stream_nb(J):
    b = (J + 15) // 16
    return next((nb for nb in STREAM_NBS if b <= nb), STREAM_NBS[-1])


def tile_blocks(M, J, ones):
    return (M + 31) // 32, (J + int(ones) + 31) // 32


def check_problem(M, S, J, ones):
    """None, or why apg_planes_gemm refuses the product: the argument rule is
    the LDS-tile kernel's for both kernels (it also keeps <4, 12> away from the
    stream kernel)."""
    MB, NB = tile_blocks(M, J, ones)
    if M < 1 or M > MAX_M or S < 1 or J < 1 or J + int(ones) > MAX_JT:
        return "range"
    if MB == 2 and NB > 4:
        return "more than 128 columns need M <= 32"
    return None


def dispatch(M, S, J, ones):
    """("stream" | "tile", MB, NB) of an accepted product; ValueError otherwise."""
    why = check_problem(M, S, J, ones)
    if why:
        raise ValueError(why)
    if use_stream(S, J):
        return ("stream", stream_mb(M), stream_nb(J))
    return ("tile",) + tile_blocks(M, J, ones)


def partial_floats(M, S, J, ones):
    """Floats of one workgroup's partial C (no argument check, as the library)."""
    if use_stream(S, J):
        return stream_mb(M) * 16 * (stream_nb(J) * 16 + 1)
    MB, NB = tile_blocks(M, J, ones)
    return MB * 32 * NB * 32


def workspace_floats(M, J, ones, num_wg):
    """apg_planes_gemm_workspace_floats: enough for either kernel."""
    return num_wg * max(partial_floats(M, 1, J, ones), partial_floats(M, 2, J, ones))


# ------------------------------------------------------------ the case table
Case = collections.namedtuple(
    "Case", "name M S J ones bias sdiv offs s1 s2")   # bias: row sums to bias_out


def _case(name, M, S, J, ones, bias, sdiv=1, offs=None, s1=None, s2=0):
    if offs is None:           # columns in reverse plane order, two planes unused in front
        offs = [2 + (J - 1 - j) for j in range(J)]
    if s1 is None:             # every segment its own set of planes
        s1 = J if S > 1 else 0
    bc = lambda v: tuple(int(x) for x in v) if hasattr(v, "__len__") else (int(v),) * J
    return Case(name, M, S, J, bool(ones), bool(bias and ones), sdiv,
                tuple(offs), bc(s1), bc(s2))


def bplane(c, j, s):
    return c.offs[j] + (s // c.sdiv) * c.s1[j] + (s % c.sdiv) * c.s2[j]


def b_planes(c):
    """Planes of the B tensor of a case: one more than the last one it reads."""
    return 2 + max(bplane(c, j, s) for j in range(c.J) for s in range(c.S))


_M_ENDS = {1: (1, 16), 2: (17, 32), 4: (33, 64)}
_J_ENDS = {1: (1, 16), 2: (17, 32), 4: (33, 64), 7: (65, 112), 8: (113, 128),
           12: (129, 192)}


def _ones_state(i):
    """(with_ones, bias_out given): three states in turn.  A shape has four
    corners and two ends, so the state is tied neither to the shape nor to an
    end of the row or column range."""
    return ((False, False), (True, False), (True, True))[i % 3]


def stream_cases():
    """S = 1: every legal <mb, nb> at the four corners of its (M, J) range.
    Where the ones column does not fit beside the top J (192; 128 for M > 32:
    the argument rule), the corner is run twice: the top J without the ones
    column - the last live B row of the last block - and one J less with it."""
    out, i = [], 0
    for mb in STREAM_MBS:
        for nb in STREAM_NBS:
            if (mb, nb) not in STREAM_SHAPES:
                continue
            for M in _M_ENDS[mb]:
                for J in _J_ENDS[nb]:
                    ones, bias = _ones_state(i)
                    i += 1
                    if ones and check_problem(M, 1, J, True):
                        out.append(_case(f"stream<{mb},{nb}> M{M} J{J}", M, 1, J, False, False))
                        J -= 1
                    out.append(_case(f"stream<{mb},{nb}> M{M} J{J}", M, 1, J, ones, bias))
    # row sums in a dead accumulator column (J = 15) and in the extra one (J = 16)
    for J in (15, 16):
        for bias in (False, True):
            out.append(_case(f"stream ones-column J{J} bias{int(bias)}", 16, 1, J, True, bias))
    return out


def tile_cases():
    """S >= 2, J >= 16: the ten <MB, NB> of the LDS-tile kernel with J + ones on
    both sides of every multiple of 32; two of them with two-level strides."""
    out, i = [], 0
    for MB, Ms in ((1, (20, 32)), (2, (33, 64))):
        for NB in range(1, 7 if MB == 1 else 5):
            for k, Jt in enumerate((max(32 * (NB - 1) + 1, 17), 32 * NB)):
                ones, bias = _ones_state(i)
                i += 1
                out.append(_case(f"tile<{MB},{NB}> M{Ms[k]} Jt{Jt}", Ms[k], 2,
                                 Jt - int(ones), ones, bias))
    # segment = (window position, step): sliding windows shared between segments
    # plus three columns with strides of their own, as the conv-weight gradient
    offs = [t * 9 + c for c in range(9) for t in range(3)] + [70, 71, 72]
    out.append(_case("tile<1,1> two-level M20 S6", 20, 6, 30, True, True, sdiv=3,
                     offs=offs, s1=[9] * 27 + [0] * 3, s2=[9] * 27 + [12] * 3))
    J = 70
    out.append(_case("tile<2,3> two-level M40 S4", 40, 4, J, True, False, sdiv=2,
                     offs=[1 + j for j in range(J)],
                     s1=[J + (j % 3) for j in range(J)], s2=[2 * J + 5 + (j % 2) for j in range(J)]))
    return out


def segmented_stream_cases():
    """S > 1 with fewer than 16 B rows: the stream kernel walks the segments."""
    return [
        _case("stream segmented M20 S10 J3", 20, 10, 3, True, True, sdiv=5,
              offs=[0, 1, 2], s1=[0, 3, 7], s2=[12, 5, 1]),
        _case("stream segmented M64 S3 J15", 64, 3, 15, False, False),
    ]


def accepted_cases():
    return stream_cases() + tile_cases() + segmented_stream_cases()


def grouped_calls(cases=None):
    """The 17 stream shapes, each by its case with the largest M and J, in
    three planes_gemm_multi calls of 6, 6 and 5 products; neighbours in a call
    differ in both block counts."""
    top = {}
    for c in sorted(cases or stream_cases(), key=lambda c: (c.M, c.J)):
        if c.S == 1:
            top[kind_of(c)[1:]] = c
    assert set(top) == STREAM_SHAPES
    cs = [top[s] for s in sorted(top)]
    cs = cs[0::3] + cs[1::3] + cs[2::3]
    return [cs[0:6], cs[6:12], cs[12:17]]


# (M, S, J, with_ones) that apg_planes_gemm must refuse without a launch
REJECTED = (
    (33, 1, 129, False),     # <4, 12> is not built
    (64, 1, 128, True),      # M > 32: J + ones <= 128
    (16, 1, 192, True),      # J + ones = 193
    (32, 2, 193, False),
)


def kind_of(c):
    """stream / tile / segmented, with the block shape."""
    k, mb, nb = dispatch(c.M, c.S, c.J, c.ones)
    return ("segmented" if k == "stream" and c.S > 1 else k), mb, nb


# ------------------------------------------------------------ operands
def bf16(x):
    """fp32 -> bf16 -> fp32, to nearest even (v_cvt_pk_bf16_f32)."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    """(h, m, l): the three bf16 terms of csrc/planes_gemm.hip's split3."""
    x = np.ascontiguousarray(x, np.float32)
    h = bf16(x)
    r = x - h                    # exact in fp32
    m = bf16(r)
    return h, m, bf16(r - m)     # exact difference, rounded once more


# Thresholds of the aligned constants, as shares of x: m >= M_MIN, l >= L_MIN
# (both positive: every term of every product is, so no running sum exceeds
# sum |a||b|).
# The smallest of the six products is then (m, m) >= 0.73^2 2^-18 = 1.066 2^-19
# of the element and (l, h), (h, l) >= 0.5 2^-17 (1 - 2^-8) = 1.99 2^-19.  (0.71
# gives 1.008 2^-19, less than 2^-19 once the 0.03 2^-19 that the six products
# themselves miss is taken off; 0.73 keeps the drop-one error above 2^-19.)
M_MIN, L_MIN = 0.73 * 2.0 ** -9, 0.5 * 2.0 ** -17
_POOL = []


def aligned_pool():
    """Distinct fp32 constants in [1, 2) whose middle and low bf16 terms are at
    least M_MIN and L_MIN of the value: about 1 draw in 34 of 200 000 (1 in 8.6
    with either sign admitted)."""
    if not _POOL:
        x = np.unique((1 + np.random.default_rng(2024).random(200000)).astype(np.float32))
        x = x[x < 2]
        h, m, l = split3(x)
        ok = (m >= M_MIN * x) & (l >= L_MIN * x)
        pool = x[ok]
        np.random.default_rng(1).shuffle(pool)
        _POOL.append(pool)
    return _POOL[0]


def operands(c, family, N, seed=0):
    """(A [M S, N], Bp [planes, N]) in fp32.
    aligned: every plane a constant of aligned_pool() - A row m holds x_m (in
        all its S planes), B plane p holds y_p, all distinct: every one of the
        six products, if missing, moves EVERY element by >= 2^-19 of it, and C
        counts elements (a column dropped, doubled or not zeroed: 1 / N);
    decades: standard normal draws, A row m scaled by 10^U(-12, 12), B plane p
        by 10^U(-3, 3): neighbouring output rows differ by orders of magnitude."""
    P = b_planes(c)
    if family == "aligned":
        pool = aligned_pool()
        assert len(pool) >= MAX_M + P, (len(pool), P)
        A = np.repeat(pool[:c.M], c.S)[:, None] * np.ones((1, N), np.float32)
        Bp = pool[MAX_M:MAX_M + P, None] * np.ones((1, N), np.float32)
    elif family == "decades":
        rng = np.random.default_rng(1000 + seed)
        A = rng.standard_normal((c.M, c.S, N)) * 10.0 ** rng.uniform(-12, 12, (c.M, 1, 1))
        A = A.reshape(c.M * c.S, N)
        Bp = rng.standard_normal((P, N)) * 10.0 ** rng.uniform(-3, 3, (P, 1))
    else:
        raise ValueError(family)
    return (np.ascontiguousarray(A, np.float32), np.ascontiguousarray(Bp, np.float32))


def flatten(c, A, Bp):
    """The product as a plain one: (A' [M, S N], B' [J, S N]) in fp32, segment s
    of row m / column j side by side."""
    N = A.shape[1]
    Af = A.reshape(c.M, c.S * N)
    Bf = np.concatenate([Bp[[bplane(c, j, s) for j in range(c.J)]] for s in range(c.S)], 1)
    return Af, Bf


def reference(c, A, Bp):
    """(ref64, sab) [M, J + ones]: the product in float64 and |A| @ |B|^T, the
    ones column as a B row of ones."""
    Af, Bf = (x.astype(np.float64) for x in flatten(c, A, Bp))
    if c.ones:
        Bf = np.concatenate((Bf, np.ones((1, Bf.shape[1]))))
    return Af @ Bf.T, np.abs(Af) @ np.abs(Bf).T


# (A term, B term) of the six matrix instructions, in the kernel's order
# (kTa / kTb of stream_body): l h, h l, m m, m h, h m, h h
PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


def emulate(c, A, Bp, drop=None):
    """The stream kernel's arithmetic with exact sums: the six products of the
    bf16 terms in float64 (`drop`: without product k), row sums from the fp32
    values."""
    Af, Bf = flatten(c, A, Bp)
    ta = [t.astype(np.float64) for t in split3(Af)]
    tb = [t.astype(np.float64) for t in split3(Bf)]
    C = sum(ta[i] @ tb[j].T for k, (i, j) in enumerate(PRODUCTS) if k != drop)
    if c.ones:
        C = np.concatenate((C, Af.astype(np.float64).sum(1, keepdims=True)), 1)
    return C


def elementwise_err(C, ref64, sab):
    """|C - ref64| / sab for every element."""
    return np.abs(np.asarray(C, np.float64) - ref64) / sab


# ------------------------------------------------------------ the bounds
U = 2.0 ** -24           # one fp32 rounding to nearest, relative
ALIGNED_BOUND = 2.0 ** -20
DROP_ONE_MIN = 2.0 ** -19


def stream_chunks_per_wave(N, S, wgs):
    return -(-(S * -(-N // 32)) // (4 * wgs))


def stream_roundings(N, S, wgs):
    """R of the stream kernel: an accumulator passes through six matrix
    instructions per chunk of 32 columns its wave multiplies, three additions
    of the four-wave sum and the final cast (the partials of the workgroups are
    added in double).  A row sum passes through 3 + 1 per chunk + 2 + 3 + 1."""
    return 6 * stream_chunks_per_wave(N, S, wgs) + 4


def tile_tiles_per_wg(N, S, wgs):
    """Most tiles of 64 columns one workgroup of the LDS-tile kernel multiplies
    (gemm_body: segmented products give XCD x the column tiles 8 c + x when the
    grid is a multiple of 8)."""
    X = 8 if (S > 1 and wgs % 8 == 0) else 1
    tps = -(-N // 64)
    return -(-(S * -(-tps // X)) // (wgs // X))


def tile_roundings(N, S, wgs):
    """R of the LDS-tile kernel: v_mfma_f32_32x32x2_f32 is an fp32 fma chain, one
    rounding per product; a wave owns 16 columns of every tile (fewer when N is
    smaller: a zero product rounds nothing), then the four-wave sum and the
    cast."""
    return min(16, N) * tile_tiles_per_wg(N, S, wgs) + 4


def decades_bound(R):
    """2^-22 = 4 u for the terms the six products leave out (the file's own
    worst case) plus R roundings, each <= u of a running sum <= sum |a||b|."""
    return (4 + R) * U


def tile_aligned_roundings(N, S, wgs):
    """The LDS-tile kernel on ALIGNED operands, one tile (N <= 64) per
    workgroup: every product of an element's tile is the same positive number
    p, so the running sum a rounding acts on is known, not just bounded.  Wave
    w multiplies n_w = min(16, N - 16 w) columns: its fma chain rounds sums of
    p, 2 p, ..., n_w p - together u p n_w (n_w + 1) / 2 where `tile_roundings`
    allows u p N for each of them; the three additions of the four-wave sum and
    the cast are taken at the whole tile as before.  In units of u times the
    tile's sum N p (the tiles of an element are added in double, so this is also
    the element's error over its sum |a||b|); a row sum's chains are shorter."""
    assert N <= 64 and tile_tiles_per_wg(N, S, wgs) == 1
    n = [max(0, min(16, N - 16 * w)) for w in range(4)]
    return sum(k * (k + 1) / 2 for k in n) / N + 4


def roundings(c, N, wgs, family="decades"):
    k = kind_of(c)[0]
    if k == "tile":
        return (tile_aligned_roundings if family == "aligned" else tile_roundings)(N, c.S, wgs)
    return stream_roundings(N, c.S, wgs)


# ------------------------------------------------------------ on the device
def problem(F, dev, c, A, Bp, pad=(1, 2, 3)):
    """A planes_gemm / planes_gemm_multi problem of case `c` with a NaN-filled,
    strided `out` view (pad: rows below, columns left, columns right) and a
    NaN-filled bias_out: dict(kw, full, bias) - kw for the call."""
    import torch
    Jc = c.J if c.bias else c.J + int(c.ones)
    full = torch.full((c.M + pad[0], pad[1] + Jc + pad[2]), float("nan"), device=dev)
    bias = torch.full((c.M,), float("nan"), device=dev) if c.bias else None
    kw = dict(A=torch.from_numpy(A).to(dev), M=c.M, S=c.S, Bp=torch.from_numpy(Bp).to(dev),
              bdesc=F.make_bdesc(dev, c.offs, list(c.s1), list(c.s2)), with_ones=c.ones,
              sdiv=c.sdiv, out=full[:c.M, pad[1]:pad[1] + Jc], bias_out=bias)
    return dict(kw=kw, full=full, bias=bias, pad=pad, Jc=Jc)


def result(c, p):
    """[M, J + ones] float64 of a finished problem; everything of `full` around
    the view must still be NaN."""
    full = p["full"].cpu().numpy().astype(np.float64)
    lo, hi = p["pad"][1], p["pad"][1] + p["Jc"]
    C = full[:c.M, lo:hi]
    rest = np.ones(full.shape, bool)
    rest[:c.M, lo:hi] = False
    assert np.isnan(full[rest]).all(), (c.name, "wrote outside its view")
    if c.bias:
        C = np.concatenate((C, p["bias"].cpu().numpy().astype(np.float64)[:, None]), 1)
    return C


def run_case(F, dev, c, family, N, wgs=None, seed=0):
    """One functional.planes_gemm call with `wgs` workgroups (None: the
    library's choice): (elementwise_err [M, J + ones], result).  A NaN left in
    the output is an infinite error."""
    A, Bp = operands(c, family, N, seed)
    p = problem(F, dev, c, A, Bp)
    before = F._GEMM_WGS
    F._GEMM_WGS = wgs
    try:
        F.planes_gemm(**p["kw"])
    finally:
        F._GEMM_WGS = before
    C = result(c, p)
    err = elementwise_err(C, *reference(c, A, Bp))
    return np.where(np.isfinite(err), err, math.inf), C


# (N, workgroups) of the all-cases test per (family, kind); None: the library's
# default, one workgroup per CU or more.  Aligned cases keep every wave to one
# chunk of 32 columns (stream: 4 chunks for the 4 waves of ONE workgroup, the
# last one ragged; segmented: S x 4 chunks over the default grid), so that
# R = 10 and the fixed 2^-20 holds by counting: 0.21 2^-22 measured for the six
# exact products + R / 4 = 2.7 in units of 2^-22, under 4 and under the 8 of a
# missing product.  The aligned LDS-tile cases fill one whole tile per segment
# and workgroup (N = 64: all four waves multiply, C counts the elements of each)
# - 12.5 roundings by tile_aligned_roundings, and no product is left out there.
PLAN = {("aligned", "stream"): (100, 1), ("aligned", "segmented"): (100, None),
        ("aligned", "tile"): (64, None),
        ("decades", "stream"): (100, None), ("decades", "segmented"): (100, None),
        ("decades", "tile"): (200, None)}
ALIGNED_MAX_R = 15      # + 0.85 u of the six products < 16 u = 2^-20


def default_wgs(lib, c):
    return lib.apg_planes_gemm_default_wgs(c.M, c.S, c.J, int(c.ones))


def bound_of(c, family, N, wgs):
    """(bound, R) of a case run with `wgs` workgroups (a number)."""
    R = roundings(c, N, wgs, family)
    if family == "aligned":
        assert R <= ALIGNED_MAX_R, (c.name, N, wgs, R)
        return ALIGNED_BOUND, R
    return decades_bound(R), R
