"""The cases of packed_extremes.py through the CPU route of the packed ops (out_dtype=torch.float32),
with and without tiled=True (one route on the CPU: equal bits): the builders and their float64
expectations are shown to be right here, on a machine without a GPU, before
test_gpu_swiglu_extremes.py and test_gpu_tiled_extremes.py hold the gfx950 kernels to them. The
expectation never uses the ops: numpy ref_unpack per chunk, float64 matmul.

What the GPU tests rest on is asserted on the reference alone: the shares of bf16-subnormal
operands and f32-subnormal products and sums, that a datapath which flushes subnormals computes
something else, that every far case has its boundary where its name says and that a parameter
taken 32 elements late differs in every column, and that the overflow cases have non-finite and
kept columns."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import _core

import packed_extremes as pe
import test_gpu_linear_extremes as gl4
import test_gpu_mxfp6_linear_extremes as gl6
from linear_extremes import SHAPES
from packed_extremes import FAR_K, FORMATS, GLU_FORMATS, P2_31, P2_32, PF, le
from test_gpu_mxfp4_swiglu import check_exact_regimes, regimes

F32 = dict(out_dtype=torch.float32)
IDS = [f.id for f in FORMATS]
HOST_CAP = 6 * 10 ** 9  # bytes a far case may commit on the host


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_values(a, b):
    """Equal NaN masks and equal values elsewhere (the CPU route's NaN payloads may depend on M)."""
    a, b = a.numpy(), b.numpy()
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan])


def _covered(wins, r):
    return any(r0 <= r < r1 for r0, r1 in wins)


def _linear(c, **kw):
    """The CPU route, which tiled=True does not change."""
    y = pe.run_linear(c, "cpu", **F32, **kw)
    assert _same(y, pe.run_linear(c, "cpu", tiled=True, **F32, **kw))
    return y


def _glu(c, **kw):
    y = pe.run_swiglu(c, "cpu", **F32, **kw)
    assert _same(y, pe.run_swiglu(c, "cpu", tiled=True, **F32, **kw))
    return y


def _tile_shapes(f):
    """The three shapes of test_gpu_tiled_extremes.py."""
    bm, bn = f.tile()
    return [(5, 48, 96), (bm + 1, 48, 160), (2 * bm + 5, bn + 16, 1056)]


def test_tiles_come_from_the_bindings():
    for f in FORMATS:
        bm, bn = f.tile()
        assert bm % 16 == 0 and bn % 16 == 0 and (bm, bn) == tuple(getattr(_core, f.name + "_tiled_tile")())


# ---------------------------------------------------------------- 1. the bottom of the range

LOW = [(f, s) for f in FORMATS for s in (100, 0)] + [(FORMATS[0], -8)]


@pytest.mark.parametrize("f,s", LOW, ids=[f"{f.id} s={s}" for f, s in LOW])
def test_subnormal_weights_at_the_tile_shapes(f, s):
    """The floors of test_linear_extremes_host.py / test_mxfp6_linear_extremes_host.py at the shapes
    the tiled suite uses, and the flushed expectation."""
    for m, n, k in _tile_shapes(f):
        c = pe.subnormal_weights(f, m, n, k, s)
        le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
        assert (np.abs(c.wf) < 2.0 ** -126).mean() > 0.2
        if s <= 0:
            prod, run, out = pe.subnormal_shares(c)
            print(f.id, s, (m, n, k), "f32-subnormal products %.4f, running sums %.4f, outputs %.4f" % (prod, run, out))
            assert np.abs(c.want).max() < 2.0 ** -100 and (c.want != 0).mean() > 0.9
            if f.name == "fp8" or (f.name, s) == ("mxfp4", -8):
                assert prod > 0.5 and run > 0.05 and out > 0.03
            else:  # MXFP4 and MXFP6 weights reach 6 and 7.5 * 2^-124: some products only at s = 0
                assert prod > 0.01
        flushed = pe.flushed_expectation(c.xf, c.wf)
        assert (flushed != c.want[:4]).mean() > 0.5  # a flush of operands or products is seen in most elements
        le.assert_f32_equal(_linear(c), c.want)


@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_subnormal_activations_at_the_tile_shapes(f):
    for m, n, k in _tile_shapes(f):
        c = pe.subnormal_activations(f, m, n, k)
        le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
        assert (np.abs(c.xf) < 2.0 ** -126).all() and (c.xf != 0).all()
        assert (np.abs(c.want[c.want != 0]) >= 2.0 ** -36).all()  # normal sums
        assert not pe.flushed_expectation(c.xf, c.wf).any() and (c.want != 0).mean() > 0.9  # flushed: all zero
        le.assert_f32_equal(_linear(c), c.want)


@pytest.mark.parametrize("which", ["gate", "up"])
@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_swiglu_subnormal_weights(f, which):
    """The floors of test_linear_extremes_host.test_swiglu_subnormal_weights, for every format at
    the shapes of both GPU suites: the low weights are bf16 subnormals (or next to them), the low
    product is a normal f32 far from the other one, and flushing the low weights changes y."""
    for m, n, k in SHAPES + _tile_shapes(f)[1:]:
        c = pe.swiglu_subnormal(f, which, m, n, k)
        pe.prove_swiglu(c)
        low, other, wlow = (c.g, c.u, c.wg) if which == "gate" else (c.u, c.g, c.wu)
        assert (np.abs(wlow) <= 7.5 * 2.0 ** -124).all() and (np.abs(wlow) < 2.0 ** -126).mean() > 0.2
        nz = np.abs(low[low != 0])
        assert nz.min() >= 2.0 ** -30 and nz.max() <= 2.0 ** 20 and (low != 0).mean() > 0.9
        assert np.abs(other).max() < 2.0 ** 125  # finite in f32, and so is silu(g) * u
        flushed = pe.flushed_expectation(c.xf, wlow)  # with the bf16-subnormal weights flushed, most of g (or u) changes
        assert (flushed != low[:4]).mean() > 0.5 and (f.name != "fp8" or not flushed.any())
        y = _glu(c)
        assert (y != 0).float().mean() > (0.9 if which == "gate" else 0.4)  # up low: y = 0 for g <= -104
        check_exact_regimes(y, c.g, c.u)


# ---------------------------------------------------------------- 2. the top of the range

@pytest.mark.parametrize("which", ["gate", "up"])
@pytest.mark.parametrize("f", GLU_FORMATS, ids=IDS[1:])
def test_swiglu_overflow_to_inf(f, which):
    for m, n, k in SHAPES + _tile_shapes(f)[1:]:
        for zeros in ((False, True) if f.name == "mxfp6" else (False,)):
            c = pe.swiglu_overflow(f, which, m, n, k, zeros=zeros)
            rows, keep = c.extra["rows"], c.extra["keep"]
            rest = np.setdiff1d(np.arange(n), rows)
            pe.prove_swiglu(c, keep)
            pe.prove_warm(c)
            want = c.extra["want"]
            assert len(rows) >= 3 and len(keep) >= n - 6 and not np.isfinite(want).any()
            assert np.isnan(want).any() and (zeros or np.isinf(want).any())  # both classes, unless 0 * inf takes all
            y = _glu(c)
            le.assert_f32_equal(y[:, rows], le.expected_f32(want).astype(np.float64))
            pe.check_regimes_to_inf(y[:, rest], c.g[:, rest], c.u[:, rest])
            le.assert_rows_bit_equal(y.t(), _glu(c, img=c.extra["clean_img"]).t(), keep)


def test_silu_mul_f32_differs_from_float64_only_where_expf_overflows():
    g = np.array([-800.0, -104.0, -88.75, -88.6875, -1.0, 0.0, 3.0, np.inf, -np.inf, np.nan])
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = pe.silu_mul_f32(g, np.full(g.shape, np.inf)), le.silu_mul64(g, np.full(g.shape, np.inf))
        e32 = np.exp(np.float32(88.75)), np.exp(np.float32(88.6875))
    assert np.isinf(e32[0]) and np.isfinite(e32[1])  # where f32's exp overflows
    assert np.isnan(a[[0, 1, 2, 5, 8, 9]]).all() and (a[[3, 4]] == -np.inf).all() and (a[[6, 7]] == np.inf).all()
    diff = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert diff.tolist() == [False, True, True] + [False] * 7


@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_nonfinite_activations_in_row_bm(f):
    """The bad row at row BM, linear and gated; the row alone gives the same bits."""
    bm = f.tile()[0]
    n, k = 48, 160
    c = pe.nonfinite_activations(f, n, k, bm + 1, row=bm)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    clean = _linear(c)
    le.assert_f32_equal(clean, c.want)
    for xb, _, want in c.extra["bad"].values():
        y = _linear(c, x=xb)
        le.assert_f32_equal(y, want)
        le.assert_rows_bit_equal(y, clean, c.extra["keep"])
        assert _same_values(_linear(c, x=xb[bm:]), y[bm:])
    c = pe.swiglu_nonfinite(f, n, k, bm + 1, row=bm)
    pe.prove_swiglu(c)
    clean = _glu(c)
    check_exact_regimes(clean, c.g, c.u)
    for xb, g, u in c.extra["bad"].values():
        want = le.silu_mul64(g[bm], u[bm])
        assert not np.isfinite(want).any()
        y = _glu(c, x=xb)
        le.assert_f32_equal(y[bm], le.expected_f32(want).astype(np.float64))
        le.assert_rows_bit_equal(y, clean, c.extra["keep"])
        assert _same_values(_glu(c, x=xb[bm:]), y[bm:])


@pytest.mark.parametrize("m,n,k", [(5, 48, 96), (17, 48, 160), (65, 528, 1056)])
@pytest.mark.parametrize("f", GLU_FORMATS, ids=IDS[1:])
def test_swiglu_nonfinite_activations(f, m, n, k):
    c = pe.swiglu_nonfinite(f, n, k, m)
    pe.prove_swiglu(c)
    clean = _glu(c)
    check_exact_regimes(clean, c.g, c.u)
    if (m, n, k) == (65, 528, 1056):  # every regime is present, as test_gpu_*_swiglu.py asserts at 64 x 528 x 1056
        assert min(r.mean() for r in regimes(c.g)) >= 0.01
    r = c.extra["row"]
    for xb, g, u in c.extra["bad"].values():
        y = _glu(c, x=xb)
        want = le.silu_mul64(g[r], u[r])
        assert not np.isfinite(want).any()
        le.assert_f32_equal(y[r], le.expected_f32(want).astype(np.float64))
        le.assert_rows_bit_equal(y, clean, c.extra["keep"])


# ---------------------------------------------------------------- 3. far into a large layer

ALL_FAR_GLU = {**pe.FAR_GLU_MXFP4, **pe.FAR_GLU}


@pytest.mark.parametrize("name", list(ALL_FAR_GLU))
def test_far_pairs_lie_where_their_names_say(name):
    """On the reference alone (S is built, the large buffer is not): far_glu_case asserts the
    positions; here the boundary is spelled out again from the name, the wrapped offsets lie in the
    never-read part, and a parameter taken 32 elements late differs in every column."""
    f = ALL_FAR_GLU[name][0]
    for m in (17, f.tile()[0] + 1):
        c = pe.far_glu_case(name, m=m)
        up_elem = c.elem_offset - c.off_s + c.up_s
        end = c.elem_offset + c.n * FAR_K
        if "behind 2^32" in name:
            assert min(c.elem_offset, c.first_byte) > P2_32
        elif "element" in name:
            b = P2_32 if "2^32" in name else P2_31
            assert c.elem_offset < b < end <= up_elem
        else:
            b = P2_32 if "2^32" in name else P2_31
            assert c.first_byte < b < c.last_byte < pe.far_up_first_byte(c)
        assert c.need < 5 * pe.GB and pe.wrapped_inside(c)
        le.prove_exact(c.xf, c.wf, 1.0, f.uw, c.want)
        le.prove_exact(c.xf, c.wu, 1.0, f.uw, c.xf @ c.wu.T)
        assert (pe.late32(c) != c.want).any(0).all() and (pe.late32(c, up=True) != c.xf @ c.wu.T).any(0).all()


@pytest.mark.parametrize("fmt,spec", [(v[0], v) for v in gl4.FAR.values()] + [("mxfp6", ("mxfp6",) + v[:3])
                                                                              for v in gl6.FAR.values()])
def test_far_linear_tables_at_bm_plus_1_rows(fmt, spec):
    _, c0, boundary, packed = spec
    f = PF(fmt, 128 if fmt == "fp8" else 32)
    off_s = 32 * 700
    if c0 is None:
        c0, off_s = pe.crossing_c0(f, boundary, packed)
    c = pe.far_case(f, c0, off_s, m=f.tile()[0] + 1)
    pe.assert_far_position(c, boundary, packed)
    assert c.need < 5 * pe.GB and pe.wrapped_inside(c)
    assert (pe.late32(c) != c.want).any(0).all()


WIDE = [FORMATS[0], FORMATS[1], FORMATS[3], PF("fp8", 512)]


@pytest.mark.parametrize("f", WIDE, ids=[f.id for f in WIDE])
def test_far_pair_of_two_workgroups_through_the_cpu_route(f):
    """70 000 chunks of 64 KiB that are never touched, then a pair of BN + 16 rows each: element
    offsets beyond 2^31 (fp8: packed bytes too). At most 2.4 GB, allocated and not written."""
    bm, bn = f.tile()
    n, gate = bn + 16, 32 * 3
    up = gate + n * FAR_K + 64
    c = pe.far_case(f, 70_000, gate, m=5, n=n, up_s=up, chunks=-(-(up + n * FAR_K) // (pe.FAR_CHUNK // 2)))
    assert c.elem_offset > P2_31 and c.need < HOST_CAP
    u = c.xf @ c.wu.T
    le.prove_exact(c.xf, c.wf, 1.0, f.uw, c.want)
    le.prove_exact(c.xf, c.wu, 1.0, f.uw, u)
    assert (pe.late32(c) != c.want).any(0).all() and (pe.late32(c, up=True) != u).any(0).all()
    buf = c.place("cpu")
    y = pe.far_linear(c, buf, **F32)
    le.assert_f32_equal(y, c.want)
    assert _same(y, pe.far_linear(c, buf, tiled=True, **F32))
    g = pe.far_swiglu(c, buf, **F32)
    check_exact_regimes(g, c.want, u)
    assert _same(g, pe.far_swiglu(c, buf, tiled=True, **F32))
    assert np.array_equal(le.mx.bf16_tensor_bits(pe.far_unpack(c, buf, c.up_s)), c.up_bits)


# ---------------------------------------------------------------- 4. rows of x and of y beyond 32 bits

@pytest.mark.parametrize("f", [FORMATS[0], FORMATS[1], FORMATS[3]], ids=["mxfp4", "mxfp6", "fp8b128"])
def test_the_checked_windows_hold_the_crossings(f):
    """The windows of test_gpu_tiled_extremes.py's large-M cases, and the small case that fills
    them through the CPU route (the 8.6 GB x itself is a GPU matter: far beyond 6 GB of host memory)."""
    bm = f.tile()[0]
    m, wins = pe.big_x_rows(bm)
    k = pe.BIG_K
    assert m * k > P2_32 and 2 * m * k + 4 * m * pe.BIG_N < 10 * pe.GB
    assert all(r0 % bm == 0 and (r1 % bm == 0 or r1 == m) and r0 < r1 for r0, r1 in wins) and wins[0][0] == 0
    for b in (P2_31, P2_32):  # element b (and byte 2 b) of x lies in a checked tile with a checked tile on either side
        r = b // k
        assert _covered(wins, r - bm) and _covered(wins, r) and (_covered(wins, r + bm) or r + bm >= m), (b, wins)
    rows = sum(r1 - r0 for r0, r1 in wins)
    assert rows <= 12 * bm
    ld = 528
    my, wy = pe.big_y_rows(bm, ld)
    assert my * ld > P2_31 and 4 * my * ld > P2_32 and 4 * (3 * ld + 8 + (my + 3) * ld) + 2 * my * 32 < 10 * pe.GB
    for b in (1 << 30, P2_31):  # element b of y: byte 2^32 and element 2^31
        r = b // ld
        assert _covered(wy, r - bm) and _covered(wy, r) and _covered(wy, r + bm), (b, wy)
    c = pe.clean_case(f, rows, pe.BIG_N, k)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    le.assert_f32_equal(_linear(c), c.want)
    g = pe.swiglu_clean(f, sum(r1 - r0 for r0, r1 in wy), pe.BIG_N, 32)
    pe.prove_swiglu(g)
    check_exact_regimes(_glu(g), g.g, g.u)


# ---------------------------------------------------------------- 5. views of x

@pytest.mark.parametrize("f", GLU_FORMATS, ids=IDS[1:])
def test_views_of_x(f):
    k, n = 160, 48
    c = pe.swiglu_clean(f, 18, n, k)
    pe.prove_swiglu(c)
    base = _glu(c)
    check_exact_regimes(base, c.g, c.u)
    for name, v in le.x_views(c.x).items():
        y = _glu(c, x=v)
        assert tuple(y.shape) == tuple(v.shape[:-1]) + (n,), name
        assert _same(y.reshape(18, n), base), name
