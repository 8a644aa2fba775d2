"""The gfx950 packed linears (mxfp4_linear.hip, fp8_linear.hip, mxfp4_swiglu.hip) at their numeric
and addressing extremes: the cases of linear_extremes.py, which test_linear_extremes_host.py runs
through the CPU route, on the kernels. The expectation is the numpy ref_unpack per chunk and a
float64 matmul; every case carries a proof, asserted here on the reference alone, that an f32
accumulation in any order is exact, so outputs are compared for equality.

1. bf16-subnormal weights (B operand of v_mfma_f32_16x16x32_bf16), bf16-subnormal activations (A
   operand) and f32-subnormal products and sums (C/D): the MFMA must keep all three.
2. weights that unpack to +-inf, f32 sums that overflow, NaN and +-inf in x.
3. a parameter behind 2^31 / 2^32 elements and packed bytes of a layer that is never read.
4. three and four passes of 64 rows into a strided `out`; views of x.

Every case runs with split_k 0 (the launcher's choice) and a forced split, f32 and bf16 output."""
import numpy as np
import pytest
import torch

import linear_extremes as le
from linear_extremes import ROW_TILES_SHAPE, SHAPES
from test_gpu_mxfp4_swiglu import check_exact_regimes

pytestmark = pytest.mark.gpu

FMT_BLOCKS = [("mxfp4", 32), ("fp8", 32), ("fp8", 128)]
# s = 100: normal products; s = 0: f32-subnormal products and sums. MXFP4 weights reach 6 * 2^-124, so at
# s = 0 few of its sums are subnormal: s = -8 (products up to 1.5 * 2^-127) puts its accumulators there
LOW_CASES = [(f, b, s) for f, b in FMT_BLOCKS for s in (100, 0)] + [("mxfp4", 32, -8)]
SPLITS = (0, 2)
DEV = "cuda"


def _variants(m, n, k):
    """(split_k, row_tiles): split_k 0 and 2, and at N = 64 two row tiles per wave forced."""
    return [(s, 0) for s in SPLITS] + ([(0, 2), (2, 2)] if n == 64 else [])


def _check_linear(c, want=None, x=None, img=None):
    """f32 output == expectation and bf16 output == its rounding, for every variant; returns the
    (f32, bf16) outputs of all variants."""
    want = c.want if want is None else want
    outs = []
    p = torch.from_numpy(c.img if img is None else img).to(DEV)
    for split_k, row_tiles in _variants(c.m, c.n, c.k):
        kw = dict(x=x, img=p, split_k=split_k, row_tiles=row_tiles)
        y32 = le.run_linear(c, DEV, out_dtype=torch.float32, **kw)
        y16 = le.run_linear(c, DEV, **kw)
        le.assert_f32_equal(y32, want)
        le.assert_bf16_is_rounded(y16, want)
        outs.append((y32, y16))
    return outs


def _prove_swiglu(c):
    le.prove_exact(c.xf, c.wg, c.ux, c.ug, c.g)
    le.prove_exact(c.xf, c.wu, c.ux, c.uu, c.u)


def _check_swiglu(c, x=None):
    """check_exact_regimes on the f32 output of a finite x (the caller checks the output of another
    x), bf16 output == the f32 output rounded once; returns the (f32, bf16) outputs of all variants."""
    outs = []
    p = torch.from_numpy(c.img).to(DEV)
    for split_k, row_tiles in _variants(c.x.shape[0], c.n, c.k):
        kw = dict(x=x, img=p, split_k=split_k, row_tiles=row_tiles)
        y32 = le.run_swiglu(c, DEV, out_dtype=torch.float32, **kw)
        y16 = le.run_swiglu(c, DEV, **kw)
        if x is None:
            print("worst err / bound", check_exact_regimes(y32, c.g, c.u))
        assert np.array_equal(le.mx.bf16_tensor_bits(y16), le.f32_to_bf16_bits(y32.cpu().numpy()).reshape(-1))
        outs.append((y32, y16))
    return outs


# ---------------------------------------------------------------- 1. the bottom of the range

@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
@pytest.mark.parametrize("fmt,block,s", LOW_CASES)
def test_subnormal_weights(gpu, fmt, block, s, m, n, k):
    """bf16-subnormal B operands; with s <= 0 also f32-subnormal products and accumulators (the host
    twin asserts their shares on the reference)."""
    c = le.subnormal_weights(fmt, m, n, k, s, block)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    _check_linear(c)


@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
@pytest.mark.parametrize("fmt,block", FMT_BLOCKS)
def test_subnormal_activations(gpu, fmt, block, m, n, k):
    """bf16-subnormal A operands against large weights."""
    c = le.subnormal_activations(fmt, m, n, k, block)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    _check_linear(c)


@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
@pytest.mark.parametrize("which", ["gate", "up"])
def test_swiglu_subnormal_weights(gpu, which, m, n, k):
    c = le.swiglu_subnormal(which, m, n, k)
    _prove_swiglu(c)
    _check_swiglu(c)


# ---------------------------------------------------------------- 2. the top of the range

@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
@pytest.mark.parametrize("zeros", [False, True])
def test_mxfp4_overflow_to_inf(gpu, zeros, m, n, k):
    """Scale bytes 253 and 254: +-inf weights give +-inf, NaN where they meet or meet a 0 of x;
    every other column keeps the bits of the run on the clean image."""
    c = le.mxfp4_overflow(m, n, k, zeros)
    cl = c.extra["clean"]
    le.prove_exact(cl.xf, cl.wf, cl.ux, cl.uw, cl.want)
    for (y32, y16), (c32, c16) in zip(_check_linear(c), _check_linear(cl)):  # variant by variant
        le.assert_rows_bit_equal(y32.t(), c32.t(), c.extra["keep"])
        le.assert_rows_bit_equal(y16.t(), c16.t(), c.extra["keep"])


@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
@pytest.mark.parametrize("block", [32, 128])
def test_fp8_sums_overflow_f32(gpu, block, m, n, k):
    """E = 120: finite weights up to 240 * 2^120 whose one-signed sums pass 2^129 give +-inf, every
    other sum stays below 2^127 and exact."""
    c = le.fp8_overflow(m, n, k, block)
    keep = c.extra["keep"]
    le.prove_exact(c.xf, c.wf[keep], c.ux, c.uw, c.want[:, keep])
    le.prove_exact(c.xf, c.wf[c.extra["warm"]], 1.0, 2.0 ** 117, c.want[:, c.extra["warm"]])  # finite at E = 120
    _check_linear(c)


NONFINITE = [(5, 48, 96), (17, 48, 160), (65, 528, 1056), (17, 64, 160)]


@pytest.mark.parametrize("m,n,k", NONFINITE)
@pytest.mark.parametrize("fmt", ["mxfp4", "fp8"])
def test_nonfinite_activations(gpu, fmt, m, n, k):
    """NaN, +inf and -inf in one row of x (row 3 of 5, 16 of 17, 64 of 65: the second pass): that
    row of y is non-finite as the float64 expectation says, every other row keeps its bits."""
    c = le.nonfinite_activations(fmt, n, k, m)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    clean = _check_linear(c)
    for xb, _, want in c.extra["bad"].values():
        for (y32, y16), (c32, c16) in zip(_check_linear(c, want=want, x=xb), clean):  # variant by variant
            le.assert_rows_bit_equal(y32, c32, c.extra["keep"])
            le.assert_rows_bit_equal(y16, c16, c.extra["keep"])


@pytest.mark.parametrize("m,n,k", NONFINITE)
def test_swiglu_nonfinite_activations(gpu, m, n, k):
    """The same through mxfp4_swiglu. Every variant (split_k 0 and 2, whose sums of g and u pass
    through the kernel's LDS reduction, and row_tiles=2 at N = 64) is held to the expectation of
    the bad row and to the bits of its own clean run in every other row."""
    c = le.swiglu_nonfinite(n, k, m)
    _prove_swiglu(c)
    clean = _check_swiglu(c)
    r = c.extra["row"]
    for xb, g, u in c.extra["bad"].values():
        want = le.silu_mul64(g[r], u[r])
        assert not np.isfinite(want).any()
        outs = _check_swiglu(c, x=xb)
        assert len(outs) == len(clean) >= 2
        for (y32, y16), (c32, c16) in zip(outs, clean):
            le.assert_f32_equal(y32[r], le.expected_f32(want).astype(np.float64))
            le.assert_rows_bit_equal(y32, c32, c.extra["keep"])
            le.assert_rows_bit_equal(y16, c16, c.extra["keep"])


# ---------------------------------------------------------------- 3. far into a large layer

GB = 10 ** 9
P2_31, P2_32 = 1 << 31, 1 << 32


def _far_buffer(c):
    assert c.need < 5 * GB
    torch.cuda.empty_cache()
    return c.place(DEV)


def _check_far_linear(c, buf):
    for split_k, row_tiles in _variants(c.x.shape[0], c.n, le.FAR_K):
        kw = dict(split_k=split_k, row_tiles=row_tiles)
        le.assert_f32_equal(le.far_linear(c, buf, out_dtype=torch.float32, **kw), c.want)
        le.assert_bf16_is_rounded(le.far_linear(c, buf, **kw), c.want)
    assert np.array_equal(le.mx.bf16_tensor_bits(le.far_unpack(c, buf)), c.bits)


FAR = {
    "mxfp4 behind 2^32 elements and bytes": ("mxfp4", 250_000, None, None),
    "mxfp4 element 2^32 inside": ("mxfp4", None, P2_32, False),
    "mxfp4 packed byte 2^32 inside": ("mxfp4", None, P2_32, True),
    "fp8 behind 2^32 elements and bytes": ("fp8", 140_000, None, None),
    "fp8 element 2^31 inside": ("fp8", None, P2_31, False),
    "fp8 packed byte 2^31 inside": ("fp8", None, P2_31, True),
    "mxfp4 element 2^32 inside, 64 rows, 2 row tiles per wave": ("mxfp4", None, P2_32, False),
    "fp8 packed byte 2^31 inside, 64 rows, 2 row tiles per wave": ("fp8", None, P2_31, True),
}


@pytest.mark.parametrize("name", list(FAR))
def test_far_into_a_large_layer(gpu, name):
    """S behind c0 chunks of 64 KiB that are allocated and never written or read: the kernels'
    chunk index, packed byte offset and block / element index beyond 32 bits. Peak 4.73 GB."""
    fmt, c0, boundary, packed = FAR[name]
    off_s = 32 * 700
    if c0 is None:
        c0, off_s = le.crossing_c0(fmt, 128, boundary, packed)
    c = le.far_case(fmt, c0, off_s, m=17, n=64 if "64 rows" in name else le.FAR_N)
    if boundary is None:
        assert c.elem_offset > P2_32 and c.first_byte > P2_32
    elif packed:
        assert c.first_byte < boundary < c.last_byte
    else:
        assert c.elem_offset < boundary < c.elem_offset + c.n * le.FAR_K
    if name == "mxfp4 element 2^32 inside":
        assert c0 == 131_071
    if name == "mxfp4 packed byte 2^32 inside":
        assert c0 == 246_723
    buf = _far_buffer(c)
    try:
        _check_far_linear(c, buf)
    finally:
        del buf
        torch.cuda.empty_cache()


@pytest.mark.parametrize("c0,gate,up", [(250_000, 32 * 3, 32 * 3 + 48 * 1056 + 64), (131_071, 32 * 10, 32 * 1030)])
def test_far_swiglu(gpu, c0, gate, up):
    """Both parameters beyond 2^32 elements and bytes; then the gate starting before element 2^32
    (which lies inside it) and the up behind it."""
    c = le.far_case("mxfp4", c0, gate, m=17, up_s=up)
    up_elem = c.elem_offset - gate + up
    if c0 == 250_000:
        assert c.elem_offset > P2_32 and c.first_byte > P2_32
    else:
        assert c.elem_offset < P2_32 < c.elem_offset + le.FAR_N * le.FAR_K and up_elem > P2_32
    buf = _far_buffer(c)
    try:
        g, u = c.want, c.xf @ c.wu.T
        for split_k in SPLITS:
            check_exact_regimes(le.far_swiglu(c, buf, out_dtype=torch.float32, split_k=split_k), g, u)
        assert np.array_equal(le.mx.bf16_tensor_bits(le.far_unpack(c, buf, up)), c.up_bits)
    finally:
        del buf
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 4. passes, strided output, views of x

@pytest.mark.parametrize("n,k,ld", [(48, 160, 80), (528, 1056, 560), (64, 160, 80)])
@pytest.mark.parametrize("m", [129, 200])
@pytest.mark.parametrize("fmt", ["mxfp4", "fp8", "swiglu"])
def test_several_passes_into_a_strided_out(gpu, fmt, m, n, k, ld):
    """M = 129 and 200: three and four passes of 64 rows, the last one partial. `out` is a view
    with a row stride beyond N inside a 0xA5-filled buffer: the values are exact and every byte
    outside y[:M, :N] is unchanged."""
    if fmt == "swiglu":
        c = le.swiglu_clean(m, n, k)
        _prove_swiglu(c)
    else:
        c = le.clean_case(fmt, m, n, k)
        le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    p = torch.from_numpy(c.img).to(DEV)
    op = le.run_swiglu if fmt == "swiglu" else le.run_linear
    for split_k in (0, 4):
        kw = dict(img=p, split_k=split_k, row_tiles=2 if n == 64 else 0)  # N = 64: two row tiles per wave forced
        y32 = op(c, DEV, out_dtype=torch.float32, **kw)
        if fmt == "swiglu":
            check_exact_regimes(y32, c.g, c.u)
        else:
            le.assert_f32_equal(y32, c.want)
        for dtype in (torch.float32, torch.bfloat16):
            buf, y = le.strided_out(m, n, ld, dtype, DEV)
            got = op(c, DEV, out=y, **kw)
            assert got.data_ptr() == y.data_ptr() and y.stride(0) == ld
            if dtype == torch.float32:
                assert torch.equal(y.contiguous().view(torch.int32), y32.view(torch.int32))
            else:
                assert np.array_equal(le.mx.bf16_tensor_bits(y), le.f32_to_bf16_bits(y32.cpu().numpy()).reshape(-1))
            le.assert_untouched_outside(buf, m, n, ld, dtype)


@pytest.mark.parametrize("fmt", ["mxfp4", "fp8", "swiglu"])
def test_views_of_x(gpu, fmt):
    """x as [2, 9, k], as sliced and transposed non-contiguous views and as a contiguous view 2
    bytes off a 16-byte boundary: the bits of the contiguous, aligned x; leading dimensions kept."""
    k, n = 160, 48
    if fmt == "swiglu":
        c = le.swiglu_clean(18, n, k)
        run = lambda x, **kw: le.run_swiglu(c, DEV, x=x, img=p, **kw)
    else:
        c = le.clean_case(fmt, 18, n, k)
        run = lambda x, **kw: le.run_linear(c, DEV, x=x, img=p, **kw)
    p = torch.from_numpy(c.img).to(DEV)
    xd = c.x.to(DEV)
    for split_k in SPLITS:
        base = run(xd, out_dtype=torch.float32, split_k=split_k)
        base16 = run(xd, split_k=split_k)
        if fmt == "swiglu":
            check_exact_regimes(base, c.g, c.u)
        else:
            le.assert_f32_equal(base, c.want)
        for name, v in le.x_views(xd).items():
            y = run(v, out_dtype=torch.float32, split_k=split_k)
            assert tuple(y.shape) == tuple(v.shape[:-1]) + (n,), name
            assert torch.equal(y.reshape(18, n).view(torch.int32), base.view(torch.int32)), name
            y16 = run(v, split_k=split_k)
            assert torch.equal(y16.reshape(18, n).view(torch.int16), base16.view(torch.int16)), name
