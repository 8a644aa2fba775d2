"""The gfx950 MXFP6 linear (mxfp6_linear.hip) at its numeric and addressing extremes: the cases of
mxfp6_linear_extremes.py, which test_mxfp6_linear_extremes_host.py runs through the CPU route, on
the kernel. The expectation is the numpy ref_unpack per chunk and a float64 matmul; every case
carries a proof, asserted here on the reference alone, that an f32 accumulation in any order is
exact, so outputs are compared for equality.

1. bf16-subnormal weights out of v_cvt_scalef32_pk32_bf16_fp6 (scale bytes 0..3, B operand of
   v_mfma_f32_16x16x32_bf16), bf16-subnormal activations (A operand), f32-subnormal products and
   sums (C/D).
2. scale bytes 253 and 254, whose weights convert to +-inf; NaN and +-inf in x.
3. a parameter across element 2^31 and across byte 2^32 of the packed image of a layer that is
   otherwise never read.
4. three and four passes of 64 rows into a strided `out`; views of x.

Every case runs with split_k 0 (the launcher's choice) and a forced split, f32 and bf16 output."""
import numpy as np
import pytest
import torch

import mxfp6_linear_extremes as e6
from mxfp6_linear_extremes import ROW_TILES_SHAPE, SHAPES

pytestmark = pytest.mark.gpu

SPLITS = (0, 2)
DEV = "cuda"


def _variants(n):
    """(split_k, row_tiles): split_k 0 and 2, and at N = 64 two row tiles per wave forced."""
    return [(s, 0) for s in SPLITS] + ([(0, 2), (2, 2)] if n == 64 else [])


def _check_linear(c, want=None, x=None):
    """f32 output == expectation and bf16 output == its rounding, for every variant; returns the
    (f32, bf16) outputs of all variants."""
    want = c.want if want is None else want
    outs = []
    p = torch.from_numpy(c.img).to(DEV)
    for split_k, row_tiles in _variants(c.n):
        kw = dict(x=x, img=p, split_k=split_k, row_tiles=row_tiles)
        y32 = e6.run_linear(c, DEV, out_dtype=torch.float32, **kw)
        y16 = e6.run_linear(c, DEV, **kw)
        e6.assert_f32_equal(y32, want)
        e6.assert_bf16_is_rounded(y16, want)
        outs.append((y32, y16))
    return outs


# ---------------------------------------------------------------- 1. the bottom of the range

@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
@pytest.mark.parametrize("s", [100, 0, -8])
def test_subnormal_weights(gpu, s, m, n, k):
    """bf16-subnormal B operands; with s <= 0 also f32-subnormal products and accumulators (the host
    twin asserts their shares on the reference)."""
    c = e6.subnormal_weights(m, n, k, s)
    e6.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    _check_linear(c)


@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
def test_subnormal_activations(gpu, m, n, k):
    """bf16-subnormal A operands against scale byte 227."""
    c = e6.subnormal_activations(m, n, k)
    e6.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    _check_linear(c)


# ---------------------------------------------------------------- 2. the top of the range

@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
@pytest.mark.parametrize("zeros", [False, True])
def test_overflow_to_inf(gpu, zeros, m, n, k):
    """Scale bytes 253 and 254: +-inf weights give +-inf, NaN where they meet or meet a 0 of x;
    every other column keeps the bits of the run on the clean image."""
    c = e6.overflow(m, n, k, zeros)
    cl = c.extra["clean"]
    e6.prove_exact(cl.xf, cl.wf, cl.ux, cl.uw, cl.want)
    for (y32, y16), (c32, c16) in zip(_check_linear(c), _check_linear(cl)):  # variant by variant
        e6.assert_rows_bit_equal(y32.t(), c32.t(), c.extra["keep"])
        e6.assert_rows_bit_equal(y16.t(), c16.t(), c.extra["keep"])


@pytest.mark.parametrize("m,n,k", [(5, 48, 96), (17, 48, 160), (65, 528, 1056), (17, 64, 160)])
def test_nonfinite_activations(gpu, m, n, k):
    """NaN, +inf and -inf in one row of x (row 3 of 5, 16 of 17, 64 of 65: the second pass): that
    row of y is non-finite as the float64 expectation says, every other row keeps its bits."""
    c = e6.nonfinite_activations(n, k, m)
    e6.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    clean = _check_linear(c)
    for xb, _, want in c.extra["bad"].values():
        for (y32, y16), (c32, c16) in zip(_check_linear(c, want=want, x=xb), clean):  # variant by variant
            e6.assert_rows_bit_equal(y32, c32, c.extra["keep"])
            e6.assert_rows_bit_equal(y16, c16, c.extra["keep"])


# ---------------------------------------------------------------- 3. far into a large layer

P2_31, P2_32 = 1 << 31, 1 << 32

FAR = {
    "behind 2^32 elements and bytes": (180_000, None, None, 48),
    "element 2^31 inside": (None, P2_31, False, 48),
    "packed byte 2^32 inside": (None, P2_32, True, 48),
    "packed byte 2^32 inside, 64 rows, 2 row tiles per wave": (None, P2_32, True, 64),
}


@pytest.mark.parametrize("name", list(FAR))
def test_far_into_a_large_layer(gpu, name):
    """S behind c0 chunks of 64 KiB that are allocated and never written or read: the kernel's
    chunk index, packed byte offset and block index beyond 32 bits. Peak 4.7 GB."""
    c0, boundary, packed, n = FAR[name]
    off_s = 32 * 700
    if c0 is None:
        c0, off_s = e6.crossing_c0(boundary, packed)
    c = e6.far_case(c0, off_s, m=17, n=n)
    e6.prove_exact(c.xf, c.wf, 1.0, 2.0 ** -4, c.want)
    if boundary is None:
        assert c.elem_offset > P2_32 and c.first_byte > P2_32
    elif packed:
        assert c.first_byte < boundary < c.last_byte
    else:
        assert c.elem_offset < boundary < c.elem_offset + c.n * e6.FAR_K
    assert c.need < 5 * 10 ** 9
    torch.cuda.empty_cache()
    buf = c.place(DEV)
    try:
        for split_k, row_tiles in _variants(c.n):
            kw = dict(split_k=split_k, row_tiles=row_tiles)
            e6.assert_f32_equal(e6.far_linear(c, buf, out_dtype=torch.float32, **kw), c.want)
            e6.assert_bf16_is_rounded(e6.far_linear(c, buf, **kw), c.want)
        assert np.array_equal(e6.m6.bf16_tensor_bits(e6.far_unpack(c, buf)), c.bits)
    finally:
        del buf
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 4. passes, strided output, views of x

@pytest.mark.parametrize("n,k,ld", [(48, 160, 80), (528, 1056, 560), (64, 160, 80)])
@pytest.mark.parametrize("m", [129, 200])
def test_several_passes_into_a_strided_out(gpu, m, n, k, ld):
    """M = 129 and 200: three and four passes of 64 rows, the last one partial. `out` is a view
    with a row stride beyond N inside a 0xA5-filled buffer: the values are exact and every byte
    outside y[:M, :N] is unchanged."""
    c = e6.clean_case(m, n, k)
    e6.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    p = torch.from_numpy(c.img).to(DEV)
    for split_k in (0, 4):
        kw = dict(img=p, split_k=split_k, row_tiles=2 if n == 64 else 0)  # N = 64: two row tiles per wave forced
        y32 = e6.run_linear(c, DEV, out_dtype=torch.float32, **kw)
        e6.assert_f32_equal(y32, c.want)
        for dtype in (torch.float32, torch.bfloat16):
            buf, y = e6.strided_out(m, n, ld, dtype, DEV)
            got = e6.run_linear(c, DEV, out=y, **kw)
            assert got.data_ptr() == y.data_ptr() and y.stride(0) == ld
            if dtype == torch.float32:
                assert torch.equal(y.contiguous().view(torch.int32), y32.view(torch.int32))
            else:
                assert np.array_equal(e6.m6.bf16_tensor_bits(y), e6.f32_to_bf16_bits(y32.cpu().numpy()).reshape(-1))
            e6.assert_untouched_outside(buf, m, n, ld, dtype)


def test_views_of_x(gpu):
    """x as [2, 9, k], as sliced and transposed non-contiguous views and as a contiguous view 2
    bytes off a 16-byte boundary: the bits of the contiguous, aligned x; leading dimensions kept."""
    k, n = 160, 48
    c = e6.clean_case(18, n, k)
    p = torch.from_numpy(c.img).to(DEV)
    xd = c.x.to(DEV)
    for split_k in SPLITS:
        base = e6.run_linear(c, DEV, x=xd, img=p, out_dtype=torch.float32, split_k=split_k)
        base16 = e6.run_linear(c, DEV, x=xd, img=p, split_k=split_k)
        e6.assert_f32_equal(base, c.want)
        for name, v in e6.x_views(xd).items():
            y = e6.run_linear(c, DEV, x=v, img=p, out_dtype=torch.float32, split_k=split_k)
            assert tuple(y.shape) == tuple(v.shape[:-1]) + (n,), name
            assert torch.equal(y.reshape(18, n).view(torch.int32), base.view(torch.int32)), name
            y16 = e6.run_linear(c, DEV, x=v, img=p, split_k=split_k)
            assert torch.equal(y16.reshape(18, n).view(torch.int16), base16.view(torch.int16)), name
