"""The gfx950 fused gated kernels of the fp8 and MXFP6 formats (fp8_swiglu.hip, mxfp6_swiglu.hip;
ops.fp8_swiglu with blocks 32 and 128, ops.mxfp6_swiglu) at their numeric and addressing extremes:
what test_gpu_linear_extremes.py asks of mxfp4_swiglu, on the cases of packed_extremes.py, which
test_packed_extremes_host.py runs through the CPU route. The expectation is the numpy ref_unpack per
chunk and two float64 matmuls; every case carries the proof, asserted here on the reference alone,
that g and u are exact in f32 in any summation order, so the f32 output is held to the three
regimes of the epilogue (check_exact_regimes of test_gpu_mxfp4_swiglu.py) and the bf16 output to
the f32 output rounded once.

1. bf16-subnormal gate weights against ordinary up weights and the reverse: one x fragment feeds
   both MFMAs, and either B operand must survive. It cannot see f32-subnormal sums: one x serves
   both products, and they lie 2^124 apart (the tiled suite and the linear suites have those).
2. gate or up rows that convert to +-inf (MXFP6 scale bytes 253 / 254) or whose f32 sums overflow
   (fp8, E = 120): those columns are +-inf or NaN as the reference says per element, every other
   column keeps the bits of the run on the clean image. NaN and +-inf in one row of x (in the second
   pass of 64 rows at M = 65): that row as silu_mul64 of the reference, every other row the bits of
   its clean run. It cannot tell which of several NaN payloads a kernel wrote.
3. a gate / up pair behind 2^32 elements and bytes of a layer that is never read, and a gate that
   crosses element 2^31, packed byte 2^31 (fp8) or packed byte 2^32 (MXFP6) with the up behind it:
   both offsets through the kernels' chunk, byte and block arithmetic. Peak 4.73 GB (fp8, 140 000
   chunks of 33 792 B). It sees a truncated index as a wrong value only: the wrapped address lies
   in the allocated low part of the buffer (asserted before the launch).
4. three and four passes of 64 rows into a strided `out`; views of x.

Every case runs with split_k 0 (the launcher's choice) and a forced split, and at N = 64 with two
row tiles per wave forced."""
import numpy as np
import pytest
import torch

import packed_extremes as pe
from linear_extremes import ROW_TILES_SHAPE, SHAPES
from packed_extremes import GLU_FORMATS, le
from test_gpu_mxfp4_swiglu import check_exact_regimes

pytestmark = pytest.mark.gpu

SPLITS = (0, 2)
DEV = "cuda"
NONFINITE = [(5, 48, 96), (17, 48, 160), (65, 528, 1056), (17, 64, 160)]
IDS = [f.id for f in GLU_FORMATS]


def _variants(n):
    """(split_k, row_tiles): split_k 0 and 2, and at N = 64 two row tiles per wave forced."""
    return [(s, 0) for s in SPLITS] + ([(0, 2), (2, 2)] if n == 64 else [])


def _run(c, x=None, img=None):
    """The (f32, bf16) outputs of every variant; the bf16 output is the f32 output rounded once."""
    outs = []
    p = torch.from_numpy(c.img if img is None else img).to(DEV)
    for split_k, row_tiles in _variants(c.n):
        kw = dict(x=x, img=p, split_k=split_k, row_tiles=row_tiles)
        y32 = pe.run_swiglu(c, DEV, out_dtype=torch.float32, **kw)
        y16 = pe.run_swiglu(c, DEV, **kw)
        assert np.array_equal(le.mx.bf16_tensor_bits(y16), le.f32_to_bf16_bits(y32.cpu().numpy()).reshape(-1))
        outs.append((y32, y16))
    return outs


def _check(c, cols=None, check=check_exact_regimes, **kw):
    outs = _run(c, **kw)
    cols = slice(None) if cols is None else cols
    for y32, _ in outs:
        print(c.f.id, "worst err / bound", check(y32[:, cols], c.g[:, cols], c.u[:, cols]))
    return outs


# ---------------------------------------------------------------- 1. the bottom of the range

@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
@pytest.mark.parametrize("which", ["gate", "up"])
@pytest.mark.parametrize("f", GLU_FORMATS, ids=IDS)
def test_subnormal_weights(gpu, f, which, m, n, k):
    c = pe.swiglu_subnormal(f, which, m, n, k)
    pe.prove_swiglu(c)
    _check(c)


# ---------------------------------------------------------------- 2. the top of the range

@pytest.mark.parametrize("m,n,k", SHAPES + [ROW_TILES_SHAPE])
@pytest.mark.parametrize("which", ["gate", "up"])
@pytest.mark.parametrize("f,zeros", pe.GLU_OVERFLOW, ids=pe.GLU_OVERFLOW_IDS)
def test_overflow_to_inf(gpu, f, zeros, which, m, n, k):
    """MXFP6 (with zeros in x also 0 * inf): +-inf weights in the gate give silu(+-inf) * u = +-inf or NaN,
    in the up silu(g) * +-inf, which is NaN where silu(g) is 0 (g = 0, and g <= -88.75, where expf
    overflows). fp8: the same from f32 sums that pass 2^129; warm rows (finite at E = 120) and
    every kept column stay in the exact regimes."""
    c = pe.swiglu_overflow(f, which, m, n, k, zeros=zeros)
    rows, keep = c.extra["rows"], c.extra["keep"]
    rest = np.setdiff1d(np.arange(n), rows)
    pe.prove_swiglu(c, keep)
    pe.prove_warm(c)
    clean = _run(c, img=c.extra["clean_img"])
    outs = _check(c, rest, check=pe.check_regimes_to_inf)
    assert len(outs) == len(clean) >= 2
    for (y32, y16), (c32, c16) in zip(outs, clean):  # variant by variant
        le.assert_f32_equal(y32[:, rows], le.expected_f32(c.extra["want"]).astype(np.float64))
        le.assert_rows_bit_equal(y32.t(), c32.t(), keep)
        le.assert_rows_bit_equal(y16.t(), c16.t(), keep)


@pytest.mark.parametrize("m,n,k", NONFINITE)
@pytest.mark.parametrize("f", GLU_FORMATS, ids=IDS)
def test_nonfinite_activations(gpu, f, m, n, k):
    c = pe.swiglu_nonfinite(f, n, k, m)
    pe.prove_swiglu(c)
    clean = _check(c)
    r = c.extra["row"]
    for xb, g, u in c.extra["bad"].values():
        want = le.silu_mul64(g[r], u[r])
        assert not np.isfinite(want).any()
        outs = _run(c, x=xb)
        assert len(outs) == len(clean) >= 2
        for (y32, y16), (c32, c16) in zip(outs, clean):
            le.assert_f32_equal(y32[r], le.expected_f32(want).astype(np.float64))
            le.assert_rows_bit_equal(y32, c32, c.extra["keep"])
            le.assert_rows_bit_equal(y16, c16, c.extra["keep"])


# ---------------------------------------------------------------- 3. far into a large layer

@pytest.mark.parametrize("name", list(pe.FAR_GLU))
def test_far_into_a_large_layer(gpu, name):
    """S behind c0 chunks of 64 KiB that are allocated and never written or read; far_glu_case
    asserts the positions (elem_offset > 2^32, first_byte < boundary < last_byte, the up behind the
    boundary). Both ranges are also unpacked and compared with the reference bits."""
    c = pe.far_glu_case(name)
    f = pe.FAR_GLU[name][0]
    le.prove_exact(c.xf, c.wf, 1.0, f.uw, c.want)
    g, u = c.want, c.xf @ c.wu.T
    le.prove_exact(c.xf, c.wu, 1.0, f.uw, u)
    assert c.need < 5 * pe.GB and pe.wrapped_inside(c)
    torch.cuda.empty_cache()
    buf = c.place(DEV)
    try:
        for split_k, row_tiles in _variants(c.n):
            y32 = pe.far_swiglu(c, buf, out_dtype=torch.float32, split_k=split_k, row_tiles=row_tiles)
            check_exact_regimes(y32, g, u)
            y16 = pe.far_swiglu(c, buf, split_k=split_k, row_tiles=row_tiles)
            assert np.array_equal(le.mx.bf16_tensor_bits(y16), le.f32_to_bf16_bits(y32.cpu().numpy()).reshape(-1))
        assert np.array_equal(le.mx.bf16_tensor_bits(pe.far_unpack(c, buf)), c.bits)
        assert np.array_equal(le.mx.bf16_tensor_bits(pe.far_unpack(c, buf, c.up_s)), c.up_bits)
    finally:
        del buf
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 4. passes, strided output, views of x

@pytest.mark.parametrize("n,k,ld", [(48, 160, 80), (528, 1056, 560), (64, 160, 80)])
@pytest.mark.parametrize("m", [129, 200])
@pytest.mark.parametrize("f", GLU_FORMATS, ids=IDS)
def test_several_passes_into_a_strided_out(gpu, f, m, n, k, ld):
    """M = 129 and 200: three and four passes of 64 rows, the last one partial. `out` is a view
    with a row stride beyond N inside a 0xA5-filled buffer: the values are in the exact regimes
    and every byte outside y[:M, :N] is unchanged."""
    c = pe.swiglu_clean(f, m, n, k)
    pe.prove_swiglu(c)
    p = torch.from_numpy(c.img).to(DEV)
    for split_k in (0, 4):
        kw = dict(img=p, split_k=split_k, row_tiles=2 if n == 64 else 0)  # N = 64: two row tiles per wave forced
        y32 = pe.run_swiglu(c, DEV, out_dtype=torch.float32, **kw)
        check_exact_regimes(y32, c.g, c.u)
        for dtype in (torch.float32, torch.bfloat16):
            buf, y = le.strided_out(m, n, ld, dtype, DEV)
            got = pe.run_swiglu(c, DEV, out=y, **kw)
            assert got.data_ptr() == y.data_ptr() and y.stride(0) == ld
            if dtype == torch.float32:
                assert torch.equal(y.contiguous().view(torch.int32), y32.view(torch.int32))
            else:
                assert np.array_equal(le.mx.bf16_tensor_bits(y), le.f32_to_bf16_bits(y32.cpu().numpy()).reshape(-1))
            le.assert_untouched_outside(buf, m, n, ld, dtype)


@pytest.mark.parametrize("f", GLU_FORMATS, ids=IDS)
def test_views_of_x(gpu, f):
    """x as [2, 9, k], as sliced and transposed non-contiguous views and as a contiguous view 2
    bytes off a 16-byte boundary: the bits of the contiguous, aligned x; leading dimensions kept."""
    k, n = 160, 48
    c = pe.swiglu_clean(f, 18, n, k)
    pe.prove_swiglu(c)
    p = torch.from_numpy(c.img).to(DEV)
    xd = c.x.to(DEV)
    for split_k in SPLITS:
        base = pe.run_swiglu(c, DEV, x=xd, img=p, out_dtype=torch.float32, split_k=split_k)
        base16 = pe.run_swiglu(c, DEV, x=xd, img=p, split_k=split_k)
        check_exact_regimes(base, c.g, c.u)
        for name, v in le.x_views(xd).items():
            y = pe.run_swiglu(c, DEV, x=v, img=p, out_dtype=torch.float32, split_k=split_k)
            assert tuple(y.shape) == tuple(v.shape[:-1]) + (n,), name
            assert torch.equal(y.reshape(18, n).view(torch.int32), base.view(torch.int32)), name
            y16 = pe.run_swiglu(c, DEV, x=v, img=p, split_k=split_k)
            assert torch.equal(y16.reshape(18, n).view(torch.int16), base16.view(torch.int16)), name
