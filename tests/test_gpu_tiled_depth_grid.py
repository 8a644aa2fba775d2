"""The four many-row gfx950 kernels (csrc/kernels/{mxfp4,fp8,mxfp6}_tiled.hip through tiled=True,
mxfp4_mx.hip through act="mxfp8") at the K depths and the grids they are served at: the table of
tiled_depth_grid.py - 2 to 416 steps of the K loop with and without a tail, after an even and an odd
count; grids of 255, 512 (two workgroups per CU) and 2049 workgroups (more than eight per CU: a second
round starts while the first is mid-K), with r8 = 7, 0 and 1 in the XCD remap; and both at once.
test_tiled_depth_grid_host.py shows on the CPU that the table is what it claims, that every case is
exact in f32 in any summation order, and that a lost K step or a swapped tile changes the expectation.

Per exact case: the f32 output equals the float64 x W^T element for element over the whole output
(gated: check_exact_regimes on exact g and u, and the two linears on the same inputs are exact); the
bf16 output is the f32 one rounded once; both are written into a view with row stride N + 16 of a
0xA5-filled buffer whose every byte outside y[:M, :N] stays (compared on the device). A second call
gives equal bits and the last row alone the bits of the full call; on the G2 and both-at-once cases
rows 0, BM - 1, BM alone and weight rows [BN - 16, BN + 32) as a parameter of their own do too.

Random and outlier inputs at K = 8160 and 28672 are held to K 2^-23 sum |x w| (W4A8: over x^ and w^);
for fp8 and MXFP6 the tiled f32 result is the untiled op's with split_k=1 bit for bit, linear and
gated. ops.mxfp8_quantize_rows at these depths equals the host codec byte for byte.

Measured on MI355X, largest err / bound of the random cases at (BM + 1, 144, 8160) and
(BM + 1, 144, 28672): MXFP4 2.6e-5 and 8.0e-6, MXFP6 3.9e-5 and 1.5e-5, fp8 block 32 6.6e-5 and 1.9e-5,
fp8 block 128 7.1e-5 and 2.1e-5, W4A8 6.4e-6 and 2.0e-6, W4A8 on the outlier x 4.5e-5; the worst
err / bound of the gated epilogue's middle regime over all exact cases 0.36. The bounds are the
derived ones and are not tightened to these. 256 tests, 18.4 s for the file, the slowest test 0.54 s
(0.83 s to build the inputs of a both-at-once case). No bug found."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import ops

import linear_extremes as le
import tiled_depth_grid as tdg
from test_gpu_mxfp4_swiglu import check_exact_regimes
from test_mxfp4_mx_host import host_quantize

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = dict(out_dtype=torch.float32)


def test_the_chip_has_no_more_cus_than_the_table_assumes(gpu):
    """The grid cases count workgroups against 256 CUs; a larger chip needs a larger table."""
    assert torch.cuda.get_device_properties(0).multi_processor_count <= tdg.CUS


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


@pytest.fixture(scope="module", params=tdg.EXACT, ids=[tdg.exact_id(p) for p in tdg.EXACT])
def built(request, gpu):
    """One (variant, case): inputs, the image on the device, the float64 expectation (torch on the
    device) - built once and left unchanged; the tests add y32, the full f32 result."""
    b = tdg.Built(*request.param)
    b.p = torch.from_numpy(b.img).to(DEV)
    b.xd = b.x.to(DEV)
    b.dev_wants = b.wants(DEV)
    b.y32 = None
    return b


def _guarded(b, dtype, **kw):
    """The case's result written through `out`, a view with row stride N + 16 into a 0xA5-filled
    buffer; every byte outside y[:M, :N] is unchanged, compared on the device."""
    ld = b.n + 16
    es = 2 if dtype == torch.bfloat16 else 4
    buf, y = le.strided_out(b.m, b.n, ld, dtype, DEV)
    lead = 3 * ld + 8
    assert y.data_ptr() == buf.data_ptr() + lead * es and y.stride(0) == ld
    got = b.run(DEV, x=b.xd, img=b.p, out=y, **kw)
    assert got.data_ptr() == y.data_ptr() and got.dtype == dtype
    kept = (buf == 0xA5).view(-1, es).all(1)  # per element of the buffer
    body = kept[lead: lead + b.m * ld].view(b.m, ld)
    assert bool(kept[:lead].all()) and bool(kept[lead + b.m * ld:].all()) and bool(body[:, b.n:].all())
    return y.contiguous()


def _assert_equal_f64(y32, want, what):
    got = y32.double()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError((what, len(bad), [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)]))
                                               for i in bad[:6]]))


def _y32(b):
    if b.y32 is None:
        b.y32 = _guarded(b, torch.float32)
    return b.y32


def test_f32_output_is_the_float64_product_and_nothing_else_is_written(built):
    b = built
    y = _y32(b)
    assert y.dtype == torch.float32 and tuple(y.shape) == (b.m, b.n)
    if not b.gated:
        _assert_equal_f64(y, b.dev_wants[0], tdg.exact_id((b.variant, b.case)))
        return
    print(b.variant, b.case.id, "worst err / bound", check_exact_regimes(y, *(w.cpu().numpy() for w in b.dev_wants)))
    for i in (0, 1):  # g and u themselves: the linear kernel on the same rows is exact
        _assert_equal_f64(b.run(DEV, x=b.xd, img=b.p, linear_of=i, **F32), b.dev_wants[i], ("linear of", i))


def test_bf16_output_is_the_f32_output_rounded_once(built):
    b = built
    y16 = _guarded(b, torch.bfloat16)
    assert same_bits(y16, _y32(b).to(torch.bfloat16))  # to nearest even
    if not b.gated:  # and so the float64 product rounded once
        assert same_bits(y16, b.dev_wants[0].float().to(torch.bfloat16))


def test_batch_invariance(built):
    """A second call gives equal bits and the last row alone the bits of the full call. On G2 and the
    both-at-once cases also rows 0, BM - 1 and BM alone, and weight rows [BN - 16, BN + 32) as a
    parameter of their own (N = 48, the offsets moved by (BN - 16) K) give their columns."""
    b = built
    y = _y32(b)
    assert same_bits(b.run(DEV, x=b.xd, img=b.p, **F32), y)
    bm, bn = tdg.tile(b.variant)
    rows = [b.m - 1] + ([0, bm - 1, bm] if b.case.name in ("G2", "both") else [])
    for r in rows:
        assert same_bits(b.run(DEV, x=b.xd[r: r + 1], img=b.p, **F32), y[r: r + 1]), r
    if b.case.name in ("G2", "both"):
        part = b.run(DEV, x=b.xd, img=b.p, offs=[o + (bn - 16) * b.k for o in b.offs], n=48, **F32)
        assert same_bits(part, y[:, bn - 16: bn + 32])


# ---------------------------------------------------------------- random and outlier inputs at depth

RANDOM = [(v, s, False) for v in tdg.VARIANTS for s in range(2)] + [("w4a8", 1, True)]
RANDOM_IDS = [f"{v}-{s}" + ("-outliers" if o else "") for v, s, o in RANDOM]


@pytest.mark.parametrize("variant,shape,outliers", RANDOM, ids=RANDOM_IDS)
def test_random_within_f32_accumulation_error(gpu, variant, shape, outliers):
    """|y - y_ref| <= K 2^-23 sum_k |x w| per element (W4A8: x^ from the host codec's bytes); the
    bf16 output is the f32 output rounded. fp8 and MXFP6: the tiled f32 results are the untiled op's
    with split_k=1 bit for bit, linear and gated (the contract the older files assert at K = 1056)."""
    m, n, k = tdg.random_shapes(variant)[shape]
    c = tdg.Random(variant, m, n, k, DEV, outliers)
    y32, y16 = c.run(DEV, **F32), c.run(DEV)
    err = np.abs(y32.cpu().numpy().astype(np.float64) - c.want)
    print(variant, (m, n, k), "outliers" if outliers else "random", "max err / bound", float((err / c.bound).max()))
    assert (err <= c.bound).all()
    assert y16.dtype == torch.bfloat16 and same_bits(y16, y32.to(torch.bfloat16))
    if c.f.name in ("fp8", "mxfp6"):
        assert same_bits(c.run(DEV, untiled=True, **F32), y32)
        assert same_bits(c.run(DEV, gated=True, untiled=True, **F32), c.run(DEV, gated=True, **F32))


def test_quantizer_equals_the_host_codec_at_depth(gpu):
    """ops.mxfp8_quantize_rows on the (2 BM + 5, 8192) integers of the both-at-once case and on the
    (BM + 1, 28672) random and outlier activations: the host codec's bytes."""
    bm = tdg.tile("w4a8")[0]
    both = next(c for c in tdg.cases("w4a8", False) if c.name == "both")
    hi = tdg.level(tdg.fmt("w4a8"), both.k)[0]
    xs = [le.scaled_ints(both.m, both.k, 5, 0, -hi, hi)[0], tdg.outlier_x(bm + 1, 28672),
          torch.randn(bm + 1, 28672, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)]
    assert tuple(xs[0].shape) == (2 * bm + 5, 8192)
    for x in xs:
        q, s = ops.mxfp8_quantize_rows(x.to(DEV))
        hq, hs = host_quantize(x)
        assert np.array_equal(q.cpu().numpy(), hq) and np.array_equal(s.cpu().numpy(), hs)
