"""The W4A8 route on the block-scaled MFMA (csrc/kernels/mxfp8_act.hip, csrc/kernels/mxfp4_mx.hip;
ops.mxfp8_quantize_rows, ops.mxfp4_linear and ops.mxfp4_swiglu with act="mxfp8",
decoder_forward(act="mxfp8")): x is quantized to MXFP8 and multiplied with the MXFP4 weights as
both lie in memory, y[m][n] = sum_k x^[m][k] w^[n][k] with one f32 accumulator per element.

The references are those of test_mxfp4_mx_host.py: the quantizer is held to the host codec byte
for byte, the products to float64 of (x^, w^) with x^ dequantized in numpy from the HOST codec's
bytes and w^ the numpy reference of test_mxfp4_linear_host.py. The cases are those of
test_gpu_mxfp4_tiled.py at this kernel's own tile (BM, BN from the binding), the contract -
batch invariance - is the same. Every x here is what the quantizer makes of it; hand-made codes
and scale bytes (subnormal products, both ends of both scale ranges, every e4m3 code, NaN scales
and codes) and the addressing extremes are in test_gpu_mxfp4_mx_extremes.py."""
import os

import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.weights import decoder_forward

import decoder_packed_reference as dp
import test_gpu_mxfp4_linear as lin
import test_gpu_mxfp4_swiglu as glu
import test_gpu_mxfp4_tiled as tiled
from test_mxfp4_linear_host import (bf16_tensor_bits, chunk_table, handmade_image, int_x, ref_weight, scale_index)
from test_mxfp4_mx_host import SPECIAL, bits_to_tensor, dequantize, host_quantize, special_bits

pytestmark = pytest.mark.gpu

KiB = 1 << 10
BM, BN = _core.mxfp4_mx_tile()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _linear(x, img, n, k, total, chunk, off=0, **kw):
    p = img if torch.is_tensor(img) else torch.from_numpy(img).cuda()
    return ops.mxfp4_linear(x.cuda(), p, n, k, src_bytes=2 * total, chunk_bytes=chunk, elem_offset=off, act="mxfp8", **kw)


def _swiglu(x, img, n, k, total, chunk, gate, up, **kw):
    p = img if torch.is_tensor(img) else torch.from_numpy(img).cuda()
    return ops.mxfp4_swiglu(x.cuda(), p, n, k, src_bytes=2 * total, chunk_bytes=chunk, gate_offset=gate, up_offset=up,
                            act="mxfp8", **kw)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------- the quantizer

def _assert_gpu_quantizer_is_the_host_codec(x):
    q, s = ops.mxfp8_quantize_rows(x.cuda())
    assert q.is_cuda and q.dtype == torch.uint8 and q.shape == x.shape
    assert s.is_cuda and s.dtype == torch.uint8 and s.shape == (*x.shape[:-1], x.shape[-1] // 32)
    hq, hs = host_quantize(x)
    assert np.array_equal(q.cpu().numpy(), hq)
    assert np.array_equal(s.cpu().numpy(), hs)


@pytest.mark.parametrize("rows,k,seed", SPECIAL)
def test_quantizer_equals_host_on_special_values(gpu, rows, k, seed):
    _assert_gpu_quantizer_is_the_host_codec(bits_to_tensor(special_bits(rows, k, seed)).view(rows, k))


@pytest.mark.parametrize("k", [32, 160, 1056])
@pytest.mark.parametrize("m", [1, 17, BM + 1])
def test_quantizer_equals_host(gpu, m, k):
    """Random bf16 bit patterns (every exponent, inf and NaN among them) and N(0, 1) rows; M K / 8
    threads: a partial last workgroup at most sizes, a partial wave at M = 1, K = 32."""
    bits = np.random.default_rng(100 * m + k).integers(0, 1 << 16, (m, k), dtype=np.uint16)
    _assert_gpu_quantizer_is_the_host_codec(bits_to_tensor(bits).view(m, k))
    g = torch.Generator().manual_seed(m + k)
    _assert_gpu_quantizer_is_the_host_codec(torch.randn(m, k, generator=g).to(torch.bfloat16))


# ---------------------------------------------------------------- exact on integers

# M in {1, 17, BM - 1, BM, BM + 1, 2 BM + 5}, N in {16, 48, BN + 16, 528}, K in {32, 96, 128, 160, 1056}
# (the K tail alone, one step alone, a step and a tail, eight steps and a tail): the triples of
# test_gpu_mxfp4_tiled.py at this kernel's tile; every value appears, and one wide layer.
EXACT = [
    (1, 16, 32), (1, 48, 1056), (1, 528, 128), (1, BN + 16, 160), (17, 16, 96), (17, 48, 128), (17, 528, 160),
    (17, BN + 16, 1056), (BM - 1, 16, 160), (BM - 1, 48, 32), (BM - 1, BN + 16, 128), (BM - 1, 528, 96),
    (BM, 16, 1056), (BM, 48, 96), (BM, BN + 16, 32), (BM, 528, 160), (BM + 1, 16, 128), (BM + 1, 48, 160),
    (BM + 1, BN + 16, 96), (BM + 1, 528, 1056), (2 * BM + 5, 16, 32), (2 * BM + 5, 48, 1056),
    (2 * BM + 5, BN + 16, 160), (2 * BM + 5, 528, 128), (17, 4128, 96),
]


@pytest.mark.parametrize("m,n,k", EXACT)
def test_exact_on_integer_inputs(gpu, m, n, k):
    """x: integers in [-8, 8], which MXFP8 holds exactly (test_mxfp4_mx_host.py); W: random codes with
    scale bytes in {126, 127, 128}: every product is a multiple of 2^-2 and |sum| <= 96 K < 2^22, so
    the f32 output equals the float64 reference in any order of summation (mxprobe: the instruction
    adds such products exactly). 64 KiB chunks, the parameter at element 96 of a layer that goes
    on 64 elements behind it."""
    assert 96 * k < 2 ** 22
    off, chunk = 32 * 3, 64 * KiB
    total = off + n * k + 64
    img = handmade_image(total, chunk, 1000 * m + n + k)
    x, xf = int_x(m, k, m + 7 * k)
    want = xf @ ref_weight(img, total, chunk, off, n, k).T
    y = _linear(x, img, n, k, total, chunk, off, out_dtype=torch.float32)
    assert y.dtype == torch.float32 and y.shape == (m, n)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), want)


@pytest.mark.parametrize("m,n,k", [(BM + 1, 48, 96), (17, 528, 160)])
@pytest.mark.parametrize("layout", list(lin.LAYOUTS))
def test_exact_across_chunk_layouts(gpu, layout, m, n, k):
    chunk, off, behind = lin.LAYOUTS[layout]
    total = off + n * k + behind
    img = handmade_image(total, chunk, 77 + k)
    x, xf = int_x(m, k, 5 + m)
    want = xf @ ref_weight(img, total, chunk, off, n, k).T
    y = _linear(x, img, n, k, total, chunk, off, out_dtype=torch.float32)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), want)


# ---------------------------------------------------------------- random inputs

RANDOM = [(BM + 1, 528, 1056), (5, 48, 160), (2 * BM + 5, 528, 1056)]


@pytest.fixture(scope="module")
def random_case(gpu):
    """Per (m, n, k): x ~ N(0, 1) in bf16 and two [n, k] weights ~ N(0, 1/k), one behind the other in
    a layer packed by ops.mxfp4_pack_layer (4 KiB chunks); the f32 and bf16 results for the first
    weight, and the float64 reference of (x^, w^) with its bound, x^ from the host codec."""
    out = {}
    g = torch.Generator().manual_seed(12)
    for m, n, k in RANDOM:
        x = torch.randn(m, k, generator=g).to(torch.bfloat16)
        w = (torch.randn(2 * n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
        total = 2 * n * k
        packed = ops.mxfp4_pack_layer(w.view(-1).cuda(), 4096)
        img = packed.cpu().numpy()
        sb = np.concatenate([img[so: so + c // 32] for _, c, _, so in chunk_table(total, 4096)])
        assert sb.min() >= 100 and sb.max() <= 140  # far from the ends of the scale range
        wf = ref_weight(img, total, 4096, 0, n, k)
        xh = dequantize(*host_quantize(x))
        out[m, n, k] = dict(x=x, packed=packed, total=total, want=xh @ wf.T,
                            bound=k * 2.0 ** -23 * (np.abs(xh) @ np.abs(wf).T),
                            y32=_linear(x, packed, n, k, total, 4096, out_dtype=torch.float32),
                            y16=_linear(x, packed, n, k, total, 4096))
    return out


@pytest.mark.parametrize("m,n,k", RANDOM[:2])
def test_random_within_f32_accumulation_error(gpu, random_case, m, n, k):
    """|y - x^ w^T| <= K 2^-23 sum_k |x^_k w^_k| per element; the bf16 output is the f32 output
    rounded to nearest even, bit for bit."""
    c = random_case[m, n, k]
    err = np.abs(c["y32"].cpu().numpy().astype(np.float64) - c["want"])
    print("max err / bound", float((err / c["bound"]).max()))
    assert (err <= c["bound"]).all()
    assert c["y16"].dtype == torch.bfloat16
    assert np.array_equal(bf16_tensor_bits(c["y16"]), bf16_tensor_bits(c["y32"].to(torch.bfloat16)))


@pytest.mark.parametrize("m,n,k", [(17, 48, 320), (BM + 1, 144, 1056)])
def test_outliers_within_f32_accumulation_error(gpu, m, n, k):
    """x = N(0, 1) * 2^j with j uniform in -14 .. 3 per element: inside every group of 8 consecutive
    k, products 2^14 and more apart stand side by side, which one block-scaled MFMA does not add
    exactly (mxprobe, accum_align). The same bound as above: the kernel has to deliver it."""
    g = torch.Generator().manual_seed(7 * m + k)
    x = (torch.randn(m, k, generator=g) * torch.exp2(torch.randint(-14, 4, (m, k), generator=g).float())).to(torch.bfloat16)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
    total = n * k
    packed = ops.mxfp4_pack_layer(w.view(-1).cuda(), 4096)
    wf = ref_weight(packed.cpu().numpy(), total, 4096, 0, n, k)
    xh = dequantize(*host_quantize(x))
    want, bound = xh @ wf.T, k * 2.0 ** -23 * (np.abs(xh) @ np.abs(wf).T)
    err = np.abs(_linear(x, packed, n, k, total, 4096, out_dtype=torch.float32).cpu().numpy().astype(np.float64) - want)
    print("max err / bound", float((err / bound).max()))
    assert (err <= bound).all()


INV = RANDOM[2]


def test_one_row_alone_gives_the_bits_of_the_full_call(gpu, random_case):
    m, n, k = INV
    c = random_case[INV]
    for r in (0, 15, 16, BM - 1, BM, 2 * BM + 4):
        alone = _linear(c["x"][r: r + 1], c["packed"], n, k, c["total"], 4096, out_dtype=torch.float32)
        assert same_bits(alone, c["y32"][r: r + 1]), r
    head = _linear(c["x"][: BM + 1], c["packed"], n, k, c["total"], 4096, out_dtype=torch.float32)
    assert same_bits(head, c["y32"][: BM + 1])


def test_a_window_of_weight_rows_gives_its_columns(gpu, random_case):
    m, n, k = INV
    c = random_case[INV]
    part = _linear(c["x"], c["packed"], 48, k, c["total"], 4096, off=(BN - 16) * k, out_dtype=torch.float32)
    assert same_bits(part, c["y32"][:, BN - 16: BN + 32])


def test_merged_qkv_equals_three_calls(gpu, random_case):
    m, n, k = INV
    c = random_case[INV]
    col = 0
    for rows in (256, 144, 128):
        alone = _linear(c["x"], c["packed"], rows, k, c["total"], 4096, off=col * k, out_dtype=torch.float32)
        assert same_bits(alone, c["y32"][:, col: col + rows]), col
        col += rows
    assert col == n


def test_deterministic(gpu, random_case):
    m, n, k = INV
    c = random_case[INV]
    for _ in range(3):
        assert same_bits(_linear(c["x"], c["packed"], n, k, c["total"], 4096, out_dtype=torch.float32), c["y32"])


# ---------------------------------------------------------------- gated

@pytest.mark.parametrize("m,n,k,layout", tiled.GATED)
def test_gated_exact_on_integer_inputs(gpu, m, n, k, layout):
    """g and u are exact in f32 on these inputs, so the result is held to the epilogue's three
    regimes of test_gpu_mxfp4_swiglu.py. 64 KiB chunks, the parameters 64 elements apart."""
    chunk, first = 64 * KiB, 32 * 3
    second = first + n * k + 64
    gate, up = {"gate first": (first, second), "up first": (second, first), "equal": (first, first)}[layout]
    total = second + n * k + 64
    img, x, g, u = glu.exact_case(m, n, k, chunk, gate, up, total, 1000 * m + n + k)
    y = _swiglu(x, img, n, k, total, chunk, gate, up, out_dtype=torch.float32)
    print("worst err / bound", glu.check_exact_regimes(y, g, u))


@pytest.mark.parametrize("m,n,k", RANDOM[:2])
@pytest.mark.parametrize("up_first", [False, True])
def test_gated_epilogue_on_the_linears_sums(gpu, random_case, m, n, k, up_first):
    """g and u inside the gated kernel are the bits of two act="mxfp8" f32 linears (one K order), so
    against silu(g) * u of those in float64 only the epilogue's error is left."""
    c = random_case[m, n, k]
    a = (c["x"], c["packed"], n, k, c["total"], 4096)
    gate, up = (n * k, 0) if up_first else (0, n * k)
    g = _linear(*a, gate, out_dtype=torch.float32).cpu().numpy().astype(np.float64)
    u = _linear(*a, up, out_dtype=torch.float32).cpu().numpy().astype(np.float64)
    y32 = _swiglu(*a, gate, up, out_dtype=torch.float32)
    ref = glu.silu_mul(g, u)
    err, bound = np.abs(y32.cpu().numpy().astype(np.float64) - ref), glu.mixed_bound(ref, u)
    print("worst err / bound", float((err / bound).max()))
    assert (err <= bound).all()
    y16 = _swiglu(*a, gate, up)
    assert np.array_equal(bf16_tensor_bits(y16), bf16_tensor_bits(y32.to(torch.bfloat16)))
    assert same_bits(_swiglu(*a, gate, up, out_dtype=torch.float32), y32)


# ---------------------------------------------------------------- special values

def test_nan_block_poisons_only_its_column(gpu):
    m, n, k, chunk, gate = 17, 48, 160, 1024, 32 * 7
    up = gate + n * k
    total = up + n * k
    img = handmade_image(total, chunk, 9)
    x, _ = int_x(m, k, 3)
    clean = _linear(x, img, n, k, total, chunk, gate, out_dtype=torch.float32).cpu()
    clean_up = _linear(x, img, n, k, total, chunk, up, out_dtype=torch.float32).cpu()
    clean_glu = _swiglu(x, img, n, k, total, chunk, gate, up, out_dtype=torch.float32).cpu()
    assert not torch.isnan(clean).any() and not torch.isnan(clean_up).any() and not torch.isnan(clean_glu).any()
    for r, blk in [(21, 0), (47, 4), (0, 3)]:  # blocks of the main loop and of the K tail
        keep = [c for c in range(n) if c != r]
        for off in (gate, up):
            bad = img.copy()
            bad[scale_index(total, chunk, off + r * k + 32 * blk)] = 0xFF
            y = _swiglu(x, bad, n, k, total, chunk, gate, up, out_dtype=torch.float32).cpu()
            assert torch.isnan(y[:, r]).all()
            assert same_bits(y[:, keep], clean_glu[:, keep])
        y = _linear(x, bad, n, k, total, chunk, gate, out_dtype=torch.float32).cpu()  # `bad` is in up: clean
        assert same_bits(y, clean)
        y = _linear(x, bad, n, k, total, chunk, up, out_dtype=torch.float32).cpu()
        assert torch.isnan(y[:, r]).all() and same_bits(y[:, keep], clean_up[:, keep])
        y16 = _linear(x, bad, n, k, total, chunk, up).cpu()
        assert torch.isnan(y16[:, r]).all() and not torch.isnan(y16[:, keep]).any()


def test_nan_in_x_poisons_only_its_row_and_inf_saturates(gpu):
    """A NaN anywhere in a row of x (main step or tail, either sign) makes that row of y NaN and no
    other. +-inf saturates to the largest code of its block, as the CPU route has it: the rows with
    an inf are finite and, the sums being exact on these inputs, equal the CPU route's."""
    m, n, k, chunk = BM + 1, 48, 160, 1024
    total = n * k
    img = handmade_image(total, chunk, 21)
    x, _ = int_x(m, k, 22)
    clean = _linear(x, img, n, k, total, chunk, out_dtype=torch.float32).cpu()
    x[3, 7], x[5, 130], x[20, 1], x[20, 150] = float("inf"), float("-inf"), float("inf"), float("-inf")
    x[BM, 40] = float("nan")
    x[9, 159] = -torch.tensor(float("nan"), dtype=torch.bfloat16)
    rows_nan, rows_inf = [9, BM], [3, 5, 20]
    y = _linear(x, img, n, k, total, chunk, out_dtype=torch.float32).cpu()
    y_glu = _swiglu(x, np.concatenate([img, img]), n, k, 2 * total, chunk, 0, total, out_dtype=torch.float32).cpu()
    for t in (y, y_glu):
        assert torch.isnan(t[rows_nan]).all()
        assert not torch.isnan(t[[r for r in range(m) if r not in rows_nan]]).any()
    rest = [r for r in range(m) if r not in rows_nan + rows_inf]
    assert same_bits(y[rest], clean[rest])
    y_cpu = ops.mxfp4_linear(x, torch.from_numpy(img), n, k, src_bytes=2 * total, chunk_bytes=chunk,
                             out_dtype=torch.float32, act="mxfp8")
    fin = [r for r in range(m) if r not in rows_nan]
    assert bool(torch.isfinite(y[rows_inf]).all()) and torch.equal(y[fin], y_cpu[fin])
    assert not torch.equal(y[rows_inf], clean[rows_inf])


# ---------------------------------------------------------------- addressing

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gated", [False, True])
def test_writes_only_its_output(gpu, dtype, gated):
    """M = BM + 1 leaves 15 rows of the second tile and N = 48 a wave and most of the column tile
    unused: with y a view into a 0xA5-filled buffer and a row stride larger than N, every byte
    outside y[:M, :N] is unchanged."""
    m, n, k, chunk = BM + 1, 48, 160, 1024
    total = 2 * n * k
    img, x, g, u = glu.exact_case(m, n, k, chunk, 0, n * k, total, 31)
    es = 2 if dtype == torch.bfloat16 else 4
    ld, lead = 80, 3 * 80 + 8
    buf = torch.full(((lead + (m + 3) * ld) * es,), 0xA5, dtype=torch.uint8, device="cuda")
    y = buf.view(dtype)[lead: lead + m * ld].view(m, ld)[:, :n]
    if gated:
        got = _swiglu(x, img, n, k, total, chunk, 0, n * k, out=y)
        want = _swiglu(x, img, n, k, total, chunk, 0, n * k, out_dtype=torch.float32).to(dtype)
    else:
        got = _linear(x, img, n, k, total, chunk, 0, out=y)
        want = torch.from_numpy(g).to(dtype).cuda()
    assert got.data_ptr() == y.data_ptr()
    assert same_bits(y.contiguous(), want)
    mask = torch.ones(buf.numel() // es, dtype=torch.bool)
    mask[lead: lead + m * ld].view(m, ld)[:, :n] = False
    outside = buf.cpu().view(-1, es)[mask]
    assert outside.numel() and bool((outside == 0xA5).all())


def test_rejects_bad_gpu_arguments(gpu):
    n, k, chunk = 64, 96, 1024
    total = 2 * n * k
    p = torch.from_numpy(handmade_image(total, chunk, 1)).cuda()
    x = torch.zeros(5, k, dtype=torch.bfloat16, device="cuda")
    y = torch.empty(5, n, dtype=torch.float32, device="cuda")
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk, act="mxfp8")
    with pytest.raises(ValueError, match="split_k"):
        ops.mxfp4_linear(x, p, n, k, split_k=2, **kw)
    with pytest.raises(ValueError, match="row_tiles"):
        ops.mxfp4_swiglu(x, p, n, k, gate_offset=0, up_offset=n * k, row_tiles=2, **kw)
    with pytest.raises(ValueError, match="outside"):
        ops.mxfp4_linear(x, p, n, k, elem_offset=n * k + 32, **kw)
    with pytest.raises(ValueError, match="act"):
        ops.mxfp4_linear(x, p, n, k, **{**kw, "act": "mxfp6"})
    q, s = ops.mxfp8_quantize_rows(x)
    a = (q.data_ptr(), s.data_ptr(), 5, n, k, y.data_ptr(), n, False, 0)
    gpu.mxfp4_linear_mx(p.data_ptr(), 2 * total, chunk, 32, *a)
    with pytest.raises(RuntimeError):  # the launchers check again on their own
        gpu.mxfp4_linear_mx(p.data_ptr(), 2 * total, chunk, 16, *a)
    with pytest.raises(RuntimeError):
        gpu.mxfp4_swiglu_mx(p.data_ptr(), 2 * total, chunk, 0, n * k + 32, *a)
    with pytest.raises(RuntimeError):
        gpu.mxfp8_quantize_rows(x.data_ptr(), 5, 48, q.data_ptr(), s.data_ptr(), 0)


# ---------------------------------------------------------------- the decoder layer

def bf16_rne(v):
    """float64 -> the nearest bf16 value (ties to even) as float64, for values in bf16's normal range."""
    mant, e = np.frexp(v)
    return np.ldexp(np.rint(mant * 256), e - 8)


@pytest.mark.parametrize("spec_name", ["tiny", "uneven"])
def test_decoder_forward_act(gpu, monkeypatch, spec_name):
    """BM + 1 rows as batch x seq through decoder_forward(act="mxfp8"): four quantize and four matmul
    launches, and every launch in situ - on the input it was given, host-quantized here - delivers
    bf16(v) for some v within the f32 bound of the float64 product of (x^, w^) (the gated launch:
    within the bound of decoder_packed_reference.py's check B, the two sums' bounds propagated
    through the epilogue). The whole-layer distance from the float64 reference of the unquantized
    layer is printed and recorded, not asserted: it is the price of 8-bit activations.

    Measured on MI355X with one MFMA per step: the down_proj of `uneven` (N = 192, K = 320, 129
    rows), whose input - silu(g) * u - has outliers, lay outside K 2^-23 sum |x^ w^| in 23 of 24768
    f32 elements, by up to 2.33 bounds, and 1 bf16 output outside the rounded interval: inside a
    group of 8 consecutive k the instruction drops a product 2^14 below the largest (mxprobe,
    accum_align). The kernel now keeps such products in separate MFMAs and every launch is within
    it."""
    rows = next((b, (BM + 1) // b) for b in (3, 1) if (BM + 1) % b == 0)
    c = dp.case(spec_name, rows, "mxfp4-5k")
    assert c.batch * c.seq == BM + 1
    params = c.layer.packed_params("cuda")
    x = c.xt.cuda()
    calls, rec = [], []
    for name in ("mxfp4_linear", "mxfp4_swiglu", "mxfp4_linear_tiled", "mxfp4_swiglu_tiled", "mxfp8_quantize_rows",
                 "mxfp4_linear_mx", "mxfp4_swiglu_mx"):
        def counted(*a, _fn=getattr(_core, name), _name=name, **kw):
            calls.append(_name)
            return _fn(*a, **kw)
        monkeypatch.setattr(_core, name, counted)
    for name in ("mxfp4_linear", "mxfp4_swiglu"):
        def wrapped(xx, packed, n, k, _fn=getattr(ops, name), _name=name, **kw):
            y = _fn(xx, packed, n, k, **kw)
            rec.append((_name, xx.detach().clone(), n, k, dict(kw), y))
            return y
        monkeypatch.setattr(ops, name, wrapped)
    y = decoder_forward(x, params, c.spec, act="mxfp8")
    torch.cuda.synchronize()
    q, l, s = "mxfp8_quantize_rows", "mxfp4_linear_mx", "mxfp4_swiglu_mx"
    assert calls == [q, l, q, l, q, s, q, l]
    assert [r[0] for r in rec] == ["mxfp4_linear", "mxfp4_linear", "mxfp4_swiglu", "mxfp4_linear"]
    launches = list(rec)
    # the whole layer first: recorded whatever the launches' checks below say
    ctl = decoder_forward(x, {k: v.cuda() for k, v in c.layer.dense.items()}, c.spec).float().cpu().numpy()
    y16 = decoder_forward(x, params, c.spec, tiled=True).float().cpu().numpy()
    line = (f"{c.id} act=mxfp8: whole-layer distance from float64 {dp.rel(y.float().cpu().numpy(), c.y64):.3e} "
            f"(W4A16 tiled {dp.rel(y16, c.y64):.3e}, plain bf16 torch {dp.rel(ctl, c.y64):.3e}, bf16 floor {c.e16:.3e})")
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles", "mxfp4_mx"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mxfp4_mx", f"decoder_distance_{spec_name}.txt"), "w") as f:
        f.write(line + "\n")
    for op, xx, n, k, kw, yy in launches:
        assert kw["act"] == "mxfp8" and "tiled" not in kw and yy.dtype == torch.bfloat16
        xh = dequantize(*host_quantize(xx.reshape(-1, k)))
        got = yy.float().cpu().numpy().astype(np.float64).reshape(-1, n)
        if op == "mxfp4_swiglu":
            (g, bg), (u, bu) = (dp.linear_bound(xh, c.layer.weight(kw[o], n, k)) for o in ("gate_offset", "up_offset"))
            want = dp.silu(g) * u
            bound = (4 * 2.0 ** -23 * np.abs(want) + 1.1 * np.abs(u) * bg + np.abs(dp.silu(g)) * bu + 1.1 * bg * bu
                     + 2.0 ** -100)
        else:
            want, bound = dp.linear_bound(xh, c.layer.weight(kw["elem_offset"], n, k))
        lo, hi = bf16_rne(want - bound), bf16_rne(want + bound)
        print(f"{c.id} {op} N = {n} K = {k}: bf16 outputs outside the rounded interval "
              f"{int(((got < lo) | (got > hi)).sum())} of {got.size}")
        assert ((lo <= got) & (got <= hi)).all(), (op, n, k)
