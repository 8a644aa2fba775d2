"""MXFP8 activations and the W4A8 route (act="mxfp8") on the CPU: the host codec of
core/mxfp8_act.h (ops.mxfp8_quantize_rows), the CPU routes of ops.mxfp4_linear and
ops.mxfp4_swiglu with act="mxfp8", and decoder_forward(act="mxfp8").

The format is core/fp8.h at block 32 with the scale stored as its exponent byte, so the codec
is held to the fp8 host codec (byte for byte) and to the error property of the format; the
products are held to a float64 reference of the dequantized operands (x^ = code * 2^(byte -
127) computed here in numpy, w^ the numpy reference of test_mxfp4_linear_host.py). The gfx950
kernels are checked against the same references in test_gpu_mxfp4_mx.py."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.weights import decoder_forward

import decoder_packed_reference as dp
from test_mxfp4_linear_host import bf16_tensor_bits, bits_to_f64, handmade_image, int_x, ref_weight

KiB = 1 << 10


# ---------------------------------------------------------------- the reference

def bits_to_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def e4m3_to_f64(codes):
    """OCP e4m3fn codes (uint8 array) as float64; 0x7F and 0xFF are NaN."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    v = np.where(e == 0, np.ldexp(m.astype(np.float64), -9), np.ldexp((8 + m).astype(np.float64), e - 10))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return np.where(c & 0x80, -v, v)


def dequantize(codes, scales):
    """x^ [rows, K] in float64 from codes [rows, K] and scale bytes [rows, K / 32]: exact."""
    codes, scales = np.asarray(codes), np.asarray(scales)
    e = np.repeat(scales.astype(np.int64) - 127, 32, axis=-1)
    return np.ldexp(e4m3_to_f64(codes), e)


def host_quantize(x):
    """(codes, scales) of ops.mxfp8_quantize_rows on the CPU, as numpy arrays."""
    q, s = ops.mxfp8_quantize_rows(x.cpu())
    return q.numpy(), s.numpy()


def special_bits(rows, k, seed):
    """Random bf16 bit patterns [rows, k] - every exponent, so subnormals, huge values and, by
    chance, inf and NaN - with blocks planted by hand: +-0 only, subnormals only, one +inf, one
    -inf, a NaN of each sign, the largest finite value (E = 120, the 240 limit), an inf among
    subnormals."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 16, (rows, k), dtype=np.uint16)
    flat = b.reshape(-1, 32)
    n = flat.shape[0]
    plant = [
        np.where(rng.integers(0, 2, 32) == 1, 0x8000, 0x0000),        # +-0
        rng.integers(1, 0x80, 32) | (rng.integers(0, 2, 32) << 15),   # bf16 subnormals
    ]
    for v, pos in [(0x7F80, 3), (0xFF80, 17), (0x7FC1, 0), (0xFFFF, 31), (0x7F7F, 8), (0xFF7F, 9)]:
        blk = rng.integers(0x3000, 0x4800, 32)  # finite values around 1
        blk[pos] = v
        plant.append(blk)
    blk = rng.integers(1, 0x80, 32)
    blk[5] = 0x7F80
    plant.append(blk)
    for i, blk in enumerate(plant):
        flat[(i * 7) % n] = np.asarray(blk, dtype=np.uint16)
    return flat.reshape(rows, k)


SPECIAL = [(9, 32, 1), (5, 96, 2), (4, 1056, 3)]  # at least 9 blocks: every planted block survives


# ---------------------------------------------------------------- the quantizer

@pytest.mark.parametrize("rows,k,seed", SPECIAL)
def test_quantizer_is_the_fp8_codec_at_block_32(rows, k, seed):
    bits = special_bits(rows, k, seed)
    x = bits_to_tensor(bits).view(rows, k)
    codes, scales = ops.mxfp8_quantize_rows(x)
    assert codes.dtype == torch.uint8 and codes.shape == (rows, k)
    assert scales.dtype == torch.uint8 and scales.shape == (rows, k // 32)
    n = rows * k
    ref = np.frombuffer(_core.fp8_pack_layer_host(bits.tobytes(), 2 * n, 32), dtype=np.uint8)
    assert ref.size == n + 4 * (n // 32)
    assert np.array_equal(codes.numpy().reshape(-1), ref[:n])
    f32 = ref[n:].view(np.uint32)
    assert ((f32 & 0x807FFFFF) == 0).all()  # powers of two
    assert np.array_equal(scales.numpy().reshape(-1), (f32 >> 23).astype(np.uint8))
    assert scales.min() >= 1 and scales.max() <= 247  # E in [-126, 120]: never the E8M0 NaN
    # NaN keeps its sign, inf saturates to the block's largest code
    nan = (bits & 0x7FFF) > 0x7F80
    assert np.array_equal(codes.numpy()[nan], (0x7F | (bits[nan] >> 8 & 0x80)).astype(np.uint8))
    inf = (bits & 0x7FFF) == 0x7F80
    assert inf.any() and nan.any()
    assert np.isin(codes.numpy()[inf] & 0x7F, (0x7E, 0x77)).all()  # 448, or 240 at E = 120
    # leading dimensions are kept
    q3, s3 = ops.mxfp8_quantize_rows(x.view(1, rows, k))
    assert q3.shape == (1, rows, k) and s3.shape == (1, rows, k // 32) and torch.equal(q3[0], codes)


@pytest.mark.parametrize("rows,k,seed", SPECIAL)
def test_quantization_error_on_finite_inputs(rows, k, seed):
    """|x^ - x| <= max(2^-4 |x|, 2^(E - 10)) per element: a three-bit mantissa under round to
    nearest, and half an e4m3 subnormal step of the block (which also covers the values a
    block's scale pushes below the format)."""
    bits = special_bits(rows, k, seed)
    codes, scales = host_quantize(bits_to_tensor(bits).view(rows, k))
    xf = bits_to_f64(bits.reshape(-1)).reshape(rows, k)
    xh = dequantize(codes, scales)
    fin = np.isfinite(xf)
    assert not np.isnan(xh[fin]).any() and np.isnan(xh[np.isnan(xf)]).all()
    e = np.repeat(scales.astype(np.int64) - 127, 32, axis=-1)
    bound = np.maximum(2.0 ** -4 * np.abs(xf), np.ldexp(1.0, e - 10))
    err = np.abs(xh - xf)
    assert (err[fin] <= bound[fin]).all(), float((err[fin] / bound[fin]).max())


def test_integers_quantize_losslessly():
    """Integers in [-8, 8]: amax 8 gives E = -5 and 32 j needs at most four significant bits (a
    smaller amax only moves E down); a block of zeros has E = 0."""
    x, xf = int_x(7, 160, 3)
    x[2, 32:64] = 0
    xf[2, 32:64] = 0
    x[3, :32] = torch.tensor([1.0, -1.0] * 16).to(torch.bfloat16)
    xf[3, :32] = [1.0, -1.0] * 16
    codes, scales = host_quantize(x)
    assert np.array_equal(dequantize(codes, scales), xf)
    assert scales[2, 1] == 127 and scales[3, 0] == 127 - 8 and scales[0, 0] in (127 - 5, 127 - 6)


def test_quantizer_rejects_bad_arguments():
    for bad in (torch.zeros(4, 32), torch.zeros(4, 48, dtype=torch.bfloat16), torch.zeros(0, 32, dtype=torch.bfloat16),
                torch.zeros((), dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            ops.mxfp8_quantize_rows(bad)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        _core.mxfp8_quantize_rows_host(0, 48, 0, 0)


# ---------------------------------------------------------------- the CPU route of act="mxfp8"

@pytest.mark.parametrize("chunk,off,m,n,k", [(1024, 32 * 7, 5, 48, 96), (64 * KiB, 32 * 3, 17, 16, 160),
                                              (1024, 0, 1, 16, 32), (64 * KiB, 32 * 3, 129, 48, 1056)])
def test_cpu_linear_is_exact_on_integers(chunk, off, m, n, k):
    """x^ = x on these inputs, W holds multiples of 2^-2 of magnitude at most 12: every partial
    sum is exact in f32, so the result equals the float64 reference."""
    assert 96 * k < 2 ** 22
    total = off + n * k
    img = handmade_image(total, chunk, 5)
    x, xf = int_x(m, k, 6)
    want = xf @ ref_weight(img, total, chunk, off, n, k).T
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk, elem_offset=off, act="mxfp8")
    y = ops.mxfp4_linear(x, torch.from_numpy(img), n, k, out_dtype=torch.float32, **kw)
    assert y.dtype == torch.float32 and y.shape == (m, n)
    assert np.array_equal(y.numpy().astype(np.float64), want)
    y16 = ops.mxfp4_linear(x.view(1, m, k), torch.from_numpy(img), n, k, tiled=True, **kw)  # `tiled` may be either
    assert y16.dtype == torch.bfloat16 and y16.shape == (1, m, n)
    assert np.array_equal(bf16_tensor_bits(y16), bf16_tensor_bits(y.to(torch.bfloat16)))  # rounded once


@pytest.fixture(scope="module")
def random_case():
    """x ~ N(0, 1), two [n, k] weights ~ N(0, 1 / k) one behind the other in a layer packed by the
    host codec (4 KiB chunks); x^ from the numpy dequantization of the host quantizer's bytes."""
    m, n, k = 21, 48, 1056
    g = torch.Generator().manual_seed(12)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    w = (torch.randn(2 * n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
    total = 2 * n * k
    img = np.frombuffer(_core.mxfp4_pack_layer_host(w.view(torch.int16).numpy().tobytes(), 4096), dtype=np.uint8).copy()
    xh = dequantize(*host_quantize(x))
    ws = [ref_weight(img, total, 4096, o, n, k) for o in (0, n * k)]
    return dict(m=m, n=n, k=k, x=x, img=torch.from_numpy(img), total=total, xh=xh, ws=ws)


def test_cpu_linear_random_against_float64(random_case):
    """|y - x^ w^T| <= K 2^-23 sum_k |x^_k w^_k| per element (f32 accumulation of K exact-in-f32
    operands, each product and each partial sum rounded once)."""
    c = random_case
    y = ops.mxfp4_linear(c["x"], c["img"], c["n"], c["k"], src_bytes=2 * c["total"], chunk_bytes=4096,
                         out_dtype=torch.float32, act="mxfp8")
    want = c["xh"] @ c["ws"][0].T
    bound = c["k"] * 2.0 ** -23 * (np.abs(c["xh"]) @ np.abs(c["ws"][0]).T)
    err = np.abs(y.numpy().astype(np.float64) - want)
    print("max err / bound", float((err / bound).max()))
    assert (err <= bound).all()
    # and it is the quantized activation, not x, that was multiplied
    xf = bits_to_f64(bf16_tensor_bits(c["x"])).reshape(c["m"], c["k"])
    assert (np.abs(xf @ c["ws"][0].T - want) > bound).any()


def test_cpu_swiglu_random_against_float64(random_case):
    c = random_case
    n, k = c["n"], c["k"]
    y = ops.mxfp4_swiglu(c["x"], c["img"], n, k, src_bytes=2 * c["total"], chunk_bytes=4096, gate_offset=0,
                         up_offset=n * k, out_dtype=torch.float32, act="mxfp8")
    (g, bg), (u, bu) = (dp.linear_bound(c["xh"], w) for w in c["ws"])
    want = dp.silu(g) * u
    bound = 4 * 2.0 ** -23 * np.abs(want) + 1.1 * np.abs(u) * bg + np.abs(dp.silu(g)) * bu + 1.1 * bg * bu + 2.0 ** -100
    err = np.abs(y.numpy().astype(np.float64) - want)
    print("max err / bound", float((err / bound).max()))
    assert (err <= bound).all()
    y16 = ops.mxfp4_swiglu(c["x"], c["img"], n, k, src_bytes=2 * c["total"], chunk_bytes=4096, gate_offset=0,
                           up_offset=n * k, act="mxfp8")
    assert np.array_equal(bf16_tensor_bits(y16), bf16_tensor_bits(y.to(torch.bfloat16)))


def test_act_rejects_bad_arguments():
    total, chunk = 32 * 7 + 2 * 48 * 96, 1024
    p = torch.from_numpy(handmade_image(total, chunk, 1))
    x = torch.zeros(5, 96, dtype=torch.bfloat16)
    lin = dict(src_bytes=2 * total, chunk_bytes=chunk, elem_offset=32 * 7)
    glu = dict(src_bytes=2 * total, chunk_bytes=chunk, gate_offset=32 * 7, up_offset=32 * 7 + 48 * 96)
    ops.mxfp4_linear(x, p, 48, 96, act="mxfp8", **lin)
    ops.mxfp4_swiglu(x, p, 48, 96, act="mxfp8", **glu)
    for fn, kw in ((ops.mxfp4_linear, lin), (ops.mxfp4_swiglu, glu)):
        with pytest.raises(ValueError, match="act"):
            fn(x, p, 48, 96, act="mxfp4", **kw)
        with pytest.raises(ValueError, match="act"):
            fn(x, p, 48, 96, act="fp8", tiled=True, **kw)
        with pytest.raises(ValueError, match="split_k"):
            fn(x, p, 48, 96, act="mxfp8", split_k=1, **kw)
        with pytest.raises(ValueError, match="row_tiles"):
            fn(x, p, 48, 96, act="mxfp8", row_tiles=1, **kw)
        with pytest.raises(ValueError, match="in_features"):
            fn(x[:, :80], p, 48, 80, act="mxfp8", **kw)


# ---------------------------------------------------------------- the decoder layer

def test_decoder_forward_act_on_the_cpu():
    c = dp.case("tiny", (3, 7), "mxfp4-5k")
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        for name in ("mxfp4_linear", "mxfp4_swiglu"):
            def wrapped(*a, _fn=getattr(ops, name), _name=name, **kw):
                seen.append((_name, kw.get("act"), "tiled" in kw))
                return _fn(*a, **kw)
            mp.setattr(ops, name, wrapped)
        y = decoder_forward(c.xt, c.layer.packed_params(), c.spec, act="mxfp8")
    assert y.dtype == torch.bfloat16 and y.shape == c.xt.shape and bool(torch.isfinite(y.float()).all())
    # q, k, v one by one on the CPU; every packed projection got act and nothing else new
    assert seen == [("mxfp4_linear", "mxfp8", False)] * 4 + [("mxfp4_swiglu", "mxfp8", False),
                                                             ("mxfp4_linear", "mxfp8", False)]
    # it is the W4A8 result: not the bits of the W4A16 pass
    assert not torch.equal(y, decoder_forward(c.xt, c.layer.packed_params(), c.spec))


@pytest.mark.parametrize("fmt", ["mxfp6-5k", "fp8b32-5k"])
def test_decoder_forward_act_rejects_other_formats(fmt):
    c = dp.case("tiny", (1, 1), fmt)
    with pytest.raises(ValueError, match="MXFP4"):
        decoder_forward(c.xt, c.layer.packed_params(), c.spec, act="mxfp8")
    with pytest.raises(ValueError, match="MXFP4"):  # the unfused routes too
        decoder_forward(c.xt, c.layer.packed_params(), c.spec, fuse=False, act="mxfp8")
    # one packed projection of another format among plain tensors
    with pytest.raises(ValueError, match="MXFP4"):
        decoder_forward(c.xt, {**c.layer.dense, "down_proj": c.layer.packed_params()["down_proj"]}, c.spec, act="mxfp8")


def test_decoder_forward_act_leaves_plain_tensors_alone():
    c = dp.case("tiny", (3, 7), "mxfp4-5k")
    y = decoder_forward(c.xt, c.layer.dense, c.spec, act="mxfp8")
    assert torch.equal(y.view(torch.int16), decoder_forward(c.xt, c.layer.dense, c.spec).view(torch.int16))
    with pytest.raises(ValueError, match="act"):
        decoder_forward(c.xt, c.layer.dense, c.spec, act="fp8")
