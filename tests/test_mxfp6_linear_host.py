"""ops.mxfp6_linear on the CPU: the CPU route of the op (the host reference dequantizes the
range, then F.linear), its argument checks, and MXFP6 PackedParams in decoder_forward next to
the other formats.

The reference is numpy and independent of the code under test: ref_unpack of test_mxfp6_host.py
applied to every chunk of the layer ([24-byte blocks][scale bytes] per source chunk, the tail
chunk on its own length), sliced to the parameter, then a float64 matmul. The gfx950 kernel is
checked against the same reference in test_gpu_mxfp6_linear.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.weights import (PRESETS, PackedParam, decoder_forward, flatten,
                                                             random_layer, unflatten, unflatten_packed)

from test_mxfp6_host import codes_to_bytes, ref_unpack

KiB = 1 << 10
SPEC = PRESETS["tiny"]


# ---------------------------------------------------------------- the reference

def chunk_table(total, chunk):
    """[(first element, elements, offset of the blocks, offset of the scale bytes)] per source chunk."""
    ce, pc = chunk // 2, chunk // 64 * 25
    return [(e0, min(ce, total - e0), c * pc, c * pc + min(ce, total - e0) // 32 * 24)
            for c, e0 in enumerate(range(0, total, ce))]


def ref_layer_bits(packed, total, chunk):
    """bf16 bit patterns of all `total` elements of a packed layer image (uint8 array)."""
    return np.concatenate([ref_unpack(packed[qo: so], packed[so: so + n // 32]) for _, n, qo, so in chunk_table(total, chunk)])


def bits_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def ref_weight(packed, total, chunk, off, n, k):
    """The [n, k] parameter at element `off` of the layer, float64."""
    return bits_to_f64(ref_layer_bits(packed, total, chunk)[off: off + n * k]).reshape(n, k)


def block_index(total, chunk, elem):
    """(offsets of the 24 bytes, offset of the scale byte) of the block that holds element `elem`:
    core/mxfp6.h's rule, written out."""
    for e0, n, qo, so in chunk_table(total, chunk):
        if e0 <= elem < e0 + n:
            r = (elem - e0) // 32
            return qo + 24 * r + np.arange(24), so + r
    raise IndexError(elem)


def handmade_image(total, chunk, seed, scales=(126, 127, 128), codes=range(64)):
    """A packed image of `total` elements (a multiple of 32) built by hand: random codes from
    `codes`, every block with its own random scale byte from `scales`. The defaults give weights
    that are multiples of 2^-4 of magnitude at most 15 (7.5 * 2)."""
    assert total % 32 == 0 and chunk % 1024 == 0
    rng = np.random.default_rng(seed)
    size = int(_core.mxfp6_packed_size(2 * total, chunk))
    img = np.zeros(size, dtype=np.uint8)
    for _, n, qo, so in chunk_table(total, chunk):
        img[qo: so] = codes_to_bytes(rng.choice(np.asarray(list(codes), dtype=np.uint8), (n // 32, 32))).reshape(-1)
        img[so: so + n // 32] = rng.choice(np.asarray(list(scales), dtype=np.uint8), n // 32)
    assert so + n // 32 == size
    return img


def int_x(m, k, seed):
    """Integers in [-8, 8] as (bf16 tensor [m, k], float64 array)."""
    v = np.random.default_rng(seed).integers(-8, 9, (m, k)).astype(np.float32)
    return torch.from_numpy(v).to(torch.bfloat16), v.astype(np.float64)


def bf16_tensor_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def prove_exact_ints(xf, wf):
    """x holds integers in [-8, 8], W multiples of 2^-4 of magnitude at most 15: every product is
    a multiple of 2^-4 and |sum| <= 1056 * 8 * 15 = 126 720 < 2^24 * 2^-4, so the f32 result is exact
    in any order and equals the float64 matmul. Asserted on the reference alone."""
    assert np.array_equal(xf, np.rint(xf)) and np.abs(xf).max() <= 8
    assert np.array_equal(wf * 16, np.rint(wf * 16)) and np.abs(wf).max() <= 15
    assert (np.abs(xf) @ np.abs(wf).T).max() < 2.0 ** 24 * 2.0 ** -4


def test_the_reference_reads_the_layout_of_the_host_codec():
    """chunk_table / block_index against core/mxfp6.cc: the whole layer and single blocks, full
    chunks and a tail chunk of 3 blocks."""
    chunk, total = 1024, 512 * 3 + 96
    img = handmade_image(total, chunk, 3, scales=range(255))
    whole = ref_layer_bits(img, total, chunk)
    assert np.array_equal(np.frombuffer(_core.mxfp6_unpack_layer_host(img.tobytes(), 2 * total, chunk), np.uint16), whole)
    for e in (0, 480, 512, 1024 + 31, 1536, total - 32, total - 1):
        qi, si = block_index(total, chunk, e)
        assert np.array_equal(ref_unpack(img[qi], img[si: si + 1]), whole[e // 32 * 32: e // 32 * 32 + 32])
    assert block_index(total, chunk, 1536)[1] == 3 * 400 + 3 * 24  # the tail chunk on its own length


# ---------------------------------------------------------------- the CPU route of the linear

@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("chunk,off,m,n,k", [(1024, 32 * 7, 5, 48, 96), (64 * KiB, 32 * 7, 17, 16, 160),
                                             (4096, 0, 1, 16, 32), (1024, 32 * 3, 3, 32, 1056)])
def test_cpu_linear_equals_linear_on_the_dequantized_weight(chunk, off, m, n, k, out_dtype):
    total = off + n * k
    img = handmade_image(total, chunk, 5, scales=range(100, 150))
    p = torch.from_numpy(img)
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    w = ops.mxfp6_unpack_range(p, 2 * total, chunk, off, n * k).view(n, k)
    assert np.array_equal(bf16_tensor_bits(w), ref_layer_bits(img, total, chunk)[off: off + n * k])
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk, elem_offset=off, out_dtype=out_dtype)
    y = ops.mxfp6_linear(x, p, n, k, **kw)
    want = F.linear(x, w) if out_dtype == torch.bfloat16 else F.linear(x.float(), w.float())
    assert y.dtype == out_dtype and y.shape == (m, n)
    assert torch.equal(y, want)
    y3 = ops.mxfp6_linear(x.view(1, m, k), p, n, k, **kw)
    assert y3.shape == (1, m, n) and torch.equal(y3[0], want)  # leading dimensions are kept


def test_cpu_linear_is_exact_on_integers():
    chunk, off, m, n, k = 1024, 32 * 7, 5, 48, 1056
    total = off + n * k
    img = handmade_image(total, chunk, 5)
    x, xf = int_x(m, k, 6)
    wf = ref_weight(img, total, chunk, off, n, k)
    prove_exact_ints(xf, wf)
    y = ops.mxfp6_linear(x, torch.from_numpy(img), n, k, src_bytes=2 * total, chunk_bytes=chunk, elem_offset=off,
                         out_dtype=torch.float32)
    assert np.array_equal(y.numpy().astype(np.float64), xf @ wf.T)


def test_linear_rejects_bad_arguments():
    chunk = 4096
    total = 32 * 7 + 48 * 96 + 32 * 3
    last = total - 48 * 96  # the last offset at which the parameter fits
    p = torch.from_numpy(handmade_image(total, chunk, 1))
    x = torch.zeros(5, 96, dtype=torch.bfloat16)
    ok = dict(src_bytes=2 * total, chunk_bytes=chunk, elem_offset=32 * 7)
    ops.mxfp6_linear(x, p, 48, 96, **ok)
    ops.mxfp6_linear(x, p, 48, 96, **{**ok, "elem_offset": last})
    bad = [
        ((x.float(), p, 48, 96), ok),                                  # activations must be bf16
        ((x, p.view(torch.int8), 48, 96), ok),                         # packed must be uint8
        ((x, p.view(2, -1), 48, 96), ok),                              # ... and 1-D
        ((x, p, 40, 96), ok),                                          # out_features % 16
        ((x[:, :80], p, 48, 80), ok),                                  # in_features % 32
        ((x[:, :64], p, 48, 96), ok),                                  # x's last dimension
        ((x[:0], p, 48, 96), ok),                                      # no rows
        ((x, p, 48, 96), {**ok, "elem_offset": 32 * 7 + 16}),          # offset off the 32-element grid
        ((x, p, 48, 96), {**ok, "elem_offset": -32}),
        ((x, p, 48, 96), {**ok, "elem_offset": last + 32}),            # runs past the layer
        ((x, p, 64, 96), ok),                                          # runs past the layer
        ((x, p, 48, 96), {**ok, "chunk_bytes": 512}),                  # chunk % 1024
        ((x, p, 48, 96), {**ok, "chunk_bytes": 1000}),
        ((x, p, 48, 96), {**ok, "chunk_bytes": 4096 + 256}),
        ((x, p, 48, 96), {**ok, "chunk_bytes": 0}),
        ((x, p, 48, 96), {**ok, "src_bytes": 2 * total + 32}),         # layer % 64
        ((x, p[:-1], 48, 96), ok),                                     # image shorter than the layout
        ((x, p, 48, 96), {**ok, "out_dtype": torch.float16}),
        ((x, p, 48, 96), {**ok, "split_k": 17}),
        ((x, p, 48, 96), {**ok, "split_k": -1}),
        ((x, p, 48, 96), {**ok, "row_tiles": 3}),
        ((x, p, 48, 96), {**ok, "row_tiles": 2}),                      # 3 tiles: 2 does not divide them
        ((x, p, 48, 96), {**ok, "out": torch.empty(5, 48, dtype=torch.bfloat16)}),  # out is for the GPU
    ]
    assert p.numel() % 2 == 0  # so that the 2-D view above exists and fails for its shape
    for args, kw in bad:
        with pytest.raises(ValueError):
            ops.mxfp6_linear(*args, **kw)
    # the packed-image checks are mxfp6_unpack_range's, word for word
    for kw in [{**ok, "chunk_bytes": 1000}, {**ok, "src_bytes": 2 * total + 32}]:
        with pytest.raises(ValueError) as a:
            ops.mxfp6_linear(x, p, 48, 96, **kw)
        with pytest.raises(ValueError) as b:
            ops.mxfp6_unpack_range(p, kw["src_bytes"], kw["chunk_bytes"], 0, 32)
        assert str(a.value) == str(b.value)
    with pytest.raises(ValueError) as a:
        ops.mxfp6_linear(x, p[:-1], 48, 96, **ok)
    with pytest.raises(ValueError) as b:
        ops.mxfp6_unpack_range(p[:-1], 2 * total, chunk, 0, 32)
    assert str(a.value) == str(b.value) and "the layout needs" in str(a.value)


# ---------------------------------------------------------------- packed parameters in decoder_forward

def _counted(monkeypatch, calls, name):
    real = getattr(ops, name)

    def counting(*a, **kw):
        calls[name] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, name, counting)


def test_forward_on_a_mix_of_tensors_mxfp6_fp8_and_mxfp4_params(monkeypatch):
    """Every projection takes the route of its own format: the result is the pass on each
    parameter's own dequantized tensor, bit for bit, with 3 mxfp6_linear, 2 fp8_linear and 2
    mxfp4_linear calls (on the CPU q, k and v are never merged) and no fused MXFP4 SwiGLU on a gate
    and an up of different formats."""
    blob = flatten(random_layer(SPEC, 21), SPEC)
    raw, chunk = blob.numpy().tobytes(), 64 * KiB

    def image(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8)

    p6 = unflatten_packed(image(_core.mxfp6_pack_layer_host(raw, chunk)), SPEC, chunk, "mxfp6")
    p8 = unflatten_packed(image(_core.fp8_pack_layer_host(raw, chunk, 128)), SPEC, chunk, "fp8", 128)
    p4 = unflatten_packed(image(_core.mxfp4_pack_layer_host(raw, chunk)), SPEC, chunk)
    mix = dict(unflatten(blob, SPEC))  # post_attention_layernorm stays a bf16 tensor
    mix.update({k: p6[k] for k in ("input_layernorm", "q_proj", "o_proj", "gate_proj")})
    mix.update({k: p8[k] for k in ("v_proj", "up_proj")})
    mix.update({k: p4[k] for k in ("k_proj", "down_proj")})
    assert {k: v.fmt for k, v in mix.items() if isinstance(v, PackedParam)} == {
        "input_layernorm": "mxfp6", "q_proj": "mxfp6", "o_proj": "mxfp6", "gate_proj": "mxfp6", "v_proj": "fp8",
        "up_proj": "fp8", "k_proj": "mxfp4", "down_proj": "mxfp4"}
    dense = {k: (v.dequantize() if isinstance(v, PackedParam) else v) for k, v in mix.items()}
    calls = {"mxfp6_linear": 0, "fp8_linear": 0, "mxfp4_linear": 0}
    for name in calls:
        _counted(monkeypatch, calls, name)
    monkeypatch.setattr(ops, "mxfp4_swiglu", lambda *a, **k: pytest.fail("gate and up have different formats"))
    x = torch.randn(1, 16, SPEC.hidden, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    want = decoder_forward(x, dense, SPEC)
    assert calls == {"mxfp6_linear": 0, "fp8_linear": 0, "mxfp4_linear": 0}
    for fuse in (True, False):
        for name in calls:
            calls[name] = 0
        assert torch.equal(decoder_forward(x, mix, SPEC, fuse=fuse), want)
        assert calls == {"mxfp6_linear": 3, "fp8_linear": 2, "mxfp4_linear": 2}


def test_forward_on_mxfp6_params_calls_the_linear_per_projection(monkeypatch):
    """A layer that is MXFP6 throughout, on the CPU: 7 mxfp6_linear calls (q, k, v, o, gate, up,
    down), the norm weights dequantized, and the bits of the pass on the dequantized tensors."""
    blob = flatten(random_layer(SPEC, 22), SPEC)
    chunk = 64 * KiB
    pp = unflatten_packed(torch.frombuffer(bytearray(_core.mxfp6_pack_layer_host(blob.numpy().tobytes(), chunk)),
                                           dtype=torch.uint8), SPEC, chunk, "mxfp6")
    calls = {"mxfp6_linear": 0}
    _counted(monkeypatch, calls, "mxfp6_linear")
    x = torch.randn(2, 8, SPEC.hidden, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16)
    y = decoder_forward(x, pp, SPEC)
    assert calls["mxfp6_linear"] == 7
    assert torch.equal(y, decoder_forward(x, {k: v.dequantize() for k, v in pp.items()}, SPEC))
