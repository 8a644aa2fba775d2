"""The CPU side of the fused gated MLP from an MXFP4-packed layer: the CPU route of
ops.mxfp4_swiglu against the same torch ops on mxfp4_unpack_range of the two ranges, its
argument checks, and decoder_forward's choice of routes (fuse=True / False, mixed dicts).
The gfx950 kernel is checked in test_gpu_mxfp4_swiglu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.weights import (PRESETS, decoder_forward, flatten, random_layer,
                                                             unflatten_packed)

from test_mxfp4_linear_host import bf16_tensor_bits, handmade_image

KiB = 1 << 10
SPEC = PRESETS["tiny"]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


@pytest.mark.parametrize("chunk", [1024, 64 * KiB])
@pytest.mark.parametrize("order", ["gate before up", "up before gate", "equal offsets"])
def test_cpu_route_is_the_torch_op_sequence(chunk, order):
    """bf16: F.silu(F.linear(x, Wg)) * F.linear(x, Wu) in bf16 - the ops a plain bf16 layer
    gets, so every intermediate is rounded as there; f32: the same sequence in f32."""
    m, n, k = 5, 48, 96
    gate, up = {"gate before up": (32 * 7, 32 * 9 + n * k), "up before gate": (32 * 3 + n * k, 32),
                "equal offsets": (32 * 5, 32 * 5)}[order]
    total = max(gate, up) + n * k  # with 1024-B chunks the later parameter ends in a short tail chunk
    img = torch.from_numpy(handmade_image(total, chunk, 8))
    x = (torch.randn(m, k, generator=torch.Generator().manual_seed(1)) / 4).to(torch.bfloat16)
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk)
    wg = ops.mxfp4_unpack_range(img, 2 * total, chunk, gate, n * k).view(n, k)
    wu = ops.mxfp4_unpack_range(img, 2 * total, chunk, up, n * k).view(n, k)
    y16 = ops.mxfp4_swiglu(x, img, n, k, gate_offset=gate, up_offset=up, **kw)
    assert y16.dtype == torch.bfloat16 and y16.shape == (m, n)
    assert np.array_equal(_bits(y16), _bits(F.silu(F.linear(x, wg)) * F.linear(x, wu)))
    y32 = ops.mxfp4_swiglu(x, img, n, k, gate_offset=gate, up_offset=up, out_dtype=torch.float32, **kw)
    assert y32.dtype == torch.float32 and y32.shape == (m, n)
    assert np.array_equal(_bits(y32), _bits(F.silu(F.linear(x.float(), wg.float())) * F.linear(x.float(), wu.float())))
    y3 = ops.mxfp4_swiglu(x.view(1, m, k), img, n, k, gate_offset=gate, up_offset=up, **kw)
    assert y3.shape == (1, m, n) and np.array_equal(_bits(y3)[0], _bits(y16))  # leading dimensions are kept


def test_swiglu_rejects_bad_arguments():
    """mxfp4_linear's list, with every offset fault applied to the gate and to the up offset."""
    n, k, chunk = 48, 96, 1024
    gate, up = 32 * 7, 32 * 7 + n * k
    total = up + n * k
    p = torch.from_numpy(handmade_image(total, chunk, 1))
    x = torch.zeros(5, k, dtype=torch.bfloat16)
    ok = dict(src_bytes=2 * total, chunk_bytes=chunk, gate_offset=gate, up_offset=up)
    ops.mxfp4_swiglu(x, p, n, k, **ok)
    bad = [
        ((x.float(), p, 48, 96), ok),                                  # activations must be bf16
        ((x, p.view(torch.int8), 48, 96), ok),                         # packed must be uint8
        ((x, p, 40, 96), ok),                                          # out_features % 16
        ((x[:, :80], p, 48, 80), ok),                                  # in_features % 32
        ((x[:, :64], p, 48, 96), ok),                                  # x's last dimension
        ((x[:0], p, 48, 96), ok),                                      # no rows
        ((x, p, 48, 96), {**ok, "gate_offset": gate + 16}),            # offsets off the block grid
        ((x, p, 48, 96), {**ok, "up_offset": up + 16}),
        ((x, p, 48, 96), {**ok, "gate_offset": up + 32}),              # run past the layer
        ((x, p, 48, 96), {**ok, "up_offset": up + 32}),
        ((x, p, 48, 96), {**ok, "gate_offset": -32}),
        ((x, p, 48, 96), {**ok, "up_offset": -32}),
        ((x, p, 64, 96), {**ok, "gate_offset": 0}),                    # up runs past the layer
        ((x, p, 64, 96), {**ok, "gate_offset": up, "up_offset": 0}),   # gate runs past the layer
        ((x, p, 48, 96), {**ok, "chunk_bytes": 1536}),                 # chunk % 1024
        ((x, p[:-1], 48, 96), ok),                                     # image shorter than the layout
        ((x, p, 48, 96), {**ok, "out_dtype": torch.float16}),
        ((x, p, 48, 96), {**ok, "split_k": 17}),
        ((x, p, 48, 96), {**ok, "row_tiles": 3}),
        ((x, p, 48, 96), {**ok, "row_tiles": 4}),
        ((x, p, 48, 96), {**ok, "row_tiles": 2}),                      # 3 tiles are no multiple of 2
        ((x, p, 48, 96), {**ok, "out": torch.empty(5, 48, dtype=torch.bfloat16)}),  # out is for the GPU
    ]
    for args, kw in bad:
        with pytest.raises(ValueError):
            ops.mxfp4_swiglu(*args, **kw)
    with pytest.raises(ValueError, match="row_tiles"):
        ops.mxfp4_swiglu(x, p, n, k, **{**ok, "row_tiles": 3})
    with pytest.raises(ValueError, match="out is for GPU"):
        ops.mxfp4_swiglu(x, p, n, k, **{**ok, "out": torch.empty(5, 48, dtype=torch.bfloat16)})


@pytest.fixture(scope="module")
def layer():
    """A `tiny` layer packed on the host (64 KiB chunks): its packed and its dequantized parameters."""
    blob = flatten(random_layer(SPEC, 33), SPEC)
    packed = torch.frombuffer(bytearray(_core.mxfp4_pack_layer_host(blob.numpy().tobytes(), 64 * KiB)), dtype=torch.uint8)
    pp = unflatten_packed(packed, SPEC, 64 * KiB)
    x = torch.randn(1, 16, SPEC.hidden, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    return pp, {k: v.dequantize() for k, v in pp.items()}, x


def test_forward_on_packed_equals_forward_on_dequantized(layer):
    """On the CPU both routes use the same values and the same torch ops: equal bits, fused
    or not, and with a dict that mixes tensors and PackedParams."""
    pp, plain, x = layer
    want = decoder_forward(x, plain, SPEC)
    assert np.array_equal(bf16_tensor_bits(decoder_forward(x, plain, SPEC, fuse=False)), bf16_tensor_bits(want))
    for fuse in (True, False):
        assert np.array_equal(bf16_tensor_bits(decoder_forward(x, pp, SPEC, fuse=fuse)), bf16_tensor_bits(want)), fuse
        for names in (["k_proj"], ["gate_proj"], ["up_proj", "q_proj"], ["input_layernorm", "down_proj"]):
            mixed = {**plain, **{n: pp[n] for n in names}}
            got = decoder_forward(x, mixed, SPEC, fuse=fuse)
            assert np.array_equal(bf16_tensor_bits(got), bf16_tensor_bits(want)), (fuse, names)


def test_forward_call_counts_on_the_cpu(layer, monkeypatch):
    """fuse=True on the CPU: gate and up are one mxfp4_swiglu; q, k and v stay three calls (one
    launch for them is a GPU route), with o and down 5 mxfp4_linear. fuse=False: 7 and 0."""
    pp, plain, x = layer
    calls = {"linear": 0, "swiglu": 0}
    linear, swiglu = ops.mxfp4_linear, ops.mxfp4_swiglu

    def count_linear(*a, **kw):
        calls["linear"] += 1
        return linear(*a, **kw)

    def count_swiglu(*a, **kw):
        calls["swiglu"] += 1
        return swiglu(*a, **kw)

    monkeypatch.setattr(ops, "mxfp4_linear", count_linear)
    monkeypatch.setattr(ops, "mxfp4_swiglu", count_swiglu)
    decoder_forward(x, pp, SPEC)
    assert calls == {"linear": 5, "swiglu": 1}
    calls.update(linear=0, swiglu=0)
    decoder_forward(x, pp, SPEC, fuse=False)
    assert calls == {"linear": 7, "swiglu": 0}
    calls.update(linear=0, swiglu=0)
    decoder_forward(x, {**pp, "up_proj": plain["up_proj"]}, SPEC)  # gate packed, up a tensor: per projection
    assert calls == {"linear": 6, "swiglu": 0}

