"""Consumers of an fp8-packed layer in place, on the CPU: the element-range unpack (core/fp8.cc
unpack_range_host, ops.fp8_unpack_range), the CPU route of ops.fp8_linear, fp8 PackedParams in
decoder_forward and Runtime.packed_layer_params.

The reference is numpy and independent of the code under test: ref_unpack of test_fp8_host.py
applied to every chunk of the layer ([codes][f32 scales] per source chunk, the tail chunk on its
own length), sliced to the element range, then a float64 matmul. The gfx950 kernel is checked
against the same reference in test_gpu_fp8_linear.py."""
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.catalog import make_workload
from distributed_llm_dissemination_amd.models.weights import (PRESETS, PackedParam, decoder_forward, flatten,
                                                             layer_nbytes, layer_params, random_layer, unflatten,
                                                             unflatten_packed)
from distributed_llm_dissemination_amd.parallel.runtime import Runtime

from test_fp8_host import BLOCKS, assert_bf16_equal, ref_unpack

KiB = 1 << 10
SPEC = PRESETS["tiny"]


# ---------------------------------------------------------------- the reference

def chunk_table(total, chunk, block):
    """[(first element, elements, offset of the codes, offset of the scales)] per source chunk."""
    ce = chunk // 2
    pc = ce + ce // block * 4
    return [(e0, min(ce, total - e0), c * pc, c * pc + min(ce, total - e0)) for c, e0 in enumerate(range(0, total, ce))]


def ref_layer_bits(packed, total, chunk, block):
    """bf16 bit patterns of all `total` elements of a packed layer image (uint8 array)."""
    return np.concatenate([ref_unpack(packed[qo: qo + n], packed[so: so + 4 * (n // block)].copy().view(np.float32), block)
                           for _, n, qo, so in chunk_table(total, chunk, block)])


def bits_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def ref_weight(packed, total, chunk, block, off, n, k):
    """The [n, k] parameter at element `off` of the layer, float64."""
    return bits_to_f64(ref_layer_bits(packed, total, chunk, block)[off: off + n * k]).reshape(n, k)


def code_index(total, chunk, block, elem):
    """Index in the packed image of element `elem`'s code."""
    for e0, n, qo, _ in chunk_table(total, chunk, block):
        if e0 <= elem < e0 + n:
            return qo + (elem - e0)
    raise IndexError(elem)


# +-{0x38 .. 0x57}: magnitudes 1 .. 15 with 3 fraction bits (multiples of 1/8), and +-0
EXACT_CODES = np.array([s | c for s in (0, 0x80) for c in [0] + list(range(0x38, 0x58))], dtype=np.uint8)


def handmade_image(total, chunk, block, seed, codes=EXACT_CODES, exps=(-1, 0, 1)):
    """A packed image of `total` elements (a multiple of `block`) built by hand: random codes
    from `codes`, every block with its own random scale 2^e, e from `exps`."""
    assert total % block == 0 and chunk % (2 * block) == 0
    rng = np.random.default_rng(seed)
    size = int(_core.fp8_packed_size(2 * total, chunk, block))
    img = np.zeros(size, dtype=np.uint8)
    for _, n, qo, so in chunk_table(total, chunk, block):
        img[qo: qo + n] = rng.choice(np.asarray(codes, dtype=np.uint8), n)
        img[so: so + 4 * (n // block)] = np.ldexp(1.0, rng.choice(np.asarray(exps), n // block)).astype(np.float32).view(np.uint8)
    assert so + 4 * (n // block) == size
    return img


def padded(elems, block):
    """`elems` rounded up to a whole number of scale blocks."""
    return -(-elems // block) * block


def int_x(m, k, seed):
    """Integers in [-8, 8] as (bf16 tensor [m, k], float64 array)."""
    v = np.random.default_rng(seed).integers(-8, 9, (m, k)).astype(np.float32)
    return torch.from_numpy(v).to(torch.bfloat16), v.astype(np.float64)


def bf16_tensor_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


# ---------------------------------------------------------------- element ranges

# 3 full chunks of 2048 elements at 4096 B and a short tail chunk of 512 (one block of 512)
CHUNK = 4096
TOTAL = 2048 * 3 + 512
RANGES = [(0, TOTAL), (0, 64), (32 * 7, 96 * 4), (2048 + 2016, 128), (32 * 5, 2048 * 2 + 64), (2048 * 3 - 32, 64),
          (2048 * 3 + 32, 96), (TOTAL - 32, 32), (64, 0)]


@pytest.fixture(scope="module")
def images():
    """Per block: (packed image over every code, NaN codes included, and scales 2^-20 .. 2^20,
    reference bits of the whole layer)."""
    out = {}
    for block in BLOCKS:
        img = handmade_image(TOTAL, CHUNK, block, 3 + block, codes=np.arange(256), exps=np.arange(-20, 21))
        out[block] = (img, ref_layer_bits(img, TOTAL, CHUNK, block))
    return out


@pytest.mark.parametrize("block", BLOCKS)
def test_unpack_range_matches_reference_slice(images, block):
    img, whole = images[block]
    assert_bf16_equal(np.frombuffer(_core.fp8_unpack_layer_host(img.tobytes(), 2 * TOTAL, CHUNK, block), np.uint16), whole)
    p = torch.from_numpy(img)
    for off, n in RANGES:
        got = ops.fp8_unpack_range(p, 2 * TOTAL, CHUNK, off, n, block)
        assert got.dtype == torch.bfloat16 and got.shape == (n,)
        assert_bf16_equal(bf16_tensor_bits(got), whole[off: off + n])
    # the host function itself takes any offset and length inside the layer
    for off, n in [(7, 1), (2000, 100), (2047, 2050), (TOTAL - 33, 33), (TOTAL, 0)]:
        out = np.full(n + 1, 0xA5A5, dtype=np.uint16)
        _core.fp8_unpack_range_host(img.ctypes.data, img.size, 2 * TOTAL, CHUNK, block, off, n, out.ctypes.data)
        assert_bf16_equal(out[:n], whole[off: off + n])
        assert out[n] == 0xA5A5
    for off, n in [(TOTAL - 31, 32), (-1, 1), (TOTAL + 1, 0), (0, -1)]:
        with pytest.raises(RuntimeError, match="outside the layer"):
            _core.fp8_unpack_range_host(img.ctypes.data, img.size, 2 * TOTAL, CHUNK, block, off, n, 0)
    with pytest.raises(RuntimeError, match="smaller"):
        _core.fp8_unpack_range_host(img.ctypes.data, img.size - 1, 2 * TOTAL, CHUNK, block, 0, 32, 0)
    with pytest.raises(RuntimeError, match="block"):  # a layout fp8::check rejects
        _core.fp8_unpack_range_host(img.ctypes.data, img.size, 2 * TOTAL, CHUNK, 48, 0, 32, 0)


def test_unpack_range_in_a_64k_chunk(images):
    """One short chunk: the layer's only chunk is laid out on its own length."""
    block = 128
    img = handmade_image(TOTAL, 64 * KiB, block, 9, codes=np.arange(256), exps=np.arange(-20, 21))
    whole = ref_layer_bits(img, TOTAL, 64 * KiB, block)
    for off, n in RANGES:
        got = ops.fp8_unpack_range(torch.from_numpy(img), 2 * TOTAL, 64 * KiB, off, n, block)
        assert_bf16_equal(bf16_tensor_bits(got), whole[off: off + n])


def test_unpack_range_rejects_bad_arguments(images):
    p = torch.from_numpy(images[128][0])
    for kw in [dict(elem_offset=16, n=32), dict(elem_offset=0, n=48), dict(elem_offset=TOTAL - 32, n=64),
               dict(elem_offset=-32, n=32), dict(elem_offset=0, n=32, chunk_bytes=1536),
               dict(elem_offset=0, n=32, src_bytes=2 * TOTAL + 256), dict(elem_offset=0, n=32, src_bytes=2 * TOTAL + 64),
               dict(elem_offset=0, n=32, block=48)]:
        a = dict(src_bytes=2 * TOTAL, chunk_bytes=CHUNK, block=128)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.fp8_unpack_range(p, a["src_bytes"], a["chunk_bytes"], a["elem_offset"], a["n"], a["block"])
    with pytest.raises(ValueError, match="uint8"):
        ops.fp8_unpack_range(p.view(torch.int8), 2 * TOTAL, CHUNK, 0, 32)


# ---------------------------------------------------------------- the CPU route of the linear

@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("block,chunk,off,m,n,k", [(128, 4096, 32 * 7, 5, 48, 96), (32, 64 * KiB, 32 * 7, 17, 16, 160),
                                                    (512, 4096, 0, 1, 16, 32), (64, 512, 32 * 3, 3, 32, 1056)])
def test_cpu_linear_equals_linear_on_the_dequantized_weight(block, chunk, off, m, n, k, out_dtype):
    total = padded(off + n * k, block)
    img = handmade_image(total, chunk, block, 5, codes=np.arange(0x7F), exps=np.arange(-6, 3))
    p = torch.from_numpy(img)
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    w = ops.fp8_unpack_range(p, 2 * total, chunk, off, n * k, block).view(n, k)
    assert_bf16_equal(bf16_tensor_bits(w), ref_layer_bits(img, total, chunk, block)[off: off + n * k])
    y = ops.fp8_linear(x, p, n, k, src_bytes=2 * total, chunk_bytes=chunk, block=block, elem_offset=off,
                       out_dtype=out_dtype)
    want = F.linear(x, w) if out_dtype == torch.bfloat16 else F.linear(x.float(), w.float())
    assert y.dtype == out_dtype and y.shape == (m, n)
    assert torch.equal(y, want)
    y3 = ops.fp8_linear(x.view(1, m, k), p, n, k, src_bytes=2 * total, chunk_bytes=chunk, block=block, elem_offset=off,
                        out_dtype=out_dtype)
    assert y3.shape == (1, m, n) and torch.equal(y3[0], want)  # leading dimensions are kept


def test_cpu_linear_is_exact_on_integers():
    """x holds integers in [-8, 8] and W multiples of 2^-4 of magnitude at most 30: the f32
    result is exact in any summation order and equals the float64 reference."""
    block, chunk, off, m, n, k = 128, 4096, 32 * 7, 5, 48, 96
    total = padded(off + n * k, block)
    img = handmade_image(total, chunk, block, 5)
    x, xf = int_x(m, k, 6)
    y = ops.fp8_linear(x, torch.from_numpy(img), n, k, src_bytes=2 * total, chunk_bytes=chunk, block=block,
                       elem_offset=off, out_dtype=torch.float32)
    assert np.array_equal(y.numpy().astype(np.float64), xf @ ref_weight(img, total, chunk, block, off, n, k).T)


def test_linear_rejects_bad_arguments():
    block, chunk = 128, 4096
    total = padded(32 * 7 + 48 * 96, block)
    last = total - 48 * 96  # the last offset at which the parameter fits
    p = torch.from_numpy(handmade_image(total, chunk, block, 1))
    x = torch.zeros(5, 96, dtype=torch.bfloat16)
    ok = dict(src_bytes=2 * total, chunk_bytes=chunk, block=block, elem_offset=32 * 7)
    ops.fp8_linear(x, p, 48, 96, **ok)
    ops.fp8_linear(x, p, 48, 96, **{**ok, "elem_offset": last})
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
        ((x, p, 48, 96), {**ok, "block": 48}),                         # not a block size
        ((x, p, 48, 96), {**ok, "block": 16}),
        ((x, p, 48, 96), {**ok, "chunk_bytes": 512}),                  # chunk % (8 * block)
        ((x, p, 48, 96), {**ok, "chunk_bytes": 4096 + 256}),
        ((x, p, 48, 96), {**ok, "chunk_bytes": 0}),
        ((x, p, 48, 96), {**ok, "src_bytes": 2 * total + 64}),         # layer % (2 * block)
        ((x, p[:-1], 48, 96), ok),                                     # image shorter than the layout
        ((x, p, 48, 96), {**ok, "out_dtype": torch.float16}),
        ((x, p, 48, 96), {**ok, "split_k": 17}),
        ((x, p, 48, 96), {**ok, "split_k": -1}),
        ((x, p, 48, 96), {**ok, "row_tiles": 3}),
        ((x, p, 48, 96), {**ok, "row_tiles": 2}),                      # 3 tiles: 2 does not divide them
        ((x, p, 48, 96), {**ok, "out": torch.empty(5, 48, dtype=torch.bfloat16)}),  # out is for the GPU
    ]
    for args, kw in bad:
        with pytest.raises(ValueError):
            ops.fp8_linear(*args, **kw)


# ---------------------------------------------------------------- packed parameter views

@pytest.fixture(scope="module")
def tiny_layer():
    blob = flatten(random_layer(SPEC, 21), SPEC)
    return blob, blob.numpy().tobytes()


@pytest.mark.parametrize("block,chunk", [(128, 64 * KiB), (32, 4096), (512, 4096)])
def test_forward_on_fp8_params_equals_forward_on_their_dequantized_tensors(tiny_layer, block, chunk):
    size = layer_nbytes(SPEC)
    packed = _core.fp8_pack_layer_host(tiny_layer[1], chunk, block)
    want = unflatten(torch.frombuffer(bytearray(_core.fp8_unpack_layer_host(packed, size, chunk, block)),
                                      dtype=torch.uint8), SPEC)
    pt = torch.frombuffer(bytearray(packed), dtype=torch.uint8)
    pp = unflatten_packed(pt, SPEC, chunk, "fp8", block)
    assert list(pp) == [n for n, _ in layer_params(SPEC)]
    for name, shape in layer_params(SPEC):
        p = pp[name]
        assert isinstance(p, PackedParam) and p.shape == tuple(shape) and p.src_bytes == size
        assert (p.fmt, p.block, p.chunk_bytes) == ("fp8", block, chunk) and p.packed.data_ptr() == pt.data_ptr()
        assert torch.equal(p.dequantize().view(torch.int16), want[name].view(torch.int16)), name
    x = torch.randn(1, 16, SPEC.hidden, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    y0 = decoder_forward(x, want, SPEC)
    for fuse in (True, False):
        assert torch.equal(decoder_forward(x, pp, SPEC, fuse=fuse), y0)
    with pytest.raises(ValueError, match="packed image needs"):
        unflatten_packed(pt[:-1], SPEC, chunk, "fp8", block)
    with pytest.raises(ValueError):
        unflatten_packed(pt, SPEC, chunk, "fp8", 48)
    with pytest.raises(ValueError):
        unflatten_packed(pt, SPEC, chunk, "fp6", block)


def test_forward_on_a_mix_of_tensors_fp8_and_mxfp4_params(tiny_layer, monkeypatch):
    """Every projection falls back to its own route: the result is the pass on each parameter's
    own dequantized tensor, no fused MXFP4 SwiGLU runs on a gate and an up of different formats."""
    size, chunk = layer_nbytes(SPEC), 64 * KiB
    p8 = unflatten_packed(torch.frombuffer(bytearray(_core.fp8_pack_layer_host(tiny_layer[1], chunk, 128)), dtype=torch.uint8),
                          SPEC, chunk, "fp8", 128)
    p4 = unflatten_packed(torch.frombuffer(bytearray(_core.mxfp4_pack_layer_host(tiny_layer[1], chunk)), dtype=torch.uint8),
                          SPEC, chunk)
    assert p4["q_proj"].fmt == "mxfp4" and p4["q_proj"].block == 32  # the defaults keep their meaning
    plain = unflatten(tiny_layer[0], SPEC)
    mix = dict(plain)
    mix.update({k: p8[k] for k in ("q_proj", "v_proj", "gate_proj", "post_attention_layernorm")})
    mix.update({k: p4[k] for k in ("k_proj", "up_proj", "down_proj")})
    dense = {k: (v.dequantize() if isinstance(v, PackedParam) else v) for k, v in mix.items()}
    calls = {"fp8": 0, "mxfp4": 0}
    linear8, linear4 = ops.fp8_linear, ops.mxfp4_linear
    monkeypatch.setattr(ops, "fp8_linear", lambda *a, **k: (calls.__setitem__("fp8", calls["fp8"] + 1), linear8(*a, **k))[1])
    monkeypatch.setattr(ops, "mxfp4_linear", lambda *a, **k: (calls.__setitem__("mxfp4", calls["mxfp4"] + 1), linear4(*a, **k))[1])
    monkeypatch.setattr(ops, "mxfp4_swiglu", lambda *a, **k: pytest.fail("gate and up have different formats"))
    x = torch.randn(1, 16, SPEC.hidden, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    assert torch.equal(decoder_forward(x, mix, SPEC), decoder_forward(x, dense, SPEC))
    assert calls == {"fp8": 3, "mxfp4": 3}


# ---------------------------------------------------------------- a session

def _session(pack, store, block, key, ranks=3):
    n, L = ranks, SPEC.layers
    size = layer_nbytes(SPEC)
    blobs = {l: flatten(random_layer(SPEC, 100 + l), SPEC) for l in range(L)}
    cfg = make_workload(n, L, size, tier="host", seeding="random", chunk_bytes=64 * KiB)
    bar = threading.Barrier(n)
    rts = [Runtime(cfg, i, engine="sim", registry={i: "127.0.0.1:0"}, chunk_bytes=64 * KiB, sim_key=key,
                   barrier=bar.wait, pack=pack, store=store, pack_block=block, layer_source=lambda l, nb: blobs[l])
           for i in range(n)]
    reg = {i: r.transport.address() for i, r in enumerate(rts)}
    for r in rts:
        r.transport.set_registry(reg)
    res = [None] * n

    def go(i):
        res[i] = rts[i].run(1, timeout=60)

    ths = [threading.Thread(target=go, args=(i,)) for i in range(n)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(120)
    return cfg, rts, res


@pytest.mark.parametrize("pack,block", [("fp8", 128), ("fp8", 32), ("mxfp4", 32)])
def test_packed_layer_params_from_a_sim_session(pack, block):
    """3 ranks, 64 KiB chunks, --store packed: the packed views decode to unpacked_layer_bytes and
    the forward pass on them equals the pass on the dequantized parameters."""
    size = layer_nbytes(SPEC)
    cfg, rts, res = _session(pack, "packed", block, f"plp{pack}{block}")
    try:
        assert all(r is not None and r.ok for r in res), [r and r.error for r in res]
        x = torch.randn(1, 16, SPEC.hidden, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
        seen = 0
        for r in rts:
            for l in cfg.assignment[r.node_id]:
                pp = r.packed_layer_params(l, SPEC)
                assert all(isinstance(v, PackedParam) and not v.packed.is_cuda for v in pp.values())
                assert all((v.fmt, v.block, v.chunk_bytes, v.src_bytes) == (pack, block, 64 * KiB, size) for v in pp.values())
                assert pp["q_proj"].packed.numel() == r.slot_sizes[l]
                plain = unflatten(torch.frombuffer(bytearray(r.unpacked_layer_bytes(l)), dtype=torch.uint8), SPEC)
                assert all(torch.equal(pp[k].dequantize().view(torch.int16), plain[k].view(torch.int16)) for k in plain)
                assert torch.equal(decoder_forward(x, pp, SPEC), decoder_forward(x, plain, SPEC))
                seen += 1
        assert seen
    finally:
        for r in rts:
            r.close()


@pytest.mark.parametrize("pack,store", [("none", "packed"), ("fp8", "bf16"), ("mxfp4", "bf16")])
def test_packed_layer_params_need_a_packed_store(pack, store):
    size = layer_nbytes(SPEC)
    cfg = make_workload(1, 1, size, tier="host", seeding="random", chunk_bytes=64 * KiB)
    rt = Runtime(cfg, 0, engine="sim", registry={0: "127.0.0.1:0"}, chunk_bytes=64 * KiB, sim_key=f"plpn{pack}{store}",
                 pack=pack, store=store, layer_source=lambda l, nb: flatten(random_layer(SPEC, 1), SPEC))
    try:
        with pytest.raises(ValueError, match="--store packed"):
            rt.packed_layer_params(0, SPEC)
    finally:
        rt.close()
