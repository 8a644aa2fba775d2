"""The CPU side of the fused gated MLP from an MXFP6- or an fp8-packed layer: the CPU routes of
ops.mxfp6_swiglu and ops.fp8_swiglu against the same torch ops on the bits of *_unpack_range of
the two ranges, their argument checks, and decoder_forward's opt-in route (fuse_gated=True).
The gfx950 kernels are checked in test_gpu_mxfp6_swiglu.py and test_gpu_fp8_swiglu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.weights import (PRESETS, decoder_forward, flatten, random_layer,
                                                             unflatten_packed)

import test_fp8_linear_host as f8
import test_mxfp6_linear_host as m6

KiB = 1 << 10
SPEC = PRESETS["tiny"]


class Fmt:
    """One layer format: a handmade image, the range unpack and the fused op, with equal signatures."""

    def __init__(self, name, block):
        self.name, self.block = name, block

    def padded(self, elems):
        return -(-elems // self.block) * self.block

    def image(self, total, chunk, seed):
        if self.name == "fp8":
            return torch.from_numpy(f8.handmade_image(total, chunk, self.block, seed))
        return torch.from_numpy(m6.handmade_image(total, chunk, seed))

    def unpack(self, p, total, chunk, off, n):
        if self.name == "fp8":
            return ops.fp8_unpack_range(p, 2 * total, chunk, off, n, self.block)
        return ops.mxfp6_unpack_range(p, 2 * total, chunk, off, n)

    def swiglu(self, x, p, n, k, **kw):
        if self.name == "fp8":
            return ops.fp8_swiglu(x, p, n, k, block=self.block, **kw)
        return ops.mxfp6_swiglu(x, p, n, k, **kw)

    def pack_layer(self, raw, chunk):
        if self.name == "fp8":
            b = _core.fp8_pack_layer_host(raw, chunk, self.block)
        else:
            b = _core.mxfp6_pack_layer_host(raw, chunk)
        return unflatten_packed(torch.frombuffer(bytearray(b), dtype=torch.uint8), SPEC, chunk, self.name, self.block)


FMTS = {"mxfp6": Fmt("mxfp6", 32), "fp8 block 32": Fmt("fp8", 32), "fp8 block 128": Fmt("fp8", 128)}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("chunk", [1024, 64 * KiB])
@pytest.mark.parametrize("order", ["gate before up", "up before gate"])
@pytest.mark.parametrize("m,n,k", [(5, 48, 96), (17, 16, 160), (3, 32, 1056)])
def test_cpu_route_is_the_torch_op_sequence(fmt, chunk, order, m, n, k):
    """bf16: F.silu(F.linear(x, Wg)) * F.linear(x, Wu) in bf16 on the unpacked ranges - the ops of
    the unfused route, so every intermediate is rounded as there; f32: the same sequence in f32.
    The two parameters lie in either order with a gap of 64 elements between them."""
    f = FMTS[fmt]
    first, second = 32 * 7, 32 * 7 + n * k + 64
    gate, up = (first, second) if order == "gate before up" else (second, first)
    total = f.padded(second + n * k)
    img = f.image(total, chunk, 8)
    x = (torch.randn(m, k, generator=torch.Generator().manual_seed(1)) / 4).to(torch.bfloat16)
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk, gate_offset=gate, up_offset=up)
    wg = f.unpack(img, total, chunk, gate, n * k).view(n, k)
    wu = f.unpack(img, total, chunk, up, n * k).view(n, k)
    assert not torch.equal(wg, wu)
    y16 = f.swiglu(x, img, n, k, **kw)
    assert y16.dtype == torch.bfloat16 and y16.shape == (m, n)
    assert np.array_equal(_bits(y16), _bits(F.silu(F.linear(x, wg)) * F.linear(x, wu)))
    y32 = f.swiglu(x, img, n, k, out_dtype=torch.float32, **kw)
    assert y32.dtype == torch.float32 and y32.shape == (m, n)
    assert np.array_equal(_bits(y32), _bits(F.silu(F.linear(x.float(), wg.float())) * F.linear(x.float(), wu.float())))
    y3 = f.swiglu(x.view(1, m, k), img, n, k, **kw)
    assert y3.shape == (1, m, n) and np.array_equal(_bits(y3)[0], _bits(y16))  # leading dimensions are kept


@pytest.mark.parametrize("fmt", ["mxfp6", "fp8 block 128"])
def test_swiglu_rejects_bad_arguments(fmt):
    """ops.mxfp4_swiglu's list, with every offset fault applied to the gate and to the up offset."""
    f = FMTS[fmt]
    n, k, chunk = 48, 96, 1024
    gate, up = 32 * 7, 32 * 7 + n * k
    total = f.padded(up + n * k)
    end = total - n * k  # the last offset at which a parameter fits
    p = f.image(total, chunk, 1)
    x = torch.zeros(5, k, dtype=torch.bfloat16)
    ok = dict(src_bytes=2 * total, chunk_bytes=chunk, gate_offset=gate, up_offset=up)
    f.swiglu(x, p, n, k, **ok)
    f.swiglu(x, p, n, k, **{**ok, "up_offset": end})
    bad = [
        ((x.float(), p, 48, 96), ok, "x must be"),                                   # activations must be bf16
        ((x, p.view(torch.int8), 48, 96), ok, "uint8"),                              # packed must be uint8
        ((x, p, 40, 96), ok, "multiple of 16"),                                      # out_features % 16
        ((x[:, :80], p, 48, 80), ok, "multiple of 16"),                              # in_features % 32
        ((x[:, :64], p, 48, 96), ok, "x must be"),                                   # x's last dimension
        ((x[:0], p, 48, 96), ok, "x must be"),                                       # no rows
        ((x, p, 48, 96), {**ok, "gate_offset": gate + 16}, None),                    # offsets off the 32 grid
        ((x, p, 48, 96), {**ok, "up_offset": up + 16}, None),
        ((x, p, 48, 96), {**ok, "gate_offset": end + 32}, "outside"),                # run past the layer
        ((x, p, 48, 96), {**ok, "up_offset": end + 32}, "outside"),
        ((x, p, 48, 96), {**ok, "gate_offset": -32}, None),
        ((x, p, 48, 96), {**ok, "up_offset": -32}, None),
        ((x, p, 64, 96), {**ok, "gate_offset": 0}, "outside"),                       # up runs past the layer
        ((x, p, 64, 96), {**ok, "gate_offset": up, "up_offset": 0}, "outside"),      # gate runs past the layer
        ((x, p, 48, 96), {**ok, "chunk_bytes": 1536}, "chunk_bytes"),                # chunk % 1024
        ((x, p[:-1], 48, 96), ok, "the layout needs"),                               # image shorter than the layout
        ((x, p, 48, 96), {**ok, "out_dtype": torch.float16}, "out_dtype"),
        ((x, p, 48, 96), {**ok, "split_k": 17}, "split_k"),
        ((x, p, 48, 96), {**ok, "split_k": -1}, "split_k"),
        ((x, p, 48, 96), {**ok, "row_tiles": 3}, "row_tiles"),
        ((x, p, 48, 96), {**ok, "row_tiles": 4}, "row_tiles"),
        ((x, p, 48, 96), {**ok, "row_tiles": 2}, "row_tiles"),                       # 3 tiles are no multiple of 2
        ((x, p, 48, 96), {**ok, "out": torch.empty(5, 48, dtype=torch.bfloat16)}, "out is for GPU"),
        ((x.to("meta"), p, 48, 96), ok, "same device"),                              # device mismatch
    ]
    for args, kw, match in bad:
        with pytest.raises(ValueError, match=match):
            f.swiglu(*args, **kw)


def test_fp8_swiglu_rejects_a_bad_block():
    n, k, chunk = 48, 96, 1024
    total = 2 * n * k
    p = FMTS["fp8 block 128"].image(total, chunk, 1)
    x = torch.zeros(5, k, dtype=torch.bfloat16)
    ok = dict(src_bytes=2 * total, chunk_bytes=chunk, gate_offset=0, up_offset=n * k)
    ops.fp8_swiglu(x, p, n, k, **ok)  # block 128 is the default
    for block in (48, 16, 1024):
        with pytest.raises(ValueError, match="block must be one of"):
            ops.fp8_swiglu(x, p, n, k, block=block, **ok)
    with pytest.raises(ValueError, match="chunk_bytes"):  # 1024 is no multiple of 8 * 512
        ops.fp8_swiglu(x, p, n, k, block=512, **ok)


# ---------------------------------------------------------------- decoder_forward

LINEAR = {"mxfp6": "mxfp6_linear", "fp8": "fp8_linear", "mxfp4": "mxfp4_linear"}
SWIGLU = {"mxfp6": "mxfp6_swiglu", "fp8": "fp8_swiglu", "mxfp4": "mxfp4_swiglu"}


def _record(monkeypatch, log, name):
    real = getattr(ops, name)

    def recording(*a, **kw):
        log.append((name, kw.get("gate_offset"), kw.get("up_offset")))
        return real(*a, **kw)

    monkeypatch.setattr(ops, name, recording)


@pytest.fixture(scope="module")
def tiny():
    blob = flatten(random_layer(SPEC, 41), SPEC)
    x = torch.randn(1, 16, SPEC.hidden, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    return blob.numpy().tobytes(), x


@pytest.mark.parametrize("fmt", ["mxfp6", "fp8 block 128", "fp8 block 32"])
def test_forward_routes_on_the_cpu(tiny, monkeypatch, fmt):
    """A `tiny` layer of one format, 64 KiB chunks. Default: 7 linear calls and the fused op never
    called. fuse_gated=True: 5 linear calls and 1 swiglu call with the offsets of gate and up.
    fuse=False wins over fuse_gated. All give equal bits (on the CPU the ops are the same)."""
    f = FMTS[fmt]
    raw, x = tiny
    pp = f.pack_layer(raw, 64 * KiB)
    log = []
    _record(monkeypatch, log, LINEAR[f.name])
    _record(monkeypatch, log, SWIGLU[f.name])

    def names():
        return [e[0] for e in log]

    y0 = decoder_forward(x, pp, SPEC)
    assert names() == [LINEAR[f.name]] * 7
    del log[:]
    y1 = decoder_forward(x, pp, SPEC, fuse_gated=True)
    assert names().count(LINEAR[f.name]) == 5 and names().count(SWIGLU[f.name]) == 1
    assert [e for e in log if e[0] == SWIGLU[f.name]] == [(SWIGLU[f.name], pp["gate_proj"].elem_offset,
                                                           pp["up_proj"].elem_offset)]
    assert pp["gate_proj"].elem_offset != pp["up_proj"].elem_offset
    del log[:]
    y2 = decoder_forward(x, pp, SPEC, fuse=False, fuse_gated=True)
    assert names() == [LINEAR[f.name]] * 7
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)) and torch.equal(y0.view(torch.int16), y2.view(torch.int16))
    assert torch.equal(y0, decoder_forward(x, {k: v.dequantize() for k, v in pp.items()}, SPEC))


def test_gate_and_up_of_different_formats_are_never_fused(tiny, monkeypatch):
    raw, x = tiny
    p6, p8 = FMTS["mxfp6"].pack_layer(raw, 64 * KiB), FMTS["fp8 block 128"].pack_layer(raw, 64 * KiB)
    p8b = FMTS["fp8 block 32"].pack_layer(raw, 64 * KiB)
    for name in SWIGLU.values():
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("gate and up do not share a layer and a format"))
    for gate, up in [(p6, p8), (p8, p6), (p8, p8b)]:
        mix = {**p6, "gate_proj": gate["gate_proj"], "up_proj": up["up_proj"]}
        dense = {k: v.dequantize() for k, v in mix.items()}
        assert torch.equal(decoder_forward(x, mix, SPEC, fuse_gated=True), decoder_forward(x, dense, SPEC))
    # a gate that is a tensor, and parameters of unequal shapes
    mix = {**p6, "gate_proj": p6["gate_proj"].dequantize()}
    assert torch.equal(decoder_forward(x, mix, SPEC, fuse_gated=True),
                       decoder_forward(x, {k: v.dequantize() for k, v in p6.items()}, SPEC))


def test_mxfp4_params_behave_the_same_with_and_without_fuse_gated(tiny, monkeypatch):
    raw, x = tiny
    pp = unflatten_packed(torch.frombuffer(bytearray(_core.mxfp4_pack_layer_host(raw, 64 * KiB)), dtype=torch.uint8),
                          SPEC, 64 * KiB)
    log = []
    _record(monkeypatch, log, "mxfp4_linear")
    _record(monkeypatch, log, "mxfp4_swiglu")
    runs = {}
    for fuse in (True, False):
        for fuse_gated in (False, True):
            del log[:]
            y = decoder_forward(x, pp, SPEC, fuse=fuse, fuse_gated=fuse_gated)
            runs[fuse, fuse_gated] = (list(log), y)
    for fuse in (True, False):
        assert runs[fuse, False][0] == runs[fuse, True][0]
        assert torch.equal(runs[fuse, False][1].view(torch.int16), runs[fuse, True][1].view(torch.int16))
    assert [e[0] for e in runs[True, True][0]].count("mxfp4_swiglu") == 1
    assert [e[0] for e in runs[False, True][0]] == ["mxfp4_linear"] * 7
