"""Decoder-layer weights as dissemination layers (the serving side of the service).

The engine moves a layer as opaque bytes (reference semantics: a layer is a
byte blob of ``LayerSize``). A model deployment wants those bytes back as the
layer's named parameters. This module fixes a byte layout for one decoder layer
of a Llama-family model - its parameters in a fixed order, each contiguous, the
blob padded to a 4 KiB multiple (so fp8 packing's whole scale blocks and the
chunk grid both fit) - and converts between the two:

    spec = PRESETS["llama3-70b"]
    blob = flatten(weights, spec)                 # host side: the layer's source bytes
    rt = Runtime(cfg, rank, ..., layer_source=lambda l, n: blobs[l])
    ...session...
    params = rt.layer_params(l, spec)             # named bf16 views of the layer in HBM (zero-copy)
    y = decoder_forward(x, params, spec)          # use them

With ``--pack mxfp4 --store packed`` the layer stays packed in HBM and is used
as it lies: ``rt.layer_params(l, spec, packed=True)`` gives a ``PackedParam`` per
name (views of the packed slot, no bf16 image anywhere) and ``decoder_forward``
runs the layer from the packed bytes in four weight launches: q, k and v, which
lie one behind the other in the blob, as one ``ops.mxfp4_linear`` of h + 2 kv rows
(on the GPU), ``o_proj``, the gate and up projections with ``silu(g) * u`` as one
``ops.mxfp4_swiglu``, and ``down_proj``. ``fuse=False`` runs one ``ops.mxfp4_linear``
per projection instead.

``--pack fp8 --store packed`` is served the same way: ``rt.packed_layer_params(l, spec)``
(which serves both formats) gives ``PackedParam``s with ``fmt="fp8"`` and the session's
scale block, and ``decoder_forward`` runs the layer from the e4m3 codes and block scales in
five weight launches: q/k/v as one ``ops.fp8_linear``, ``o_proj``, gate, up (``silu(g) * u`` is
plain torch) and ``down_proj``. ``decoder_forward(..., fuse_gated=True)`` opts in to the fused
``ops.fp8_swiglu`` for gate and up: four weight launches.

``--pack mxfp6 --store packed`` gives ``PackedParam``s with ``fmt="mxfp6"`` from the same
call, and ``decoder_forward`` runs the layer from the e2m3 blocks and E8M0 scale bytes in
five weight launches as well: q/k/v as one ``ops.mxfp6_linear``, ``o_proj``, gate, up and
``down_proj``, or in four with ``fuse_gated=True`` (``ops.mxfp6_swiglu``). Only the two norm
weights are dequantized.

Those launch counts hold per 64 rows of input: the kernels above are decode kernels. With
``decoder_forward(..., tiled=True)`` (opt-in) every packed projection, in any of the three
formats, runs on its format's many-row kernel instead (``tiled=True`` of the same op): four
weight launches for any batch * seq (fp8 and MXFP6: with ``fuse_gated=True``, else five), each
row of a projection a function of that row of its input alone.

``decoder_forward`` is a plain PyTorch reference of the layer (RMSNorm,
grouped-query attention with rotary embeddings, SwiGLU MLP) that the tests run
on received weights against the originals.

Generating a token does not re-run the prefix: ``decoder_step`` (opt-in) is one decode
step of the same layer against a ``KVCache`` in HBM.

    cache = KVCache.allocate(spec, batch, capacity, device="cuda")
    y = decoder_forward(x, params, spec, cache=cache)     # the prefill: also fills positions [0, seq)
    y1 = decoder_step(x1, params, spec, cache)            # x1 [batch, 1, hidden]: one more token each

The step runs the projections on the routes above (their 1 .. 16 row kernels), rotates q and
k at each sequence's position and appends k and v in one ``ops.rope_append`` launch, and
attends with ``ops.attn_decode``, which reads every K and V row once per KV head instead of
once per query head and whose result for a sequence has the same bits in any batch. The
lengths live on the device: a step has no host round trip.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import torch
import torch.nn.functional as F

ALIGN = 4096


@dataclass(frozen=True)
class DecoderSpec:
    name: str
    hidden: int
    intermediate: int
    heads: int
    kv_heads: int
    layers: int
    rope_theta: float = 500000.0
    eps: float = 1e-5

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads


PRESETS: Dict[str, DecoderSpec] = {
    "llama3-8b": DecoderSpec("llama3-8b", 4096, 14336, 32, 8, 32),
    "llama3-70b": DecoderSpec("llama3-70b", 8192, 28672, 64, 8, 80),
    "llama3.1-405b": DecoderSpec("llama3.1-405b", 16384, 53248, 128, 8, 126),
    "tiny": DecoderSpec("tiny", 256, 512, 4, 2, 4),
}


def layer_params(spec: DecoderSpec) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of one decoder layer's parameters, in blob order (torch Linear: [out, in])."""
    h, i, kv = spec.hidden, spec.intermediate, spec.kv_heads * spec.head_dim
    return [
        ("input_layernorm", (h,)),
        ("q_proj", (h, h)),
        ("k_proj", (kv, h)),
        ("v_proj", (kv, h)),
        ("o_proj", (h, h)),
        ("post_attention_layernorm", (h,)),
        ("gate_proj", (i, h)),
        ("up_proj", (i, h)),
        ("down_proj", (h, i)),
    ]


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= s
    return n


def layer_nbytes(spec: DecoderSpec, elem_bytes: int = 2) -> int:
    """Bytes of one layer's blob (bf16 parameters, padded to ALIGN)."""
    raw = sum(_numel(s) for _, s in layer_params(spec)) * elem_bytes
    return -(-raw // ALIGN) * ALIGN


def random_layer(spec: DecoderSpec, seed: int, dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    """Initialised like a real layer (norm weights 1 +- noise, projections ~N(0, 1/fan_in))."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in layer_params(spec):
        if len(shape) == 1:
            w = 1.0 + 0.02 * torch.randn(shape, generator=g)
        else:
            w = torch.randn(shape, generator=g) / shape[1] ** 0.5
        out[name] = w.to(dtype)
    return out


def flatten(weights: Dict[str, torch.Tensor], spec: DecoderSpec) -> torch.Tensor:
    """The layer's blob: a contiguous uint8 CPU tensor of layer_nbytes(spec) bytes."""
    blob = torch.zeros(layer_nbytes(spec), dtype=torch.uint8)
    off = 0
    for name, shape in layer_params(spec):
        w = weights[name]
        if tuple(w.shape) != shape or w.dtype != torch.bfloat16:
            raise ValueError(f"{name}: expected bf16 {shape}, got {w.dtype} {tuple(w.shape)}")
        n = w.numel() * 2
        blob[off:off + n] = w.detach().cpu().contiguous().view(-1).view(torch.uint8)
        off += n
    return blob


def unflatten(blob: torch.Tensor, spec: DecoderSpec) -> Dict[str, torch.Tensor]:
    """Named bf16 views of a layer blob (uint8 or bf16 tensor on any device; no copy)."""
    if blob.dtype != torch.uint8:
        blob = blob.view(torch.uint8)
    blob = blob.view(-1)
    if blob.numel() < layer_nbytes(spec):
        raise ValueError(f"blob holds {blob.numel()} B, the layer needs {layer_nbytes(spec)}")
    out = {}
    off = 0
    for name, shape in layer_params(spec):
        n = _numel(shape) * 2
        out[name] = blob[off:off + n].view(torch.bfloat16).view(shape)
        off += n
    return out


@dataclass(frozen=True)
class PackedParam:
    """One parameter of a layer that is held packed - `fmt` "mxfp4" (core/mxfp4.h),
    "mxfp6" (core/mxfp6.h) or "fp8" (core/fp8.h, one scale per `block` elements): elements [elem_offset,
    elem_offset + numel) of the layer of `src_bytes` bf16 bytes whose packed image, in
    chunks of `chunk_bytes`, is `packed`. A view: nothing is copied."""
    packed: torch.Tensor
    src_bytes: int
    chunk_bytes: int
    elem_offset: int
    shape: Tuple[int, ...]
    fmt: str = "mxfp4"
    block: int = 32

    @property
    def device(self) -> torch.device:
        return self.packed.device

    def dequantize(self) -> torch.Tensor:
        """The parameter as a bf16 tensor on the packed tensor's device."""
        from ..ops import fp8_unpack_range, mxfp4_unpack_range, mxfp6_unpack_range

        if self.fmt == "fp8":
            return fp8_unpack_range(self.packed, self.src_bytes, self.chunk_bytes, self.elem_offset,
                                    _numel(self.shape), self.block).view(self.shape)
        if self.fmt == "mxfp6":
            return mxfp6_unpack_range(self.packed, self.src_bytes, self.chunk_bytes, self.elem_offset,
                                      _numel(self.shape)).view(self.shape)
        return mxfp4_unpack_range(self.packed, self.src_bytes, self.chunk_bytes, self.elem_offset,
                                  _numel(self.shape)).view(self.shape)


Param = Union[torch.Tensor, PackedParam]


def unflatten_packed(packed: torch.Tensor, spec: DecoderSpec, chunk_bytes: int, fmt: str = "mxfp4",
                     block: int = 32) -> Dict[str, PackedParam]:
    """Named parameters of a packed layer blob (a uint8 tensor on any device, the image of
    layer_nbytes(spec) source bytes in chunks of `chunk_bytes`; no copy): MXFP4, with
    fmt="mxfp6" MXFP6 (block 32 as well), or with fmt="fp8" the fp8 format with one scale
    per `block` elements."""
    from ..ops import fp8_packed_size, mxfp4_packed_size, mxfp6_packed_size

    if packed.dtype != torch.uint8:
        raise ValueError("packed must be uint8")
    if fmt not in ("mxfp4", "mxfp6", "fp8"):
        raise ValueError(f"fmt must be 'mxfp4', 'mxfp6' or 'fp8', not {fmt!r}")
    packed = packed.view(-1)
    src = layer_nbytes(spec)
    if fmt == "fp8":
        if block not in (32, 64, 128, 256, 512):
            raise ValueError("an fp8 scale block is 32, 64, 128, 256 or 512 elements")
        if chunk_bytes <= 0 or chunk_bytes % (8 * block):
            raise ValueError(f"chunk_bytes must be a positive multiple of 8 * block ({8 * block})")
        need = fp8_packed_size(src, chunk_bytes, block)
    else:
        if block != 32:
            raise ValueError(f"{fmt.upper()} has a fixed scale block of 32 elements")
        if chunk_bytes <= 0 or chunk_bytes % 1024:
            raise ValueError("chunk_bytes must be a positive multiple of 1024")
        need = (mxfp6_packed_size if fmt == "mxfp6" else mxfp4_packed_size)(src, chunk_bytes)
    if packed.numel() < need:
        raise ValueError(f"packed holds {packed.numel()} B, the layer's packed image needs {need}")
    out = {}
    off = 0
    for name, shape in layer_params(spec):
        out[name] = PackedParam(packed, src, chunk_bytes, off, tuple(shape), fmt, block)
        off += _numel(shape)
    return out


def _check_act_fmt(w: "PackedParam", act: Optional[str]) -> None:
    if act is not None and w.fmt != "mxfp4":
        raise ValueError(f"act={act!r} runs MXFP4-packed projections only, this one is packed as {w.fmt}")


def _linear(x: torch.Tensor, w: Param, tiled: bool = False, act: Optional[str] = None) -> torch.Tensor:
    """x @ w.T: from the packed bytes for a PackedParam (ops.mxfp4_linear, ops.mxfp6_linear
    or ops.fp8_linear by its format), F.linear for a tensor. `tiled`: the many-row kernel
    of a PackedParam's format (tiled=True of the same op); a tensor has none. `act`: the
    op's act= for an MXFP4 PackedParam, a ValueError for another format, nothing for a
    tensor."""
    if isinstance(w, PackedParam):
        from ..ops import fp8_linear, mxfp4_linear, mxfp6_linear

        _check_act_fmt(w, act)
        # `tiled` and `act` are passed only when set: without them the call is what it always was
        kw = {"tiled": True} if tiled else {}
        if act is not None:
            kw["act"] = act
        if w.fmt == "mxfp6":
            return mxfp6_linear(x, w.packed, w.shape[0], w.shape[1], src_bytes=w.src_bytes,
                                chunk_bytes=w.chunk_bytes, elem_offset=w.elem_offset, out_dtype=x.dtype, **kw)
        if w.fmt == "fp8":
            return fp8_linear(x, w.packed, w.shape[0], w.shape[1], src_bytes=w.src_bytes, chunk_bytes=w.chunk_bytes,
                              block=w.block, elem_offset=w.elem_offset, out_dtype=x.dtype, **kw)
        return mxfp4_linear(x, w.packed, w.shape[0], w.shape[1], src_bytes=w.src_bytes, chunk_bytes=w.chunk_bytes,
                            elem_offset=w.elem_offset, out_dtype=x.dtype, **kw)
    return F.linear(x, w)


def _dense(w: Param) -> torch.Tensor:
    return w.dequantize() if isinstance(w, PackedParam) else w


def _rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()).to(x.dtype)


def _rope(x: torch.Tensor, theta: float) -> torch.Tensor:
    """Rotary embedding over [batch, heads, seq, head_dim] (rotate-half convention)."""
    d = x.shape[-1]
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, device=x.device, dtype=torch.float32) / d))
    pos = torch.arange(x.shape[-2], device=x.device, dtype=torch.float32)
    ang = torch.outer(pos, inv)
    cos, sin = torch.cat([ang, ang], -1).cos(), torch.cat([ang, ang], -1).sin()
    x1, x2 = x.float()[..., : d // 2], x.float()[..., d // 2:]
    return (x.float() * cos + torch.cat([-x2, x1], -1) * sin).to(x.dtype)


def _same_layer(*ws: Param) -> bool:
    """All PackedParams over the same packed bytes with one format and layout."""
    if not all(isinstance(w, PackedParam) for w in ws):
        return False
    p0 = ws[0].packed
    return all(w.packed.device == p0.device and w.packed.data_ptr() == p0.data_ptr() and w.packed.numel() == p0.numel()
               and w.src_bytes == ws[0].src_bytes and w.chunk_bytes == ws[0].chunk_bytes
               and w.fmt == ws[0].fmt and w.block == ws[0].block for w in ws[1:])


def _qkv(h: torch.Tensor, p: Dict[str, Param], fuse: bool, tiled: bool = False, act: Optional[str] = None):
    """q, k and v of h. On the GPU, three PackedParams of one layer that lie one behind
    the other with equal in_features are one [h + 2 kv, h] weight and take one launch;
    the result is split by views. On the CPU (and for anything else) one call each."""
    wq, wk, wv = p["q_proj"], p["k_proj"], p["v_proj"]
    if (fuse and h.is_cuda and _same_layer(wq, wk, wv) and wq.shape[1] == wk.shape[1] == wv.shape[1]
            and wk.elem_offset == wq.elem_offset + _numel(wq.shape)
            and wv.elem_offset == wk.elem_offset + _numel(wk.shape)):
        nq, nk, nv = wq.shape[0], wk.shape[0], wv.shape[0]
        y = _linear(h, PackedParam(wq.packed, wq.src_bytes, wq.chunk_bytes, wq.elem_offset, (nq + nk + nv, wq.shape[1]),
                                   wq.fmt, wq.block), tiled, act)
        return y[..., :nq], y[..., nq:nq + nk], y[..., nq + nk:]
    return _linear(h, wq, tiled, act), _linear(h, wk, tiled, act), _linear(h, wv, tiled, act)


def _gated(h: torch.Tensor, wg: Param, wu: Param, fuse: bool, fuse_gated: bool = False,
           tiled: bool = False, act: Optional[str] = None) -> torch.Tensor:
    """silu(h @ wg.T) * (h @ wu.T): one ops.mxfp4_swiglu for two MXFP4 PackedParams of
    one layer with equal shapes (on the CPU the very ops of the other route). Two fp8 or
    two MXFP6 PackedParams take one ops.fp8_swiglu / ops.mxfp6_swiglu only with
    `fuse_gated` as well (opt-in) and otherwise one linear each, as does anything else.
    `tiled` goes to whichever call is made: the fused op's tiled=True, or `_linear`'s - two
    tiled linears and the torch epilogue for fp8 and MXFP6 without `fuse_gated`. `act`
    goes the same way (MXFP4 only; another packed format raises ValueError)."""
    if fuse and _same_layer(wg, wu) and wg.shape == wu.shape:
        from ..ops import fp8_swiglu, mxfp4_swiglu, mxfp6_swiglu

        _check_act_fmt(wg, act)
        kw = dict(src_bytes=wg.src_bytes, chunk_bytes=wg.chunk_bytes, gate_offset=wg.elem_offset,
                  up_offset=wu.elem_offset, out_dtype=h.dtype, **({"tiled": True} if tiled else {}))
        if act is not None:
            kw["act"] = act
        if wg.fmt == "mxfp4":
            return mxfp4_swiglu(h, wg.packed, wg.shape[0], wg.shape[1], **kw)
        if fuse_gated and wg.fmt == "mxfp6":
            return mxfp6_swiglu(h, wg.packed, wg.shape[0], wg.shape[1], **kw)
        if fuse_gated and wg.fmt == "fp8":
            return fp8_swiglu(h, wg.packed, wg.shape[0], wg.shape[1], block=wg.block, **kw)
    return F.silu(_linear(h, wg, tiled, act)) * _linear(h, wu, tiled, act)


def _rope_tables(capacity: int, d: int, theta: float, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos and sin [capacity, d] of `_rope` for positions 0 .. capacity - 1: the same
    expressions on the same device, so row t holds the bits `_rope` uses at position t."""
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, device=device, dtype=torch.float32) / d))
    pos = torch.arange(capacity, device=device, dtype=torch.float32)
    ang = torch.outer(pos, inv)
    return torch.cat([ang, ang], -1).cos(), torch.cat([ang, ang], -1).sin()


@dataclass
class KVCache:
    """One layer's KV cache for `decoder_step`: `k` and `v` bf16 [batch, kv_heads,
    capacity, head_dim] (k rotated), `lens` int32 [batch] on their device - positions
    [0, lens[b]) of sequence b are valid, whatever lies behind is never read - the
    rotary tables `cos`, `sin` f32 [capacity, head_dim], and `max_len`, a host upper
    bound of `lens` that sizes the attention's grid without a device round trip."""
    k: torch.Tensor
    v: torch.Tensor
    lens: torch.Tensor
    cos: torch.Tensor
    sin: torch.Tensor
    capacity: int
    max_len: int = 0

    @classmethod
    def allocate(cls, spec: DecoderSpec, batch: int, capacity: int, device="cpu",
                 lens: Optional[torch.Tensor] = None) -> "KVCache":
        """An empty cache: K and V uninitialised, lengths zero. `lens` (int32 [batch] on
        `device`) lets the layers of a model share one length tensor."""
        if batch < 1 or capacity < 1:
            raise ValueError("batch and capacity must be positive")
        device = torch.device(device)
        if lens is None:
            lens = torch.zeros(batch, dtype=torch.int32, device=device)
        elif lens.dtype != torch.int32 or tuple(lens.shape) != (batch,) or lens.device.type != device.type:
            raise ValueError(f"lens must be an int32 [{batch}] tensor on {device}")
        shape = (batch, spec.kv_heads, capacity, spec.head_dim)
        cos, sin = _rope_tables(capacity, spec.head_dim, spec.rope_theta, device)
        return cls(torch.empty(shape, dtype=torch.bfloat16, device=device),
                   torch.empty(shape, dtype=torch.bfloat16, device=device), lens, cos, sin, capacity, 0)


def decoder_forward(x: torch.Tensor, p: Dict[str, Param], spec: DecoderSpec, fuse: bool = True,
                    fuse_gated: bool = False, tiled: bool = False, act: Optional[str] = None,
                    cache: Optional[KVCache] = None) -> torch.Tensor:
    """One decoder layer on x [batch, seq, hidden] (causal self-attention; with `cache`
    the prefill of a KV cache, see the end).
    Each parameter is a bf16 tensor or a PackedParam: a packed linear runs from its
    packed bytes (ops.mxfp4_linear, ops.mxfp6_linear or ops.fp8_linear), a packed norm
    weight is dequantized once. With `fuse`, MXFP4 gate and up projections run as one
    ops.mxfp4_swiglu and, on the GPU, packed q, k and v of any one format as one linear;
    parameters that do not allow it (a mix of tensors and PackedParams or of formats,
    other layouts) fall back per projection. With `fuse` and `fuse_gated`, fp8 and MXFP6
    gate and up projections of one layer run as one ops.fp8_swiglu / ops.mxfp6_swiglu as
    well (4 weight launches on the GPU instead of 5); MXFP4 is the same either way.
    `tiled` (opt-in) runs every packed projection - merged q/k/v, o_proj, gate/up and
    down_proj, in any of the three formats - on the many-row kernels (the format's
    *_linear / *_swiglu op with tiled=True): for MXFP4, and for fp8 and MXFP6 with
    `fuse_gated`, 4 weight launches for any batch * seq instead of 4 per 64 rows (fp8
    and MXFP6 without `fuse_gated`: 5, gate and up as two tiled linears), each row of a
    projection a function of that row of its input alone. It is ignored for plain
    tensors, and on the CPU it changes nothing.
    `act="mxfp8"` (opt-in) runs every MXFP4-packed projection as W4A8 (act= of
    ops.mxfp4_linear / ops.mxfp4_swiglu): the projection's input is quantized to MXFP8
    and multiplied on the block-scaled MFMA - four quantize and four matmul launches
    for any batch * seq with `fuse`. The result is that of the quantized activations,
    not of the W4A16 routes. A packed projection of another format raises ValueError
    instead of silently running W.A16; plain tensors are untouched; any other `act`
    raises ValueError.
    `cache` (opt-in): the pass is the prefill of that `KVCache` - the rotated k and the
    v of all seq positions are also stored at positions [0, seq) of every sequence,
    `cache.lens` becomes seq everywhere and `cache.max_len` seq; `decoder_step` goes on
    from there. The result is the same with and without it."""
    if act not in (None, "mxfp8"):
        raise ValueError(f"act must be None or 'mxfp8', got {act!r}")
    b, s, _ = x.shape
    hd, nh, nkv = spec.head_dim, spec.heads, spec.kv_heads
    if cache is not None:
        _check_cache(cache, spec, b, x.device)
        if s > cache.capacity:
            raise ValueError(f"{s} positions do not fit a cache of {cache.capacity}")
    h = _rms_norm(x, _dense(p["input_layernorm"]), spec.eps)
    q, k, v = _qkv(h, p, fuse, tiled, act)
    q = q.view(b, s, nh, hd).transpose(1, 2)
    k = k.view(b, s, nkv, hd).transpose(1, 2)
    v = v.view(b, s, nkv, hd).transpose(1, 2)
    q, k = _rope(q, spec.rope_theta), _rope(k, spec.rope_theta)
    if cache is not None:
        cache.k[:, :, :s] = k
        cache.v[:, :, :s] = v
        cache.lens.fill_(s)
        cache.max_len = s
    k = k.repeat_interleave(nh // nkv, dim=1)
    v = v.repeat_interleave(nh // nkv, dim=1)
    a = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    x = x + _linear(a.transpose(1, 2).reshape(b, s, nh * hd), p["o_proj"], tiled, act)
    h = _rms_norm(x, _dense(p["post_attention_layernorm"]), spec.eps)
    return x + _linear(_gated(h, p["gate_proj"], p["up_proj"], fuse, fuse_gated, tiled, act), p["down_proj"], tiled,
                       act)


def _check_cache(cache: KVCache, spec: DecoderSpec, batch: int, device: torch.device) -> None:
    want = (batch, spec.kv_heads, cache.capacity, spec.head_dim)
    if tuple(cache.k.shape) != want or tuple(cache.v.shape) != want:
        raise ValueError(f"the cache holds k {tuple(cache.k.shape)} and v {tuple(cache.v.shape)}, "
                         f"this batch and spec need {want}")
    if cache.k.device != device:
        raise ValueError(f"the cache is on {cache.k.device}, x on {device}")


def decoder_step(x: torch.Tensor, p: Dict[str, Param], spec: DecoderSpec, cache: KVCache, fuse: bool = True,
                 fuse_gated: bool = False, act: Optional[str] = None, advance: bool = True) -> torch.Tensor:
    """One decode step of a decoder layer: x [batch, 1, hidden] is the new token of every
    sequence, `cache` holds the k and v of the lens[b] tokens before it (a prefill by
    ``decoder_forward(..., cache=cache)`` or earlier steps). The layer is `decoder_forward`'s
    - the same norms, `_qkv`, `_linear` and `_gated`, so plain tensors, every packed route,
    `fuse`, `fuse_gated` and `act="mxfp8"` mean what they mean there - with the attention
    done against the cache: ``ops.rope_append`` rotates q and k at position lens[b] and
    appends k and v, ``ops.attn_decode`` attends over the lens[b] + 1 positions, reading K
    and V once per KV head. Nothing is read back to the host: the lengths stay on the
    device and `cache.max_len` sizes the launch.
    `advance` adds 1 to `cache.lens` (on the device) and to `cache.max_len`; with
    advance=False the caller does both once for all layers that share `lens`.
    ValueError for seq != 1, a batch or spec other than the cache's, and a full cache
    (`max_len` == `capacity`)."""
    if act not in (None, "mxfp8"):
        raise ValueError(f"act must be None or 'mxfp8', got {act!r}")
    if x.dim() != 3 or x.shape[1] != 1:
        raise ValueError(f"decoder_step takes x [batch, 1, hidden], got {tuple(x.shape)}")
    b = x.shape[0]
    _check_cache(cache, spec, b, x.device)
    if cache.max_len >= cache.capacity:
        raise ValueError(f"the cache is full: {cache.max_len} of {cache.capacity} positions")
    from ..ops import attn_decode, rope_append

    h = _rms_norm(x, _dense(p["input_layernorm"]), spec.eps)
    q, k, v = _qkv(h, p, fuse, False, act)
    q = rope_append(q, k, v, cache.cos, cache.sin, cache.k, cache.v, cache.lens)
    a = attn_decode(q, cache.k, cache.v, cache.lens + 1, max_len=cache.max_len + 1, out_dtype=x.dtype)
    if advance:
        cache.lens.add_(1)
        cache.max_len += 1
    x = x + _linear(a.view(b, 1, spec.heads * spec.head_dim), p["o_proj"], False, act)
    h = _rms_norm(x, _dense(p["post_attention_layernorm"]), spec.eps)
    return x + _linear(_gated(h, p["gate_proj"], p["up_proj"], fuse, fuse_gated, False, act), p["down_proj"], False,
                       act)
