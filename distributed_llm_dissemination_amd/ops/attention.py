"""The attention ops against a KV cache in HBM (csrc/kernels/attn_decode.hip, attn_prefill.hip and their
MXFP8 files) and their
host references, under the conventions of kernels.py (current stream, every check before any launch).

    # one decode step's attention: caches bf16 [B, kv_heads, capacity, d], lens / pos int32 [B] on the device
    q_rot = ops.rope_append(q, k, v, cos, sin, k_cache, v_cache, pos)     # rotate q and k at pos, append k and v
    a = ops.attn_decode(q_rot, k_cache, v_cache, pos + 1)                 # [B, heads * d], K and V read once per KV head
    # the same against an MXFP8 cache (attn_decode_mxfp8.hip): uint8 codes [B, kv_heads, capacity, d] and uint8
    # E8M0 scale bytes [B, kv_heads, capacity, d / 32] per cache, passed as k_scale= and v_scale=; d 64 or 128
    q_rot = ops.rope_append(q, k, v, cos, sin, k_codes, v_codes, pos, k_scale=k_scale, v_scale=v_scale)
    a = ops.attn_decode(q_rot, k_codes, v_codes, pos + 1, k_scale=k_scale, v_scale=v_scale)
    # S tokens a sequence (prefill, chunked prefill, extend): q/k/v [B, S, heads or kv_heads * d], start int32 [B]
    q_rot = ops.rope_append_seq(q, k, v, cos, sin, k_cache, v_cache, start)   # positions start[b] + i
    a = ops.attn_prefill(q_rot, k_cache, v_cache, start)                      # [B, S, heads * d], causal, reads the cache
    # the same against an MXFP8 cache (attn_prefill_mxfp8.hip): codes and scale bytes as above, contiguous
    q_rot = ops.rope_append_seq(q, k, v, cos, sin, k_codes, v_codes, start, k_scale=k_scale, v_scale=v_scale)
    a = ops.attn_prefill(q_rot, k_codes, v_codes, start, k_scale=k_scale, v_scale=v_scale)
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _core
from .kernels import _mxfp8_values, _stream, mxfp8_quantize_rows

__all__ = ["rope_append", "attn_decode", "rope_append_seq", "attn_prefill"]

_ATTN_D = (32, 64, 128)
_ATTN_MXFP8_D = (64, 128)
_ATTN_MAX_CAPACITY = 1 << 20


def _check_caches(k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: Optional[torch.Tensor] = None,
                  v_scale: Optional[torch.Tensor] = None) -> Tuple[int, int, int, int]:
    """(B, kv_heads, capacity, d) of a pair of KV caches, checked: bf16 caches without scales, or
    the uint8 codes of MXFP8 caches with the uint8 scale bytes of both."""
    mx = k_scale is not None or v_scale is not None
    if mx and (k_scale is None or v_scale is None):
        raise ValueError("an MXFP8 cache needs both k_scale and v_scale")
    want = torch.uint8 if mx else torch.bfloat16
    for name, c in (("k_cache", k_cache), ("v_cache", v_cache)):
        if c.dtype != want:
            raise ValueError(f"{name} must be {want} {'with' if mx else 'without'} k_scale and v_scale, got {c.dtype}")
        if c.dim() != 4 or c.numel() == 0:
            raise ValueError(f"{name} must be [B, kv_heads, capacity, d], got {tuple(c.shape)}")
        if not c.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if c.is_cuda and c.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")
    if k_cache.shape != v_cache.shape or k_cache.device != v_cache.device:
        raise ValueError("k_cache and v_cache must have one shape and one device")
    b, kvh, cap, d = k_cache.shape
    if d not in (_ATTN_MXFP8_D if mx else _ATTN_D):
        raise ValueError(f"head_dim must be one of {_ATTN_MXFP8_D if mx else _ATTN_D}, got {d}")
    if cap > _ATTN_MAX_CAPACITY:
        raise ValueError(f"capacity must be at most {_ATTN_MAX_CAPACITY} positions, got {cap}")
    if mx:
        for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            if t.dtype != torch.uint8 or tuple(t.shape) != (b, kvh, cap, d // 32) or t.device != k_cache.device:
                raise ValueError(f"{name} must be a uint8 [{b}, {kvh}, {cap}, {d // 32}] tensor on the caches' device")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if t.is_cuda and t.data_ptr() % 4:
                raise ValueError(f"{name} must be 4-byte aligned")
    return b, kvh, cap, d


def _mxfp8_rows(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """[..., d] codes and [..., d / 32] scale bytes as the bf16 values the kernel multiplies, in f32."""
    d = codes.shape[-1]
    vals = _mxfp8_values(codes.reshape(-1, d), scales.reshape(-1, d // 32))
    return vals.to(torch.bfloat16).float().view(codes.shape)


def _check_index(t: torch.Tensor, name: str, b: int, device: torch.device) -> None:
    if t.dtype != torch.int32:
        raise ValueError(f"{name} must be {torch.int32}, got {t.dtype}")
    if tuple(t.shape) != (b,) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [{b}] tensor, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name} must be on the caches' device")


def _check_rope_tables(cos: torch.Tensor, sin: torch.Tensor, cap: int, d: int, device: torch.device) -> None:
    for name, t in (("cos", cos), ("sin", sin)):
        if t.dtype != torch.float32 or tuple(t.shape) != (cap, d) or not t.is_contiguous() or t.device != device:
            raise ValueError(f"{name} must be a contiguous f32 [{cap}, {d}] tensor on the caches' device")


def _check_heads(heads: int, kvh: int) -> None:
    if heads % kvh:
        raise ValueError(f"heads ({heads}) must be a multiple of kv_heads ({kvh})")


def _check_out_dtype(out_dtype: torch.dtype) -> None:
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")


def _aligned_q(q: torch.Tensor) -> torch.Tensor:
    """`q` itself where it is contiguous on a 16-byte-aligned base, else a copy that is."""
    if not q.is_contiguous():
        q = q.contiguous()
    return q.clone() if q.data_ptr() % 16 else q


def _check_rows(t: torch.Tensor, name: str, device: torch.device, shape_ok: bool, want: str) -> None:
    if t.dtype != torch.bfloat16:
        raise ValueError(f"{name} must be {torch.bfloat16}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name} must be on the caches' device")
    if not shape_ok:
        raise ValueError(f"{name} must be {want}, got {tuple(t.shape)}")


def _rows(t: torch.Tensor, name: str, b: int, n: int, device: torch.device) -> torch.Tensor:
    """`t` as bf16 rows [b, n] with unit stride along the row and any row stride: the view
    itself where it allows that (a last-dimension slice of a merged projection), else a copy."""
    _check_rows(t, name, device, t.numel() == b * n and t.dim() >= 1 and t.shape[-1] == n,
                f"[{b}, ..., {n}] with {b} rows")
    lead = [i for i in range(t.dim() - 1) if t.shape[i] != 1]
    if t.stride(-1) == 1 and len(lead) <= 1:
        ld = t.stride(lead[0]) if lead else n
        if ld >= n:
            return t.as_strided((b, n), (ld, 1))
    return t.reshape(b, n).contiguous()


def _rows_seq(t: torch.Tensor, name: str, b: int, s: int, n: int, device: torch.device) -> torch.Tensor:
    """`t` [b, s, n] as bf16 rows [b * s, n] with unit stride along the row, one row stride that is a multiple
    of 8 elements and, on the GPU, a 16-byte-aligned base: the view itself where it allows that, else a copy."""
    _check_rows(t, name, device, tuple(t.shape) == (b, s, n), f"[{b}, {s}, {n}]")
    ld = t.stride(1) if s > 1 else (t.stride(0) if b > 1 else n)
    if (t.stride(2) == 1 and ld >= n and ld % 8 == 0 and (b == 1 or s == 1 or t.stride(0) == s * ld)
            and (not t.is_cuda or t.data_ptr() % 16 == 0)):
        return t.as_strided((b * s, n), (ld, 1))
    return t.reshape(b * s, n).contiguous()


def _rope_cpu(q2: torch.Tensor, k2: torch.Tensor, v2: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
              k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor, heads: int,
              k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The host route of both rope ops: rows [B * S, heads or kv_heads * d] at positions `pos` int64 [B, S].
    With scales the bf16 rows go through the host MXFP8 codec into the caches. Returns q rotated
    [B, S, heads, d]."""
    b, s = pos.shape
    _, kvh, cap, d = k_cache.shape
    ok = (pos >= 0) & (pos < cap)
    p = pos.clamp(0, cap - 1)
    c, sn = cos[p][:, :, None, :], sin[p][:, :, None, :]  # [B, S, 1, d]

    def rot(x, nh):
        x = x.reshape(b, s, nh, d).float()
        return (x * c + torch.cat([-x[..., d // 2:], x[..., : d // 2]], -1) * sn).to(torch.bfloat16)

    q_out = torch.where(ok[:, :, None, None], rot(q2, heads), torch.zeros((), dtype=torch.bfloat16))
    bi, si = ok.nonzero(as_tuple=True)
    k_new, v_new = rot(k2, kvh)[bi, si], v2.reshape(b, s, kvh, d)[bi, si]
    if k_scale is not None and bi.numel():
        (k_new, ks), (v_new, vs) = mxfp8_quantize_rows(k_new), mxfp8_quantize_rows(v_new)
        k_scale[bi, :, p[bi, si]] = ks
        v_scale[bi, :, p[bi, si]] = vs
    k_cache[bi, :, p[bi, si]] = k_new
    v_cache[bi, :, p[bi, si]] = v_new
    return q_out


def _rows16(t: torch.Tensor) -> torch.Tensor:
    """Rows [b, n] for 16-byte loads: `t` itself where its row stride is a multiple of 8 elements on a
    16-byte-aligned base, else a copy."""
    if t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous() if not t.is_contiguous() else t.clone()


def rope_append(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor, *,
                k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rotary embedding of one new token per sequence, fused with the cache append.

    `q` [B, ..., heads * d], `k` and `v` [B, ..., kv_heads * d] are bf16 rows of B sequences
    (unit stride along the row, any row stride: the three last-dimension slices of one merged
    q/k/v projection are used where they lie, as are three separate tensors); `k_cache` and
    `v_cache` bf16 [B, kv_heads, capacity, d], contiguous, d 32, 64 or 128; `cos`, `sin` f32
    [capacity, d], the tables of the rotate-half rotary embedding; `pos` int32 [B] on the
    caches' device. Returns q rotated at `pos`, bf16 [B, heads, d], and writes k rotated at
    `pos` and v as it is to position pos[b] of every KV head of sequence b. The rotation is
    ``x * cos + rot(x) * sin`` in f32 - two rounded products, one rounded sum, no FMA - rounded
    once to bf16: the bits plain torch gives for the same expression. A pos[b] outside
    [0, capacity) writes nothing to the caches and gives a zero q row.
    GPU: one launch on the current stream, no synchronization (`pos` is never read on the
    host). CPU: plain torch.
    MXFP8 caches (`k_scale` and `v_scale` given; attn_decode_mxfp8.hip): `k_cache` and
    `v_cache` are the uint8 e4m3fn codes [B, kv_heads, capacity, d], 16-byte aligned, and the
    scales the uint8 E8M0 bytes [B, kv_heads, capacity, d // 32], one per 32 d, all
    contiguous; d 64 or 128. The returned q has the bits of the bf16 route; k is rotated and
    rounded to bf16, then quantized, v is quantized as it is: the bytes written are those of
    `mxfp8_quantize_rows` (the host codec) of the rows the bf16 route writes, scale bytes in
    [1, 247]. An out-of-range pos[b] writes nothing to the four tensors. GPU: still one
    launch, 16-byte loads (rows whose stride or base does not allow them are copied first).
    bf16 caches with a scale, uint8 caches without both, scales of another shape, dtype,
    device or layout and d = 32 are ValueErrors before any launch."""
    b, kvh, cap, d = _check_caches(k_cache, v_cache, k_scale, v_scale)
    dev = k_cache.device
    _check_index(pos, "pos", b, dev)
    _check_rope_tables(cos, sin, cap, d, dev)
    if q.dim() < 1 or q.shape[-1] <= 0 or q.shape[-1] % d:
        raise ValueError(f"q must be [B, ..., heads * {d}], got {tuple(q.shape)}")
    heads = q.shape[-1] // d
    _check_heads(heads, kvh)
    if heads + 2 * kvh > 65535:
        raise ValueError("heads + 2 * kv_heads must fit a grid dimension (65535)")
    q2, k2, v2 = _rows(q, "q", b, heads * d, dev), _rows(k, "k", b, kvh * d, dev), _rows(v, "v", b, kvh * d, dev)
    if not dev.type == "cuda":
        return _rope_cpu(q2, k2, v2, cos, sin, k_cache, v_cache, pos.long()[:, None], heads, k_scale,
                         v_scale).view(b, heads, d)
    q_out = torch.empty(b, heads, d, dtype=torch.bfloat16, device=dev)
    if k_scale is not None:
        if cos.data_ptr() % 16 or sin.data_ptr() % 16:
            raise ValueError("cos and sin must be 16-byte aligned")
        q2, k2, v2 = _rows16(q2), _rows16(k2), _rows16(v2)
        _core.attn_rope_append_mxfp8(q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0), v2.data_ptr(),
                                     v2.stride(0), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), b, heads, kvh, d,
                                     cap, q_out.data_ptr(), k_cache.data_ptr(), k_scale.data_ptr(),
                                     v_cache.data_ptr(), v_scale.data_ptr(), _stream())
        return q_out
    _core.attn_rope_append(q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0), v2.data_ptr(), v2.stride(0),
                           pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), b, heads, kvh, d, cap, q_out.data_ptr(),
                           k_cache.data_ptr(), v_cache.data_ptr(), _stream())
    return q_out


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor, *,
                k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None,
                max_len: Optional[int] = None, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Grouped-query attention of one query token per sequence against a KV cache:
    row b of the [B, heads * d] result is, per head h, ``softmax(q[b, h] @ K.T / sqrt(d)) @ V``
    over K, V = cache[b, h // (heads // kv_heads), :lens[b]].

    `q` bf16 [B, heads, d]; the caches bf16 [B, kv_heads, capacity, d], contiguous, d 32, 64
    or 128, capacity at most 2**20, heads // kv_heads in 1..16; `lens` int32 [B] on the
    caches' device, 0 <= lens[b] <= `max_len`, a host upper bound that sizes the grid and the
    workspace (default: the capacity - a decode loop that knows its lengths should pass it).
    Positions at or behind lens[b] are never read - the cache there may hold anything - and
    lens[b] == 0 gives a zero row. `out_dtype` bf16 or f32; the bf16 result is the f32 one
    rounded to nearest even.
    GPU (attn_decode.hip): a workgroup serves one (sequence, KV head, chunk of
    `_core.attn_decode_chunk()` positions) and all the query heads of the KV head, so K and V
    are read once per KV head; f32 scores and online softmax, P rounded to bf16 for P @ V on
    the bf16 MFMA; f32 chunk partials in a workspace, merged in ascending chunk order by a
    second launch. Chunk boundaries are multiples of the constant, so a sequence's row has the
    same bits in any batch, at any slot, under any capacity and `max_len`. Two launches on the
    current stream, no synchronization, no atomics. CPU: per sequence the definition in f32.
    `lens` outside the promise: a negative lens[b] is 0 (a zero row), one above the capacity is
    the capacity; a lens[b] above `max_len` gives a finite row of finite cache rows (GPU: the
    positions below lens[b] of the chunks that cover `max_len`) and never reads outside the
    caches or the workspace. No other sequence's row changes by a bit in any of these cases.
    Magnitudes, on the GPU: finite scores of any size are exact in the softmax (a weight that
    underflows is exactly 0), bf16-subnormal V and f32-subnormal products are kept, not
    flushed. Non-finite values inside the valid prefix stay with the query heads of their
    (sequence, KV head) and leave every other element its bits: a NaN in a K row makes those
    heads' rows NaN; +inf in a V element makes that d of those heads +inf where the position
    has weight, and NaN where its weight underflowed to 0 (0 * inf; the definition gives
    +inf). A head one of whose scores q . k overflows f32 to +inf gets a NaN row (the
    definition: the V row of that position). The numerator sum(p~ v), p~ = exp(s - max s) <=
    1, is summed in f32 before the division by sum(p~): where it overflows the result is +-inf
    although the quotient would be finite.
    MXFP8 caches (`k_scale` and `v_scale` given; attn_decode_mxfp8.hip): `k_cache` and
    `v_cache` are the uint8 e4m3fn codes [B, kv_heads, capacity, d], 16-byte aligned, the
    scales the uint8 E8M0 bytes [B, kv_heads, capacity, d // 32], block j of a row being
    elements [32 j, 32 j + 32); all contiguous, d 64 or 128 - 33/64 of the bf16 cache's bytes.
    Dequantization is ``code * 2**(byte - 127)`` rounded to bf16 to nearest even, which is
    exact except where the product falls between bf16 subnormals (a subnormal code at a byte
    of 3 or less). The result is that of this op on the dequantized cache - f32 scores,
    online softmax per 32 positions, P rounded to bf16, the same chunks and combine - and as
    bit-invariant to batch, slot, capacity and `max_len`; bit equality with the bf16 kernel
    is not promised, because K's d sit in other k slots of the MFMA. The GPU kernel
    dequantizes codes in registers into the bf16 MFMA's operands, K from 16-byte and V from 8-
    (d = 64: 4-) byte loads, and loads neither codes nor scale bytes at or behind lens[b].
    The quantizers write scale bytes in [1, 247]; a byte of 255 or a NaN code (0x7F / 0xFF)
    inside the valid prefix makes the rows of that (sequence, KV head) NaN - in K all of
    each row, in V the d of the code or the 32 d of the byte's block - and leaves every
    other row its bits; a byte of 0 is outside the contract (an unspecified value, no
    out-of-bounds access). CPU: the valid prefix dequantized, then the definition in f32.
    bf16 caches with a scale, uint8 caches without both, scales of another shape, dtype,
    device or layout and d = 32 are ValueErrors before any launch."""
    b, kvh, cap, d = _check_caches(k_cache, v_cache, k_scale, v_scale)
    dev = k_cache.device
    _check_out_dtype(out_dtype)
    _check_rows(q, "q", dev, q.dim() == 3 and q.shape[0] == b and q.shape[2] == d and q.shape[1] >= 1,
                f"[{b}, heads, {d}]")
    heads = q.shape[1]
    _check_heads(heads, kvh)
    if heads // kvh > 16:
        raise ValueError(f"at most 16 query heads per KV head, got {heads // kvh}")
    _check_index(lens, "lens", b, dev)
    max_len = cap if max_len is None else int(max_len)
    if not 1 <= max_len <= cap:
        raise ValueError(f"max_len must be in 1..capacity ({cap}), got {max_len}")
    if dev.type != "cuda":
        y = torch.zeros(b, heads, d, dtype=torch.float32)
        g = heads // kvh
        for i, n in enumerate(lens.tolist()):
            n = min(max(n, 0), cap)
            if n == 0:
                continue
            if k_scale is None:
                kk, vv = k_cache[i, :, :n].float(), v_cache[i, :, :n].float()
            else:
                kk, vv = _mxfp8_rows(k_cache[i, :, :n], k_scale[i, :, :n]), _mxfp8_rows(v_cache[i, :, :n], v_scale[i, :, :n])
            kk, vv = kk.repeat_interleave(g, dim=0), vv.repeat_interleave(g, dim=0)  # [heads, n, d]
            s = torch.einsum("hd,hnd->hn", q[i].float(), kk) / d ** 0.5
            y[i] = torch.einsum("hn,hnd->hd", torch.softmax(s, -1), vv)
        return y.view(b, heads * d).to(out_dtype)
    q = _aligned_q(q)
    nbytes = _core.attn_decode_workspace_bytes(b, heads, kvh, d, cap, max_len)
    if nbytes < 0 or b * heads > 0x7FFFFFFF:
        raise ValueError("the batch is too large for one launch")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    y = torch.empty(b, heads * d, dtype=out_dtype, device=dev)
    if k_scale is not None:
        _core.attn_decode_mxfp8(q.data_ptr(), k_cache.data_ptr(), k_scale.data_ptr(), v_cache.data_ptr(),
                                v_scale.data_ptr(), lens.data_ptr(), b, heads, kvh, d, cap, max_len, ws.data_ptr(),
                                nbytes, y.data_ptr(), out_dtype == torch.bfloat16, _stream())
        return y
    _core.attn_decode(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), lens.data_ptr(), b, heads, kvh, d, cap,
                      max_len, ws.data_ptr(), nbytes, y.data_ptr(), out_dtype == torch.bfloat16, _stream())
    return y


def _kv_view(t: torch.Tensor) -> torch.Tensor:
    """`t` [B, kv_heads, T, d] itself where the prefill kernel can read it in place - unit stride
    along d, every other stride a multiple of 8 elements and not negative, a 16-byte-aligned
    base - else a contiguous copy."""
    ok = t.stride(3) == 1 and all(t.shape[i] == 1 or (t.stride(i) >= 0 and t.stride(i) % 8 == 0) for i in range(3))
    if ok and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous() if not t.is_contiguous() else t.clone()


def _kv_strides(t: torch.Tensor) -> Tuple[int, int, int]:
    return tuple(t.stride(i) if t.shape[i] > 1 else 0 for i in range(3))


def _prefill_cpu(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, start: Optional[torch.Tensor],
                 k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The host route of attn_prefill: per sequence the definition in f32, [B, S, heads * d] f32; with scales
    on the dequantized valid prefix."""
    b, s, heads, d = q.shape
    kvh, t_len = k.shape[1], k.shape[2]
    y = torch.zeros(b, s, heads, d, dtype=torch.float32)
    st = [0] * b if start is None else [min(max(n, 0), t_len) for n in start.tolist()]
    g = heads // kvh
    for i in range(b):
        rows = min(s, t_len - st[i])  # rows whose position is below T
        if rows <= 0:
            continue
        n = st[i] + rows
        if k_scale is None:
            kk, vv = k[i, :, :n].float(), v[i, :, :n].float()
        else:
            kk, vv = _mxfp8_rows(k[i, :, :n], k_scale[i, :, :n]), _mxfp8_rows(v[i, :, :n], v_scale[i, :, :n])
        kk, vv = kk.repeat_interleave(g, dim=0), vv.repeat_interleave(g, dim=0)  # [heads, n, d]
        sc = torch.einsum("shd,hnd->hsn", q[i, :rows].float(), kk) / d ** 0.5
        seen = torch.arange(n)[None, :] <= (st[i] + torch.arange(rows))[:, None]
        p = torch.softmax(sc.masked_fill(~seen, float("-inf")), -1)
        y[i, :rows] = torch.einsum("hsn,hnd->shd", p, vv)
    return y.view(b, s, heads * d)


def _attn_prefill_mxfp8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, start: Optional[torch.Tensor],
                        k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor],
                        out_dtype: torch.dtype) -> torch.Tensor:
    """attn_prefill against MXFP8 caches: every check, then the host route or attn_prefill_mxfp8.hip."""
    b, kvh, t_len, d = _check_caches(k, v, k_scale, v_scale)
    dev = k.device
    _check_rows(q, "q", dev, q.dim() == 4 and q.shape[0] == b and q.shape[3] == d and q.shape[1] >= 1
                and q.shape[2] >= 1, f"[{b}, S, heads, {d}]")
    s, heads = q.shape[1], q.shape[2]
    _check_heads(heads, kvh)
    if s > _ATTN_MAX_CAPACITY:
        raise ValueError(f"S must be at most {_ATTN_MAX_CAPACITY}, got {s}")
    if start is not None:
        _check_index(start, "start", b, dev)
    if dev.type != "cuda":
        return _prefill_cpu(q, k, v, start, k_scale, v_scale).to(out_dtype)
    if b > (1 << 20) or b * heads * -(-s // _core.attn_prefill_tiles()[0]) > 0x7FFFFFFF:
        raise ValueError("the batch is too large for one launch")
    q = _aligned_q(q)
    y = torch.empty(b, s, heads * d, dtype=out_dtype, device=dev)
    _core.attn_prefill_mxfp8(q.data_ptr(), k.data_ptr(), k_scale.data_ptr(), v.data_ptr(), v_scale.data_ptr(),
                             0 if start is None else start.data_ptr(), b, s, heads, kvh, d, t_len, y.data_ptr(),
                             out_dtype == torch.bfloat16, _stream())
    return y


def attn_prefill(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, start: Optional[torch.Tensor] = None, *,
                 k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None,
                 out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Causal grouped-query attention of S new tokens per sequence against K and V that already
    hold them (a prefill, or the extend of a cache by S tokens): row (b, i) of the [B, S, heads *
    d] result is, per head h, ``softmax(q[b, i, h] @ K.T / sqrt(d)) @ V`` over K, V = k / v[b, h //
    (heads // kv_heads), :start[b] + i + 1].

    `q` bf16 [B, S, heads, d]; `k` and `v` bf16 [B, kv_heads, T, d], d 32, 64 or 128, any heads
    // kv_heads >= 1, S and T at most 2**20. A view with unit stride along d whose other strides
    are multiples of 8 elements on a 16-byte-aligned base is read where it lies - a `KVCache`'s
    tensors, or the k / v column slices of one merged q/k/v projection viewed as [B, S,
    kv_heads, d].transpose(1, 2) - anything else is made contiguous first. `start` int32 [B] on
    the tensors' device (never read on the host), or None for zeros: token i of sequence b sits
    at position start[b] + i. Positions at or behind min(start[b] + S, T) are never read - the
    cache there may hold anything. `out_dtype` bf16 or f32; the bf16 result is the f32 one
    rounded to nearest even.
    GPU (attn_prefill.hip): a workgroup of four waves serves one (sequence, query head, tile of
    BQ = 128 rows; `_core.attn_prefill_tiles()` gives (BQ, BK)), a wave 32 rows; K and V tiles of
    BK = 64 positions at absolute positions 0, BK, ... are fetched once per workgroup into
    double-buffered, swizzled LDS; scores K Q^T and the output V^T P^T run on the bf16 MFMA with
    f32 scores, an online softmax per 32 positions and P rounded to bf16 (attn_decode's
    numerics); the heads of a KV group are neighbouring workgroups and the longest query tile
    is issued first. A row's bits depend on its q row, its position and the K / V rows up to it
    alone: the same in any batch, at any slot, for any S, start, T, strides and split of the
    tokens into passes. One launch on the current stream; no workspace, atomics or
    synchronization. CPU: per sequence the definition in f32.
    Outside the promise: a negative start[b] counts as 0; a row whose position is >= T is a zero
    row and loads nothing. Non-finite values inside a sequence's valid positions, on the GPU: a
    NaN in a K row makes the rows that see its position NaN, in the query heads of its KV head;
    a non-finite V element at position j makes that d non-finite in the rows at and behind j,
    and NaN in the rows fewer than 63 positions BEFORE j whose wave still visits j's 32
    positions - there it meets a weight of exactly 0 (the definition: no effect). Every other
    row, head and sequence keeps its bits.
    MXFP8 caches (`k_scale` and `v_scale` given; attn_prefill_mxfp8.hip): `k` and `v` are the
    uint8 e4m3fn codes [B, kv_heads, T, d], 16-byte aligned, the scales the uint8 E8M0 bytes
    [B, kv_heads, T, d // 32] of `attn_decode`'s format; all contiguous (no strided views), d
    64 or 128. GPU: the same decomposition; a tile's codes, 16 a lane and load, and scale
    bytes are dequantized once per workgroup on the way from registers into LDS, which then
    holds the bf16 tile the bf16 kernel holds. For codes and scale bytes whose dequantization
    ``code * 2**(byte - 127)`` is exact in bf16 - everything the quantizers write - the result
    has the bits of this op on the dequantized bf16 cache, in f32 and in bf16, and with them
    its invariance (batch, slot, S, start, T, split into passes) and its non-finite
    behaviour: a NaN code (0x7F / 0xFF) or a scale byte of 255 inside the valid positions
    acts as the NaN values it dequantizes to. A scale byte of 0 is outside the contract (an
    unspecified value, no out-of-bounds access). Neither codes nor scale bytes at or behind
    min(start[b] + S, T) are loaded. CPU: the valid prefix dequantized, then the definition in
    f32. bf16 tensors with a scale, uint8 tensors without both, scales of another shape,
    dtype, device or layout and d = 32 are ValueErrors before any launch."""
    _check_out_dtype(out_dtype)
    if k_scale is not None or v_scale is not None:
        return _attn_prefill_mxfp8(q, k, v, start, k_scale, v_scale, out_dtype)
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype != torch.bfloat16:
            raise ValueError(f"{name} must be {torch.bfloat16}, got {t.dtype}")
        if t.dim() != 4 or t.numel() == 0:
            raise ValueError(f"{name} must be 4-dimensional and not empty, got {tuple(t.shape)}")
        if t.device != q.device:
            raise ValueError(f"{name} must be on q's device")
    if k.shape != v.shape:
        raise ValueError(f"k and v must have one shape, got {tuple(k.shape)} and {tuple(v.shape)}")
    b, s, heads, d = q.shape
    if d not in _ATTN_D:
        raise ValueError(f"head_dim must be one of {_ATTN_D}, got {d}")
    kvh, t_len = k.shape[1], k.shape[2]
    if k.shape[0] != b or k.shape[3] != d:
        raise ValueError(f"k and v must be [{b}, kv_heads, T, {d}], got {tuple(k.shape)}")
    _check_heads(heads, kvh)
    if s > _ATTN_MAX_CAPACITY or t_len > _ATTN_MAX_CAPACITY:
        raise ValueError(f"S and T must be at most {_ATTN_MAX_CAPACITY}, got {s} and {t_len}")
    dev = q.device
    if start is not None:
        _check_index(start, "start", b, dev)
    if dev.type != "cuda":
        return _prefill_cpu(q, k, v, start).to(out_dtype)
    if b > (1 << 20) or b * heads * -(-s // _core.attn_prefill_tiles()[0]) > 0x7FFFFFFF:
        raise ValueError("the batch is too large for one launch")
    q, k, v = _aligned_q(q), _kv_view(k), _kv_view(v)
    y = torch.empty(b, s, heads * d, dtype=out_dtype, device=dev)
    _core.attn_prefill(q.data_ptr(), k.data_ptr(), v.data_ptr(), 0 if start is None else start.data_ptr(), b, s, heads,
                       kvh, d, t_len, _kv_strides(k), _kv_strides(v), y.data_ptr(), out_dtype == torch.bfloat16,
                       _stream())
    return y


def rope_append_seq(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                    k_cache: torch.Tensor, v_cache: torch.Tensor, start: Optional[torch.Tensor] = None, *,
                    k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`rope_append` for S tokens per sequence in one launch: the rotary embedding of q and k at
    positions start[b] + i, fused with the cache append.

    `q` [B, S, heads * d], `k` and `v` [B, S, kv_heads * d] are bf16 (unit stride along the
    row; rows b * S + i one stride apart, a multiple of 8 elements: the three last-dimension
    slices of one merged q/k/v projection are used where they lie, as are three contiguous
    tensors; anything else is copied); `k_cache` and `v_cache` bf16 [B, kv_heads, capacity, d],
    contiguous, d 32, 64 or 128; `cos`, `sin` f32 [capacity, d]; `start` int32 [B] on the caches'
    device, or None for zeros. Returns q rotated, bf16 [B, S, heads, d], and writes k rotated and
    v as it is to position start[b] + i of every KV head of sequence b. The rotation is
    ``x * cos + rot(x) * sin`` in f32 - two rounded products, one rounded sum, no FMA - rounded
    once to bf16: the bits of `rope_append` and of plain torch. A position outside [0,
    capacity) writes nothing to the caches and gives a zero q row.
    GPU (attn_prefill.hip): one launch on the current stream, 16-byte loads and stores - a
    thread rotates 8 d of the lower half with their partners of the upper half - and no
    synchronization (`start` is never read on the host). CPU: plain torch.
    MXFP8 caches (`k_scale` and `v_scale` given; attn_prefill_mxfp8.hip): `k_cache` and
    `v_cache` are the uint8 codes and the scales the uint8 E8M0 bytes of `rope_append`'s
    format, d 64 or 128. The returned q has the bits of the bf16 route; the four tensors
    receive exactly the bytes S successive ``rope_append(..., k_scale=, v_scale=)`` calls
    write - the host codec's of the rows the bf16 route writes - and no other byte changes; a
    position outside [0, capacity) writes nothing to them. GPU: still one launch - `rope_append`'s
    thread map and quantizer, one workgroup per (token, 256 items of its heads), B * S below
    2**31. bf16 caches with a scale, uint8 caches without both, scales of another shape,
    dtype, device or layout and d = 32 are ValueErrors before any launch."""
    b, kvh, cap, d = _check_caches(k_cache, v_cache, k_scale, v_scale)
    dev = k_cache.device
    if start is not None:
        _check_index(start, "start", b, dev)
    _check_rope_tables(cos, sin, cap, d, dev)
    if q.dim() != 3 or q.shape[0] != b or q.shape[1] < 1 or q.shape[2] <= 0 or q.shape[2] % d:
        raise ValueError(f"q must be [{b}, S, heads * {d}], got {tuple(q.shape)}")
    s, heads = q.shape[1], q.shape[2] // d
    _check_heads(heads, kvh)
    if s > _ATTN_MAX_CAPACITY or b * s > (1 << 31) or heads > 65535:
        raise ValueError("too many tokens or heads for one launch")
    q2, k2, v2 = (_rows_seq(q, "q", b, s, heads * d, dev), _rows_seq(k, "k", b, s, kvh * d, dev),
                  _rows_seq(v, "v", b, s, kvh * d, dev))
    if dev.type != "cuda":
        st = torch.zeros(b, dtype=torch.long) if start is None else start.long()
        return _rope_cpu(q2, k2, v2, cos, sin, k_cache, v_cache, st[:, None] + torch.arange(s)[None, :], heads,
                         k_scale, v_scale)
    q_out = torch.empty(b, s, heads, d, dtype=torch.bfloat16, device=dev)
    if k_scale is not None:
        if cos.data_ptr() % 16 or sin.data_ptr() % 16:
            raise ValueError("cos and sin must be 16-byte aligned")
        if b * s > 0x7FFFFFFF:
            raise ValueError("too many tokens for one launch")
        _core.attn_rope_append_seq_mxfp8(q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0), v2.data_ptr(),
                                         v2.stride(0), 0 if start is None else start.data_ptr(), cos.data_ptr(),
                                         sin.data_ptr(), b, s, heads, kvh, d, cap, q_out.data_ptr(),
                                         k_cache.data_ptr(), k_scale.data_ptr(), v_cache.data_ptr(),
                                         v_scale.data_ptr(), _stream())
        return q_out
    _core.attn_rope_append_seq(q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0), v2.data_ptr(), v2.stride(0),
                               0 if start is None else start.data_ptr(), cos.data_ptr(), sin.data_ptr(), b, s, heads,
                               kvh, d, cap, q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), _stream())
    return q_out
