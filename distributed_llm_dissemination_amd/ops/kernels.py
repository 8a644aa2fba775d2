"""PyTorch-facing wrappers of the gfx950 kernels (csrc/kernels/*.hip).

Every op takes and returns CUDA (HIP) tensors (the consumers of a packed
layer, mxfp4_unpack_range, mxfp4_linear, mxfp4_swiglu, fp8_unpack_range,
fp8_linear, fp8_swiglu, mxfp6_unpack_range, mxfp6_linear and mxfp6_swiglu, and the two ops of a decode step
against a KV cache, rope_append and attn_decode, also take CPU tensors and then use the host reference) and runs on the caller's current stream, so it composes with PyTorch work without extra synchronization. Shapes,
dtypes, alignment and sizes are checked on the host before any launch (a kernel
must never be handed a buffer smaller than its grid assumes).

    import torch
    from distributed_llm_dissemination_amd import ops
    x = torch.randn(1 << 24, dtype=torch.bfloat16, device="cuda")
    q, s = ops.fp8_pack(x)                    # OCP e4m3fn + one f32 scale per 128 values
    y = ops.fp8_unpack(q, s)                  # bf16 again
    q4, s4 = ops.mxfp4_pack(x)                # MXFP4: e2m1 pairs + one E8M0 scale per 32 values
    q6, s6 = ops.mxfp6_pack(x)                # MXFP6: 24 bytes of e2m3 codes + one E8M0 scale per 32 values
    crc = ops.crc32c(x.view(torch.uint8), 64 << 20)   # CRC32C per 64 MiB chunk
    w = x.view(4096, 4096)                              # a bf16 [out, in] weight ...
    p = ops.mxfp4_pack_layer(x, 64 << 20)               # ... as an MXFP4-packed layer (17/64 of the bytes)
    h = torch.randn(8, 4096, dtype=torch.bfloat16, device="cuda")
    y = ops.mxfp4_linear(h, p, 4096, 4096, src_bytes=2 * x.numel(), chunk_bytes=64 << 20)   # h @ w.T from the packed bytes
    z = ops.mxfp4_swiglu(h, p, 2048, 4096, src_bytes=2 * x.numel(), chunk_bytes=64 << 20,   # silu(h @ wg.T) * (h @ wu.T),
                         gate_offset=0, up_offset=2048 * 4096)                              # wg, wu = w[:2048], w[2048:]
    p8 = ops.fp8_pack_layer(x, 64 << 20)                # the same layer fp8-packed (33/64 of the bytes at block 128)
    y8 = ops.fp8_linear(h, p8, 4096, 4096, src_bytes=2 * x.numel(), chunk_bytes=64 << 20)   # h @ w.T from those bytes
    p6 = ops.mxfp6_pack_layer(x, 64 << 20)              # the same layer MXFP6-packed (25/64 of the bytes)
    y6 = ops.mxfp6_linear(h, p6, 4096, 4096, src_bytes=2 * x.numel(), chunk_bytes=64 << 20) # h @ w.T from those bytes
    z6 = ops.mxfp6_swiglu(h, p6, 2048, 4096, src_bytes=2 * x.numel(), chunk_bytes=64 << 20, # the gated front half from
                          gate_offset=0, up_offset=2048 * 4096)                             # those bytes (fp8_swiglu: p8)
    # one decode step's attention: caches bf16 [B, kv_heads, capacity, d], lens / pos int32 [B] on the device
    q_rot = ops.rope_append(q, k, v, cos, sin, k_cache, v_cache, pos)     # rotate q and k at pos, append k and v
    a = ops.attn_decode(q_rot, k_cache, v_cache, pos + 1)                 # [B, heads * d], K and V read once per KV head

These are the kernels the data engine runs itself (staging-time fp8 packing,
per-chunk CRC verification of every landed chunk); here they are usable on
their own, e.g. to check or unpack a layer a rank received.
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from .. import _core

__all__ = [
    "fill_random_",
    "crc32c",
    "crc32c_values",
    "fp8_pack",
    "fp8_unpack",
    "fp8_pack_layer",
    "fp8_verify_unpack",
    "fp8_verify_unpack_chunks",
    "fp8_packed_size",
    "mxfp4_pack",
    "mxfp4_unpack",
    "mxfp4_pack_layer",
    "mxfp4_verify_unpack",
    "mxfp4_verify_unpack_chunks",
    "mxfp4_packed_size",
    "mxfp4_unpack_range",
    "mxfp4_linear",
    "mxfp4_swiglu",
    "mxfp6_pack",
    "mxfp6_unpack",
    "mxfp6_pack_layer",
    "mxfp6_verify_unpack",
    "mxfp6_verify_unpack_chunks",
    "mxfp6_packed_size",
    "mxfp6_unpack_range",
    "mxfp6_linear",
    "fp8_unpack_range",
    "fp8_linear",
    "mxfp6_swiglu",
    "fp8_swiglu",
    "rope_append",
    "attn_decode",
]

_FP8_BLOCKS = (32, 64, 128, 256, 512)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _check_dev(t: torch.Tensor, name: str, dtype=None, align: int = 16) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if t.data_ptr() % align:
        raise ValueError(f"{name} must be {align}-byte aligned")


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def fill_random_(t: torch.Tensor, seed: int) -> torch.Tensor:
    """Fill `t` with counter-based random bytes (splitmix64 of (seed, 8-byte index));
    byte-identical to `_core.fill_random_host(nbytes, seed)`."""
    _check_dev(t, "t", align=1)
    _core.fill_random(t.data_ptr(), _nbytes(t), seed, _stream())
    return t


def crc32c(t: torch.Tensor, chunk_bytes: int = 0) -> torch.Tensor:
    """CRC32C (Castagnoli) of every `chunk_bytes` chunk of `t`'s bytes (whole
    tensor when 0), as an int32 GPU tensor holding the uint32 bit patterns. One
    chunk may have any length; several need a chunk size that is a multiple of
    16 (every chunk starts 16-B aligned)."""
    _check_dev(t, "t")
    n = _nbytes(t)
    chunk = min(chunk_bytes or n, n)
    if n <= 0:
        return torch.empty(0, dtype=torch.int32, device=t.device)
    if chunk < n and chunk % 16:
        raise ValueError("chunk_bytes must be a multiple of 16 when the tensor holds several chunks")
    nchunks = (n + chunk - 1) // chunk
    out = torch.empty(nchunks, dtype=torch.int32, device=t.device)
    # the fold words of the launch: zeroed (kernels.h: the kernel leaves them zeroed)
    ws = torch.zeros(_core.crc32c_workspace_bytes(n, chunk), dtype=torch.uint8, device=t.device)
    _core.crc32c_chunks_async(t.data_ptr(), n, chunk, out.data_ptr(), ws.data_ptr(), _stream())
    return out


def crc32c_values(crcs: torch.Tensor) -> List[int]:
    """The unsigned CRC values of a `crc32c()` result (synchronizes)."""
    return [v & 0xFFFFFFFF for v in crcs.tolist()]


def fp8_pack(x: torch.Tensor, block: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 -> OCP fp8 e4m3fn with one power-of-two f32 scale per `block` values
    (2^E, the smallest E >= -126 with the block's finite amax <= 448 * 2^E; core/fp8.h).
    Non-finite inputs: +-inf saturate to +-448*scale, NaN stays NaN.
    Returns (q: float8_e4m3fn [n], scales: float32 [n / block])."""
    _check_dev(x, "x", torch.bfloat16)
    if block not in _FP8_BLOCKS:
        raise ValueError(f"block must be one of {_FP8_BLOCKS}")
    n = x.numel()
    if n % block:
        raise ValueError(f"numel ({n}) must be a multiple of block ({block})")
    q = torch.empty(n, dtype=torch.float8_e4m3fn, device=x.device)
    s = torch.empty(n // block, dtype=torch.float32, device=x.device)
    _core.fp8_pack(x.data_ptr(), n, q.data_ptr(), s.data_ptr(), block, _stream())
    return q, s


def fp8_unpack(q: torch.Tensor, scales: torch.Tensor, block: int = 128) -> torch.Tensor:
    """Inverse of `fp8_pack`: bf16 values q * scale (round to nearest even)."""
    if q.dtype not in (torch.float8_e4m3fn, torch.uint8):
        raise ValueError("q must be float8_e4m3fn (or its uint8 bytes)")
    _check_dev(q, "q")
    _check_dev(scales, "scales", torch.float32, align=4)
    if block not in _FP8_BLOCKS:
        raise ValueError(f"block must be one of {_FP8_BLOCKS}")
    n = q.numel()
    if n % block or scales.numel() != n // block:
        raise ValueError("scales must hold one value per block of q")
    y = torch.empty(n, dtype=torch.bfloat16, device=q.device)
    _core.fp8_unpack(q.data_ptr(), scales.data_ptr(), n, y.data_ptr(), block, _stream())
    return y


def fp8_packed_size(src_bytes: int, chunk_bytes: int, block: int = 128) -> int:
    """Bytes of a bf16 layer of `src_bytes` in the chunked fp8 wire/HBM layout."""
    return _core.fp8_packed_size(src_bytes, chunk_bytes, block)


def fp8_pack_layer(x: torch.Tensor, chunk_bytes: int, block: int = 128) -> torch.Tensor:
    """A whole bf16 layer into the data engine's packed layout (core/fp8.h): per
    source chunk of `chunk_bytes`, [e4m3fn values][f32 scales]. Returns uint8."""
    _check_dev(x, "x", torch.bfloat16)
    src = _nbytes(x)
    if chunk_bytes <= 0 or chunk_bytes % 4096 or src % (2 * block):
        raise ValueError("chunk_bytes must be a positive multiple of 4096 and the layer a whole number of blocks")
    out = torch.empty(fp8_packed_size(src, chunk_bytes, block), dtype=torch.uint8, device=x.device)
    _core.fp8_pack_chunks(x.data_ptr(), src, chunk_bytes, block, out.data_ptr(), _stream())
    return out


def fp8_verify_unpack(packed: torch.Tensor, src_bytes: int, chunk_bytes: int,
                      block: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """One fused pass over a packed layer: CRC32C of every packed chunk and the
    dequantized bf16 layer. Returns (bf16 [src_bytes / 2], crcs int32 [chunks])."""
    _check_dev(packed, "packed", torch.uint8)
    if chunk_bytes <= 0 or chunk_bytes % 4096 or src_bytes % (2 * block) or block not in _FP8_BLOCKS:
        raise ValueError("bad chunk_bytes / src_bytes / block")
    pbytes = fp8_packed_size(src_bytes, chunk_bytes, block)
    if packed.numel() < pbytes:
        raise ValueError(f"packed holds {packed.numel()} bytes, the layout needs {pbytes}")
    pchunk = chunk_bytes // 2 + chunk_bytes // 2 // block * 4
    nchunks = (pbytes + pchunk - 1) // pchunk
    out = torch.empty(src_bytes // 2, dtype=torch.bfloat16, device=packed.device)
    crcs = torch.empty(nchunks, dtype=torch.int32, device=packed.device)
    ws = torch.zeros(_core.crc32c_workspace_bytes(pbytes, pchunk), dtype=torch.uint8, device=packed.device)
    _core.fp8_verify_unpack_async(packed.data_ptr(), src_bytes, chunk_bytes, block, out.data_ptr(), crcs.data_ptr(),
                                  ws.data_ptr(), _stream())
    return out, crcs


def fp8_verify_unpack_chunks(chunks: List[Tuple[torch.Tensor, int]], block: int = 128
                             ) -> Tuple[List[torch.Tensor], torch.Tensor]:
    """The engine's batched form: independent packed chunks [(packed uint8, src_len), ...]
    (each the core/fp8.h image of `src_len` bf16 bytes, up to `_core.crc32c_batch_max()`
    of them) checked and dequantized in ONE launch. Returns ([bf16 per chunk], crcs int32)."""
    if not chunks or len(chunks) > _core.crc32c_batch_max():
        raise ValueError(f"1 to {_core.crc32c_batch_max()} chunks per launch")
    if block not in _FP8_BLOCKS:
        raise ValueError(f"block must be one of {_FP8_BLOCKS}")
    outs, items = [], []
    dev = chunks[0][0].device
    for packed, src_len in chunks:
        _check_dev(packed, "packed", torch.uint8)
        if packed.device != dev:
            raise ValueError("every chunk of one launch must be on the same GPU")
        if src_len <= 0 or src_len % (2 * block):
            raise ValueError("src_len must be a positive multiple of 2 * block")
        need = src_len // 2 + src_len // 2 // block * 4
        if packed.numel() < need:
            raise ValueError(f"packed chunk holds {packed.numel()} bytes, its layout needs {need}")
        y = torch.empty(src_len // 2, dtype=torch.bfloat16, device=dev)
        outs.append(y)
        items.append((packed.data_ptr(), src_len, y.data_ptr()))
    crcs = torch.empty(len(chunks), dtype=torch.int32, device=dev)
    ws = torch.zeros(_core.crc32c_batch_workspace_bytes(), dtype=torch.uint8, device=dev)
    _core.fp8_verify_unpack_batch_async(items, block, crcs.data_ptr(), ws.data_ptr(), _stream())
    return outs, crcs


# ---- MXFP4 (core/mxfp4.h): e2m1 codes, two per byte, one E8M0 scale byte per 32 values

_MX_BLOCK = 32


def mxfp4_pack(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 -> MXFP4 (OCP MX): e2m1 codes, two per byte (element 2k in the low
    nibble), and one E8M0 scale byte per 32 values (2^E, the smallest E in
    [-126, 125] with the block's finite amax <= 6 * 2^E; core/mxfp4.h). Values
    round to the nearest code, ties to the even one; +-inf saturate to +-6 * 2^E;
    a block that holds a NaN is stored as scale 0xFF with zero codes.
    Returns (q: uint8 [n / 2], scales: uint8 [n / 32]);
    ``q.view(torch.float4_e2m1fn_x2)`` and ``scales.view(torch.float8_e8m0fnu)``
    are the matching torch dtypes."""
    _check_dev(x, "x", torch.bfloat16)
    n = x.numel()
    if n % _MX_BLOCK:
        raise ValueError(f"numel ({n}) must be a multiple of {_MX_BLOCK}")
    q = torch.empty(n // 2, dtype=torch.uint8, device=x.device)
    s = torch.empty(n // _MX_BLOCK, dtype=torch.uint8, device=x.device)
    _core.mxfp4_pack(x.data_ptr(), n, q.data_ptr(), s.data_ptr(), _stream())
    return q, s


def _as_bytes(t: torch.Tensor, name: str, other) -> torch.Tensor:
    if t.dtype == torch.uint8:
        return t
    if other is not None and t.dtype == other:
        return t.view(torch.uint8)
    raise ValueError(f"{name} must be uint8" + (f" or {other}" if other is not None else ""))


def mxfp4_unpack(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Inverse of `mxfp4_pack`: bf16 values code * 2^(scale - 127), exact (bf16
    subnormals included); scale 0xFF gives NaN (0x7FC0) for the whole block.
    `q` uint8 [n / 2] (or its ``torch.float4_e2m1fn_x2`` view), `scales` uint8
    [n / 32] (or its ``torch.float8_e8m0fnu`` view)."""
    q = _as_bytes(q, "q", getattr(torch, "float4_e2m1fn_x2", None))
    scales = _as_bytes(scales, "scales", getattr(torch, "float8_e8m0fnu", None))
    _check_dev(q, "q")
    _check_dev(scales, "scales", align=1)
    n = q.numel() * 2
    if n % _MX_BLOCK or scales.numel() != n // _MX_BLOCK:
        raise ValueError("scales must hold one byte per 16 bytes of q")
    y = torch.empty(n, dtype=torch.bfloat16, device=q.device)
    _core.mxfp4_unpack(q.data_ptr(), scales.data_ptr(), n, y.data_ptr(), _stream())
    return y


def mxfp4_packed_size(src_bytes: int, chunk_bytes: int) -> int:
    """Bytes of a bf16 layer of `src_bytes` in the chunked MXFP4 wire/HBM layout."""
    return _core.mxfp4_packed_size(src_bytes, chunk_bytes)


def mxfp4_pack_layer(x: torch.Tensor, chunk_bytes: int) -> torch.Tensor:
    """A whole bf16 layer into the data engine's packed layout (core/mxfp4.h): per
    source chunk of `chunk_bytes`, [e2m1 codes][E8M0 scales]. Returns uint8."""
    _check_dev(x, "x", torch.bfloat16)
    src = _nbytes(x)
    if chunk_bytes <= 0 or chunk_bytes % 4096 or src % (2 * _MX_BLOCK):
        raise ValueError("chunk_bytes must be a positive multiple of 4096 and the layer a multiple of 64 B")
    out = torch.empty(mxfp4_packed_size(src, chunk_bytes), dtype=torch.uint8, device=x.device)
    _core.mxfp4_pack_chunks(x.data_ptr(), src, chunk_bytes, out.data_ptr(), _stream())
    return out


def mxfp4_verify_unpack(packed: torch.Tensor, src_bytes: int, chunk_bytes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """One fused pass over an MXFP4-packed layer: CRC32C of every packed chunk and
    the dequantized bf16 layer. Returns (bf16 [src_bytes / 2], crcs int32 [chunks])."""
    _check_dev(packed, "packed", torch.uint8)
    if chunk_bytes <= 0 or chunk_bytes % 4096 or src_bytes <= 0 or src_bytes % (2 * _MX_BLOCK):
        raise ValueError("bad chunk_bytes / src_bytes")
    pbytes = mxfp4_packed_size(src_bytes, chunk_bytes)
    if packed.numel() < pbytes:
        raise ValueError(f"packed holds {packed.numel()} bytes, the layout needs {pbytes}")
    pchunk = chunk_bytes // 4 + chunk_bytes // 64
    nchunks = (pbytes + pchunk - 1) // pchunk
    out = torch.empty(src_bytes // 2, dtype=torch.bfloat16, device=packed.device)
    crcs = torch.empty(nchunks, dtype=torch.int32, device=packed.device)
    ws = torch.zeros(_core.crc32c_workspace_bytes(pbytes, pchunk), dtype=torch.uint8, device=packed.device)
    _core.mxfp4_verify_unpack_async(packed.data_ptr(), src_bytes, chunk_bytes, out.data_ptr(), crcs.data_ptr(),
                                    ws.data_ptr(), _stream())
    return out, crcs


def mxfp4_verify_unpack_chunks(chunks: List[Tuple[torch.Tensor, int]]) -> Tuple[List[torch.Tensor], torch.Tensor]:
    """The engine's batched form: independent packed chunks [(packed uint8, src_len), ...]
    (each the core/mxfp4.h image of `src_len` bf16 bytes, up to `_core.crc32c_batch_max()`
    of them) checked and dequantized in ONE launch. Returns ([bf16 per chunk], crcs int32)."""
    if not chunks or len(chunks) > _core.crc32c_batch_max():
        raise ValueError(f"1 to {_core.crc32c_batch_max()} chunks per launch")
    outs, items = [], []
    dev = chunks[0][0].device
    for packed, src_len in chunks:
        _check_dev(packed, "packed", torch.uint8)
        if packed.device != dev:
            raise ValueError("every chunk of one launch must be on the same GPU")
        if src_len <= 0 or src_len % (2 * _MX_BLOCK):
            raise ValueError("src_len must be a positive multiple of 64")
        need = src_len // 4 + src_len // 64
        if packed.numel() < need:
            raise ValueError(f"packed chunk holds {packed.numel()} bytes, its layout needs {need}")
        y = torch.empty(src_len // 2, dtype=torch.bfloat16, device=dev)
        outs.append(y)
        items.append((packed.data_ptr(), src_len, y.data_ptr()))
    crcs = torch.empty(len(chunks), dtype=torch.int32, device=dev)
    ws = torch.zeros(_core.crc32c_batch_workspace_bytes(), dtype=torch.uint8, device=dev)
    _core.mxfp4_verify_unpack_batch_async(items, crcs.data_ptr(), ws.data_ptr(), _stream())
    return outs, crcs


# ---- consumers of a packed layer in place: a parameter is the elements
# [elem_offset, elem_offset + numel) of the layer (core/mxfp4.h unpack_range_host)

def _check_packed_layer(packed: torch.Tensor, src_bytes: int, chunk_bytes: int) -> int:
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("packed must be a contiguous 1-D uint8 tensor")
    if chunk_bytes <= 0 or chunk_bytes % 1024 or src_bytes <= 0 or src_bytes % (2 * _MX_BLOCK):
        raise ValueError("chunk_bytes must be a positive multiple of 1024 and src_bytes a positive multiple of 64")
    need = mxfp4_packed_size(src_bytes, chunk_bytes)
    if packed.numel() < need:
        raise ValueError(f"packed holds {packed.numel()} bytes, the layout needs {need}")
    if packed.is_cuda and packed.data_ptr() % 16:
        raise ValueError("packed must be 16-byte aligned")
    return need


def _check_range(src_bytes: int, elem_offset: int, n: int) -> None:
    if elem_offset < 0 or n < 0 or elem_offset % _MX_BLOCK or n % _MX_BLOCK:
        raise ValueError(f"elem_offset and the element count must be non-negative multiples of {_MX_BLOCK}")
    if elem_offset + n > src_bytes // 2:
        raise ValueError(f"elements [{elem_offset}, {elem_offset + n}) lie outside a layer of {src_bytes // 2}")


def mxfp4_unpack_range(packed: torch.Tensor, src_bytes: int, chunk_bytes: int, elem_offset: int, n: int) -> torch.Tensor:
    """Elements [elem_offset, elem_offset + n) of an MXFP4-packed layer (the chunked
    layout of `mxfp4_pack_layer`) as bf16 [n], on `packed`'s device. Offset and
    count are multiples of 32. GPU: the unpack kernel once per source chunk the
    range touches, on the current stream; CPU: the host reference."""
    _check_packed_layer(packed, src_bytes, chunk_bytes)
    _check_range(src_bytes, elem_offset, n)
    out = torch.empty(n, dtype=torch.bfloat16, device=packed.device)
    if n == 0:
        return out
    if not packed.is_cuda:
        _core.mxfp4_unpack_range_host(packed.data_ptr(), packed.numel(), src_bytes, chunk_bytes, elem_offset, n,
                                      out.data_ptr())
        return out
    total, ce, pchunk = src_bytes // 2, chunk_bytes // 2, chunk_bytes // 4 + chunk_bytes // 64
    e, end, stream = elem_offset, elem_offset + n, _stream()
    while e < end:
        c, r = divmod(e, ce)
        nc = min(ce, total - c * ce)
        take = min(end - e, nc - r)
        base = packed.data_ptr() + c * pchunk
        # r and e - elem_offset are multiples of 32: q 16-B, the output 64-B aligned
        _core.mxfp4_unpack(base + r // 2, base + nc // 2 + r // _MX_BLOCK, take, out.data_ptr() + 2 * (e - elem_offset),
                           stream)
        e += take
    return out


# ---- MXFP6 (core/mxfp6.h): e2m3 codes, 24 bytes per 32 values (value i at bits
# [6i, 6i + 6) of its block), one E8M0 scale byte per 32 values

_MX6_BLOCK_BYTES = 24


def _on_cpu(t: torch.Tensor, name: str, dtype=None) -> bool:
    """True for a CPU tensor (checked like _check_dev's, without device or alignment)."""
    if t.is_cuda:
        return False
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    return True


def mxfp6_pack(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 -> MXFP6 (OCP MX, e2m3): 24 bytes of 6-bit codes per 32 values (value i
    of a block at bits [6i, 6i + 6) of its 24 bytes read as one little-endian
    integer) and one E8M0 scale byte per 32 values (2^E, the smallest E in
    [-126, 125] with the block's finite amax <= 7.5 * 2^E; core/mxfp6.h). Values
    round to the nearest code, ties to the even one; +-inf saturate to
    +-7.5 * 2^E; a block that holds a NaN is stored as scale 0xFF with zero codes.
    Returns (q: uint8 [3 n / 4], scales: uint8 [n / 32]). CPU tensors go through
    the host reference."""
    cpu = _on_cpu(x, "x", torch.bfloat16)
    if not cpu:
        _check_dev(x, "x", torch.bfloat16)
    n = x.numel()
    if n % _MX_BLOCK:
        raise ValueError(f"numel ({n}) must be a multiple of {_MX_BLOCK}")
    if cpu:
        qb, sb = _core.mxfp6_pack_host(x.view(torch.int16).numpy().tobytes())
        return torch.frombuffer(bytearray(qb), dtype=torch.uint8), torch.frombuffer(bytearray(sb), dtype=torch.uint8)
    q = torch.empty(n // _MX_BLOCK * _MX6_BLOCK_BYTES, dtype=torch.uint8, device=x.device)
    s = torch.empty(n // _MX_BLOCK, dtype=torch.uint8, device=x.device)
    _core.mxfp6_pack(x.data_ptr(), n, q.data_ptr(), s.data_ptr(), _stream())
    return q, s


def mxfp6_unpack(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Inverse of `mxfp6_pack`: bf16 values code * 2^(scale - 127), exact (bf16
    subnormals included); scale 0xFF gives NaN (0x7FC0) for the whole block.
    `q` uint8 [3 n / 4], `scales` uint8 [n / 32] (or its ``torch.float8_e8m0fnu``
    view). CPU tensors go through the host reference."""
    q = _as_bytes(q, "q", None)
    scales = _as_bytes(scales, "scales", getattr(torch, "float8_e8m0fnu", None))
    cpu = _on_cpu(q, "q")
    if cpu:
        _on_cpu(scales, "scales")
    else:
        _check_dev(q, "q", align=8)
        _check_dev(scales, "scales", align=1)
    if q.device != scales.device:
        raise ValueError("q and scales must be on the same device")
    if q.numel() % _MX6_BLOCK_BYTES or scales.numel() != q.numel() // _MX6_BLOCK_BYTES:
        raise ValueError("scales must hold one byte per 24 bytes of q")
    n = scales.numel() * _MX_BLOCK
    if cpu:
        out = _core.mxfp6_unpack_host(q.numpy().tobytes(), scales.numpy().tobytes())
        return torch.frombuffer(bytearray(out), dtype=torch.bfloat16) if n else torch.empty(0, dtype=torch.bfloat16)
    y = torch.empty(n, dtype=torch.bfloat16, device=q.device)
    _core.mxfp6_unpack(q.data_ptr(), scales.data_ptr(), n, y.data_ptr(), _stream())
    return y


def mxfp6_packed_size(src_bytes: int, chunk_bytes: int) -> int:
    """Bytes of a bf16 layer of `src_bytes` in the chunked MXFP6 wire/HBM layout (25/64)."""
    return _core.mxfp6_packed_size(src_bytes, chunk_bytes)


def mxfp6_pack_layer(x: torch.Tensor, chunk_bytes: int) -> torch.Tensor:
    """A whole bf16 layer into the data engine's packed layout (core/mxfp6.h): per
    source chunk of `chunk_bytes`, [e2m3 blocks][E8M0 scales]. Returns uint8. CPU
    tensors go through the host reference."""
    cpu = _on_cpu(x, "x", torch.bfloat16)
    if not cpu:
        _check_dev(x, "x", torch.bfloat16)
    src = _nbytes(x)
    if chunk_bytes <= 0 or chunk_bytes % 4096 or src % (2 * _MX_BLOCK):
        raise ValueError("chunk_bytes must be a positive multiple of 4096 and the layer a multiple of 64 B")
    out = torch.empty(mxfp6_packed_size(src, chunk_bytes), dtype=torch.uint8, device=x.device)
    if cpu:
        _core.mxfp6_pack_layer_into(x.data_ptr(), src, chunk_bytes, out.data_ptr())
    else:
        _core.mxfp6_pack_chunks(x.data_ptr(), src, chunk_bytes, out.data_ptr(), _stream())
    return out


def mxfp6_verify_unpack(packed: torch.Tensor, src_bytes: int, chunk_bytes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """CRC32C of every packed chunk of an MXFP6-packed layer and the dequantized
    bf16 layer: the CRC walk, then the unpack kernel, on the current stream (the
    packed bytes are read twice; kernels/mxfp6.hip).
    Returns (bf16 [src_bytes / 2], crcs int32 [chunks])."""
    _check_dev(packed, "packed", torch.uint8)
    if chunk_bytes <= 0 or chunk_bytes % 4096 or src_bytes <= 0 or src_bytes % (2 * _MX_BLOCK):
        raise ValueError("bad chunk_bytes / src_bytes")
    pbytes = mxfp6_packed_size(src_bytes, chunk_bytes)
    if packed.numel() < pbytes:
        raise ValueError(f"packed holds {packed.numel()} bytes, the layout needs {pbytes}")
    pchunk = chunk_bytes // 64 * 25
    nchunks = (pbytes + pchunk - 1) // pchunk
    out = torch.empty(src_bytes // 2, dtype=torch.bfloat16, device=packed.device)
    crcs = torch.empty(nchunks, dtype=torch.int32, device=packed.device)
    ws = torch.zeros(_core.crc32c_workspace_bytes(pbytes, pchunk), dtype=torch.uint8, device=packed.device)
    _core.mxfp6_verify_unpack_async(packed.data_ptr(), src_bytes, chunk_bytes, out.data_ptr(), crcs.data_ptr(),
                                    ws.data_ptr(), _stream())
    return out, crcs


def mxfp6_verify_unpack_chunks(chunks: List[Tuple[torch.Tensor, int]]) -> Tuple[List[torch.Tensor], torch.Tensor]:
    """The engine's batched form: independent packed chunks [(packed uint8, src_len), ...]
    (each the core/mxfp6.h image of `src_len` bf16 bytes, up to `_core.crc32c_batch_max()`
    of them) checked in one CRC launch and dequantized in one unpack launch.
    Returns ([bf16 per chunk], crcs int32)."""
    if not chunks or len(chunks) > _core.crc32c_batch_max():
        raise ValueError(f"1 to {_core.crc32c_batch_max()} chunks per launch")
    outs, items = [], []
    dev = chunks[0][0].device
    for packed, src_len in chunks:
        _check_dev(packed, "packed", torch.uint8)
        if packed.device != dev:
            raise ValueError("every chunk of one launch must be on the same GPU")
        if src_len <= 0 or src_len % (2 * _MX_BLOCK):
            raise ValueError("src_len must be a positive multiple of 64")
        need = src_len // 64 * 25
        if packed.numel() < need:
            raise ValueError(f"packed chunk holds {packed.numel()} bytes, its layout needs {need}")
        y = torch.empty(src_len // 2, dtype=torch.bfloat16, device=dev)
        outs.append(y)
        items.append((packed.data_ptr(), src_len, y.data_ptr()))
    crcs = torch.empty(len(chunks), dtype=torch.int32, device=dev)
    ws = torch.zeros(_core.crc32c_batch_workspace_bytes(), dtype=torch.uint8, device=dev)
    _core.mxfp6_verify_unpack_batch_async(items, crcs.data_ptr(), ws.data_ptr(), _stream())
    return outs, crcs


def _check_mxfp6_layer(packed: torch.Tensor, src_bytes: int, chunk_bytes: int) -> int:
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("packed must be a contiguous 1-D uint8 tensor")
    if chunk_bytes <= 0 or chunk_bytes % 1024 or src_bytes <= 0 or src_bytes % (2 * _MX_BLOCK):
        raise ValueError("chunk_bytes must be a positive multiple of 1024 and src_bytes a positive multiple of 64")
    need = mxfp6_packed_size(src_bytes, chunk_bytes)
    if packed.numel() < need:
        raise ValueError(f"packed holds {packed.numel()} bytes, the layout needs {need}")
    if packed.is_cuda and packed.data_ptr() % 16:
        raise ValueError("packed must be 16-byte aligned")
    return need


def mxfp6_unpack_range(packed: torch.Tensor, src_bytes: int, chunk_bytes: int, elem_offset: int, n: int) -> torch.Tensor:
    """Elements [elem_offset, elem_offset + n) of an MXFP6-packed layer (the chunked
    layout of `mxfp6_pack_layer`) as bf16 [n], on `packed`'s device. Offset and
    count are multiples of 32. GPU: the unpack kernel once per source chunk the
    range touches, on the current stream; CPU: the host reference."""
    _check_mxfp6_layer(packed, src_bytes, chunk_bytes)
    _check_range(src_bytes, elem_offset, n)
    out = torch.empty(n, dtype=torch.bfloat16, device=packed.device)
    if n == 0:
        return out
    if not packed.is_cuda:
        _core.mxfp6_unpack_range_host(packed.data_ptr(), packed.numel(), src_bytes, chunk_bytes, elem_offset, n,
                                      out.data_ptr())
        return out
    total, ce, pchunk = src_bytes // 2, chunk_bytes // 2, chunk_bytes // 64 * 25
    e, end, stream = elem_offset, elem_offset + n, _stream()
    while e < end:
        c, r = divmod(e, ce)
        nc = min(ce, total - c * ce)
        take = min(end - e, nc - r)
        base = packed.data_ptr() + c * pchunk
        # r and e - elem_offset are multiples of 32: q 8-B, the output 64-B aligned
        _core.mxfp6_unpack(base + r // _MX_BLOCK * _MX6_BLOCK_BYTES,
                           base + nc // _MX_BLOCK * _MX6_BLOCK_BYTES + r // _MX_BLOCK, take,
                           out.data_ptr() + 2 * (e - elem_offset), stream)
        e += take
    return out


# ---- MXFP8 activations (core/mxfp8_act.h): e4m3fn codes and one E8M0 scale byte per 32
# values along the last dimension, the x side of the W4A8 route (act="mxfp8")

def mxfp8_quantize_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 `x` [..., K] (K a multiple of 32) -> (codes uint8 [..., K], scales uint8
    [..., K / 32]): OCP e4m3fn codes and one E8M0 byte per 32 values along K. Scale,
    codes, saturation (+-inf become the largest code) and NaN (0x7F | sign) are those
    of `fp8_pack(x, block=32)`, byte for byte, and the scale byte is the exponent of
    its f32 scale; the value is ``code * 2**(byte - 127)``. GPU: one launch on the
    current stream for any number of rows; CPU: the host codec, the same bytes."""
    if x.dtype != torch.bfloat16:
        raise ValueError(f"x must be {torch.bfloat16}, got {x.dtype}")
    if x.dim() < 1 or x.shape[-1] <= 0 or x.shape[-1] % _MX_BLOCK or x.numel() == 0:
        raise ValueError(f"x must be [..., K] with K a positive multiple of {_MX_BLOCK} and at least one row, "
                         f"got {tuple(x.shape)}")
    k = x.shape[-1]
    x2 = x.reshape(-1, k)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if x2.data_ptr() % 16:
        x2 = x2.clone()
    m = x2.shape[0]
    codes = torch.empty(m, k, dtype=torch.uint8, device=x.device)
    scales = torch.empty(m, k // _MX_BLOCK, dtype=torch.uint8, device=x.device)
    if x.is_cuda:
        _core.mxfp8_quantize_rows(x2.data_ptr(), m, k, codes.data_ptr(), scales.data_ptr(), _stream())
    else:
        _core.mxfp8_quantize_rows_host(x2.data_ptr(), m * k, codes.data_ptr(), scales.data_ptr())
    return codes.view(*x.shape[:-1], k), scales.view(*x.shape[:-1], k // _MX_BLOCK)


def _mxfp8_values(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """code * 2^(byte - 127) as f32 [rows, K]: exact (at most 2^-135, at least 448 * 2^120)."""
    k = codes.shape[-1]
    v = codes.reshape(-1, k // _MX_BLOCK, _MX_BLOCK).view(torch.float8_e4m3fn).float()
    return torch.ldexp(v, scales.reshape(-1, k // _MX_BLOCK, 1).to(torch.int32) - 127).view(-1, k)


def _check_act(act: Optional[str], split_k: int, row_tiles: int) -> None:
    if act is None:
        return
    if act != "mxfp8":
        raise ValueError(f"act must be None or 'mxfp8', got {act!r}")
    if split_k:
        raise ValueError("split_k must be 0 with act='mxfp8': the native kernel never splits K")
    if row_tiles:
        raise ValueError("row_tiles must be 0 with act='mxfp8': the native kernel has one tile shape")


def _check_tiled(tiled: bool, split_k: int, row_tiles: int) -> None:
    if tiled and split_k:
        raise ValueError("split_k must be 0 with tiled=True: the tiled kernel never splits K")
    if tiled and row_tiles:
        raise ValueError("row_tiles must be 0 with tiled=True: the tiled kernel has one tile shape")


def mxfp4_linear(x: torch.Tensor, packed: torch.Tensor, out_features: int, in_features: int, *, src_bytes: int,
                 chunk_bytes: int, elem_offset: int = 0, out_dtype: torch.dtype = torch.bfloat16,
                 split_k: int = 0, row_tiles: int = 0, out: Optional[torch.Tensor] = None,
                 tiled: bool = False, act: Optional[str] = None) -> torch.Tensor:
    """``x @ W.T`` for a bf16 `x` [..., in_features] and the [out_features, in_features]
    weight stored as elements [elem_offset, ...) of the MXFP4-packed layer `packed`
    (`src_bytes` of bf16 in chunks of `chunk_bytes`, the layout of `mxfp4_pack_layer`).

    GPU: one kernel on the current stream reads the codes and scales where they
    lie, dequantizes in registers and accumulates in f32 on the bf16 MFMA; no bf16
    copy of the weight is made. The result is deterministic (`split_k`, 0 = chosen
    from the shape, is the number of K slices reduced in a fixed order; `row_tiles`,
    0 = chosen from the shape, the 16-row tiles of W a wave feeds from one x fragment).
    CPU: the host reference dequantizes the range, then ``F.linear`` - in f32 for an
    f32 result, in bf16 (what a plain bf16 weight gets) for a bf16 one.
    in_features and elem_offset are multiples of 32, out_features of 16.
    `out` (GPU only): a [rows, out_features] f32 or bf16 tensor to write, unit
    stride along its rows and any row stride; its dtype replaces `out_dtype`.
    `tiled` (GPU; the CPU route is the same either way): the kernel for many rows
    (mxfp4_tiled.hip) - one launch for any number of rows, x shared through LDS, W
    read once per `_core.mxfp4_tiled_tile()[0]` rows instead of once per 64. K is
    never split there, so a row of the result depends on that row of x alone (the
    same bits in any batch); `split_k` and `row_tiles` must stay 0.
    `act="mxfp8"` (opt-in, W4A8): x is quantized to MXFP8 (`mxfp8_quantize_rows`) on
    the current stream and the product runs on the block-scaled MFMA
    (mxfp4_mx.hip), codes and scale bytes of both sides as they lie in memory: two
    launches for any number of rows. The result is ``sum_k x^[m][k] * w^[n][k]`` with
    x^ the quantized activation, one f32 accumulator per element walking K in
    ascending order (batch invariant like the tiled kernel). It is the only kernel
    for `act`, so `tiled` may be either and `split_k` and `row_tiles` must stay 0.
    +-inf in x saturates to the largest code of its block (core/fp8.h) where the
    W4A16 kernels carry it through; a NaN in x gives a NaN row; a weight block with
    scale byte 0xFF gives a NaN column. The instruction drops a product 2^14 or
    more below the largest of its group of 8 consecutive k, so the kernel issues
    three MFMAs per step, one per exponent class of x^ (mxfp4_mx.hip's header):
    the result is an f32-accurate sum also on inputs with outliers, at a third of
    the instruction's rate. CPU: the host codec,
    x^ and w^ in f32, ``F.linear`` in f32; a bf16 result is that rounded once.
    The CPU route's w^ is the bf16 of `mxfp4_unpack_range`, the GPU multiplies
    ``code * 2**(byte - 127)``: the two are equal for every code under every scale
    byte 0..254 except the 12 pairs that reach 2**128 (the magnitudes 4 and 6, i.e.
    nibbles 6 and 7, under byte 253; 2, 3, 4 and 6, nibbles 4..7, under byte 254;
    either sign), which are +-inf on the CPU route."""
    _check_tiled(tiled, split_k, row_tiles)
    _check_act(act, split_k, row_tiles)
    if out is not None:
        out_dtype = out.dtype
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"x must be {torch.bfloat16}, got {x.dtype}")
    n, k = int(out_features), int(in_features)
    if n <= 0 or n % 16 or k <= 0 or k % _MX_BLOCK:
        raise ValueError("out_features must be a positive multiple of 16 and in_features of 32")
    if x.dim() < 1 or x.shape[-1] != k or x.numel() == 0:
        raise ValueError(f"x must be [..., {k}] with at least one row, got {tuple(x.shape)}")
    if x.device != packed.device:
        raise ValueError("x and packed must be on the same device")
    if not 0 <= split_k <= 16:
        raise ValueError("split_k must be in 0..16")
    if row_tiles not in (0, 1, 2, 4) or (row_tiles and n // 16 % row_tiles):
        raise ValueError("row_tiles must be 0, 1, 2 or 4 and divide out_features / 16")
    _check_packed_layer(packed, src_bytes, chunk_bytes)
    _check_range(src_bytes, elem_offset, n * k)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, k)
    if not x.is_cuda:
        if out is not None:
            raise ValueError("out is for GPU tensors")
        w = mxfp4_unpack_range(packed, src_bytes, chunk_bytes, elem_offset, n * k).view(n, k)
        if act is not None:
            y = torch.nn.functional.linear(_mxfp8_values(*mxfp8_quantize_rows(x2)), w.float()).to(out_dtype)
        elif out_dtype == torch.float32:
            y = torch.nn.functional.linear(x2.float(), w.float())
        else:
            y = torch.nn.functional.linear(x2, w)
        return y.view(*lead, n)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if x2.data_ptr() % 16:
        x2 = x2.clone()
    m = x2.shape[0]
    if out is None:
        y = torch.empty(m, n, dtype=out_dtype, device=x.device)
    else:
        y = out
        if y.device != x.device or tuple(y.shape) != (m, n) or y.stride(1) != 1 or y.stride(0) < n:
            raise ValueError(f"out must be [{m}, {n}] on x's device with unit stride along rows")
    if act is not None:
        xq, xs = mxfp8_quantize_rows(x2)
        _core.mxfp4_linear_mx(packed.data_ptr(), src_bytes, chunk_bytes, elem_offset, xq.data_ptr(), xs.data_ptr(), m,
                              n, k, y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, _stream())
        return y if out is not None else y.view(*lead, n)
    if tiled:
        _core.mxfp4_linear_tiled(packed.data_ptr(), src_bytes, chunk_bytes, elem_offset, x2.data_ptr(), m, n, k,
                                 y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, _stream())
        return y if out is not None else y.view(*lead, n)
    _core.mxfp4_linear(packed.data_ptr(), src_bytes, chunk_bytes, elem_offset, x2.data_ptr(), m, n, k, y.data_ptr(),
                       y.stride(0), out_dtype == torch.bfloat16, split_k, row_tiles, _stream())
    return y if out is not None else y.view(*lead, n)


def _check_fp8_layer(packed: torch.Tensor, src_bytes: int, chunk_bytes: int, block: int) -> int:
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("packed must be a contiguous 1-D uint8 tensor")
    if block not in _FP8_BLOCKS:
        raise ValueError(f"block must be one of {_FP8_BLOCKS}")
    if chunk_bytes <= 0 or chunk_bytes % (8 * block):
        raise ValueError(f"chunk_bytes must be a positive multiple of 8 * block ({8 * block}): packed chunks "
                         "then start 16-byte aligned")
    if src_bytes <= 0 or src_bytes % (2 * block):
        raise ValueError(f"src_bytes must be a positive multiple of 2 * block ({2 * block})")
    need = fp8_packed_size(src_bytes, chunk_bytes, block)
    if packed.numel() < need:
        raise ValueError(f"packed holds {packed.numel()} bytes, the layout needs {need}")
    if packed.is_cuda and packed.data_ptr() % 16:
        raise ValueError("packed must be 16-byte aligned")
    return need


def fp8_unpack_range(packed: torch.Tensor, src_bytes: int, chunk_bytes: int, elem_offset: int, n: int,
                     block: int = 128) -> torch.Tensor:
    """Elements [elem_offset, elem_offset + n) of an fp8-packed layer (the chunked
    layout of `fp8_pack_layer`) as bf16 [n], on `packed`'s device. Offset and count
    are multiples of 32. GPU: the unpack kernel once per piece of a source chunk the
    range touches (the whole blocks of the chunk in one launch; where the range starts
    or ends inside a scale block, that part in power-of-two pieces), on the current
    stream; CPU: the host reference."""
    _check_fp8_layer(packed, src_bytes, chunk_bytes, block)
    _check_range(src_bytes, elem_offset, n)
    out = torch.empty(n, dtype=torch.bfloat16, device=packed.device)
    if n == 0:
        return out
    if not packed.is_cuda:
        _core.fp8_unpack_range_host(packed.data_ptr(), packed.numel(), src_bytes, chunk_bytes, block, elem_offset, n,
                                    out.data_ptr())
        return out
    total, ce = src_bytes // 2, chunk_bytes // 2
    pchunk = ce + ce // block * 4
    e, end, stream = elem_offset, elem_offset + n, _stream()
    while e < end:
        c, r = divmod(e, ce)
        nc = min(ce, total - c * ce)
        lim = min(end - e, nc - r)
        if r % block == 0 and lim >= block:
            take, blk = lim // block * block, block  # whole scale blocks
        else:
            # part of one scale block: the kernel wants whole blocks, so a power-of-two piece
            # (32 at least) goes as one block of its own length with that block's scale
            take = blk = 1 << (min(lim, block - r % block).bit_length() - 1)
        base = packed.data_ptr() + c * pchunk
        # r and e - elem_offset are multiples of 32: q 16-B (at least), the output 64-B aligned
        _core.fp8_unpack(base + r, base + nc + 4 * (r // block), take, out.data_ptr() + 2 * (e - elem_offset), blk,
                         stream)
        e += take
    return out


def fp8_linear(x: torch.Tensor, packed: torch.Tensor, out_features: int, in_features: int, *, src_bytes: int,
               chunk_bytes: int, block: int = 128, elem_offset: int = 0, out_dtype: torch.dtype = torch.bfloat16,
               split_k: int = 0, row_tiles: int = 0, out: Optional[torch.Tensor] = None,
               tiled: bool = False) -> torch.Tensor:
    """``x @ W.T`` for a bf16 `x` [..., in_features] and the [out_features, in_features]
    weight stored as elements [elem_offset, ...) of the fp8-packed layer `packed`
    (`src_bytes` of bf16 in chunks of `chunk_bytes` with one scale per `block` elements,
    the layout of `fp8_pack_layer`).

    GPU: one kernel on the current stream reads the e4m3 codes and the block scales
    where they lie, dequantizes in registers and accumulates in f32 on the bf16 MFMA;
    no bf16 copy of the weight is made. `split_k`, `row_tiles`, `out` and the
    determinism are `mxfp4_linear`'s. CPU: the host reference dequantizes the range,
    then ``F.linear`` - in f32 for an f32 result, in bf16 for a bf16 one.
    in_features and elem_offset are multiples of 32, out_features of 16, and
    chunk_bytes of 8 * block (every packed chunk then starts 16-byte aligned; the
    engine's chunk sizes do).
    `tiled` as in `mxfp4_linear`: the kernel for many rows (fp8_tiled.hip), one launch
    for any number of rows, W read once per `_core.fp8_tiled_tile()[0]` rows. Its f32
    result is bit for bit the untiled kernel's with ``split_k=1``."""
    _check_tiled(tiled, split_k, row_tiles)
    if out is not None:
        out_dtype = out.dtype
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"x must be {torch.bfloat16}, got {x.dtype}")
    n, k = int(out_features), int(in_features)
    if n <= 0 or n % 16 or k <= 0 or k % 32:
        raise ValueError("out_features must be a positive multiple of 16 and in_features of 32")
    if x.dim() < 1 or x.shape[-1] != k or x.numel() == 0:
        raise ValueError(f"x must be [..., {k}] with at least one row, got {tuple(x.shape)}")
    if x.device != packed.device:
        raise ValueError("x and packed must be on the same device")
    if not 0 <= split_k <= 16:
        raise ValueError("split_k must be in 0..16")
    if row_tiles not in (0, 1, 2, 4) or (row_tiles and n // 16 % row_tiles):
        raise ValueError("row_tiles must be 0, 1, 2 or 4 and divide out_features / 16")
    _check_fp8_layer(packed, src_bytes, chunk_bytes, block)
    _check_range(src_bytes, elem_offset, n * k)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, k)
    if not x.is_cuda:
        if out is not None:
            raise ValueError("out is for GPU tensors")
        w = fp8_unpack_range(packed, src_bytes, chunk_bytes, elem_offset, n * k, block).view(n, k)
        if out_dtype == torch.float32:
            y = torch.nn.functional.linear(x2.float(), w.float())
        else:
            y = torch.nn.functional.linear(x2, w)
        return y.view(*lead, n)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if x2.data_ptr() % 16:
        x2 = x2.clone()
    m = x2.shape[0]
    if out is None:
        y = torch.empty(m, n, dtype=out_dtype, device=x.device)
    else:
        y = out
        if y.device != x.device or tuple(y.shape) != (m, n) or y.stride(1) != 1 or y.stride(0) < n:
            raise ValueError(f"out must be [{m}, {n}] on x's device with unit stride along rows")
    if tiled:
        _core.fp8_linear_tiled(packed.data_ptr(), src_bytes, chunk_bytes, block, elem_offset, x2.data_ptr(), m, n, k,
                               y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, _stream())
        return y if out is not None else y.view(*lead, n)
    _core.fp8_linear(packed.data_ptr(), src_bytes, chunk_bytes, block, elem_offset, x2.data_ptr(), m, n, k,
                     y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, split_k, row_tiles, _stream())
    return y if out is not None else y.view(*lead, n)


def mxfp6_linear(x: torch.Tensor, packed: torch.Tensor, out_features: int, in_features: int, *, src_bytes: int,
                 chunk_bytes: int, elem_offset: int = 0, out_dtype: torch.dtype = torch.bfloat16,
                 split_k: int = 0, row_tiles: int = 0, out: Optional[torch.Tensor] = None,
                 tiled: bool = False) -> torch.Tensor:
    """``x @ W.T`` for a bf16 `x` [..., in_features] and the [out_features, in_features]
    weight stored as elements [elem_offset, ...) of the MXFP6-packed layer `packed`
    (`src_bytes` of bf16 in chunks of `chunk_bytes`, the layout of `mxfp6_pack_layer`).

    GPU: one kernel on the current stream reads the 24-byte blocks of e2m3 codes and
    their E8M0 scale bytes where they lie, dequantizes a block per instruction in
    registers and accumulates in f32 on the bf16 MFMA; no bf16 copy of the weight is
    made. `split_k`, `row_tiles`, `out` and the determinism are `mxfp4_linear`'s.
    CPU: the host reference dequantizes the range, then ``F.linear`` - in f32 for an
    f32 result, in bf16 for a bf16 one.
    in_features and elem_offset are multiples of 32, out_features of 16, and
    chunk_bytes of 1024 (every packed chunk then starts 16-byte aligned).
    `tiled` as in `mxfp4_linear`: the kernel for many rows (mxfp6_tiled.hip), one launch
    for any number of rows, W read once per `_core.mxfp6_tiled_tile()[0]` rows. Its f32
    result is bit for bit the untiled kernel's with ``split_k=1``."""
    _check_tiled(tiled, split_k, row_tiles)
    if out is not None:
        out_dtype = out.dtype
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"x must be {torch.bfloat16}, got {x.dtype}")
    n, k = int(out_features), int(in_features)
    if n <= 0 or n % 16 or k <= 0 or k % _MX_BLOCK:
        raise ValueError("out_features must be a positive multiple of 16 and in_features of 32")
    if x.dim() < 1 or x.shape[-1] != k or x.numel() == 0:
        raise ValueError(f"x must be [..., {k}] with at least one row, got {tuple(x.shape)}")
    if x.device != packed.device:
        raise ValueError("x and packed must be on the same device")
    if not 0 <= split_k <= 16:
        raise ValueError("split_k must be in 0..16")
    if row_tiles not in (0, 1, 2, 4) or (row_tiles and n // 16 % row_tiles):
        raise ValueError("row_tiles must be 0, 1, 2 or 4 and divide out_features / 16")
    _check_mxfp6_layer(packed, src_bytes, chunk_bytes)
    _check_range(src_bytes, elem_offset, n * k)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, k)
    if not x.is_cuda:
        if out is not None:
            raise ValueError("out is for GPU tensors")
        w = mxfp6_unpack_range(packed, src_bytes, chunk_bytes, elem_offset, n * k).view(n, k)
        if out_dtype == torch.float32:
            y = torch.nn.functional.linear(x2.float(), w.float())
        else:
            y = torch.nn.functional.linear(x2, w)
        return y.view(*lead, n)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if x2.data_ptr() % 16:
        x2 = x2.clone()
    m = x2.shape[0]
    if out is None:
        y = torch.empty(m, n, dtype=out_dtype, device=x.device)
    else:
        y = out
        if y.device != x.device or tuple(y.shape) != (m, n) or y.stride(1) != 1 or y.stride(0) < n:
            raise ValueError(f"out must be [{m}, {n}] on x's device with unit stride along rows")
    if tiled:
        _core.mxfp6_linear_tiled(packed.data_ptr(), src_bytes, chunk_bytes, elem_offset, x2.data_ptr(), m, n, k,
                                 y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, _stream())
        return y if out is not None else y.view(*lead, n)
    _core.mxfp6_linear(packed.data_ptr(), src_bytes, chunk_bytes, elem_offset, x2.data_ptr(), m, n, k, y.data_ptr(),
                       y.stride(0), out_dtype == torch.bfloat16, split_k, row_tiles, _stream())
    return y if out is not None else y.view(*lead, n)


def mxfp4_swiglu(x: torch.Tensor, packed: torch.Tensor, out_features: int, in_features: int, *, src_bytes: int,
                 chunk_bytes: int, gate_offset: int, up_offset: int, out_dtype: torch.dtype = torch.bfloat16,
                 split_k: int = 0, row_tiles: int = 0, out: Optional[torch.Tensor] = None,
                 tiled: bool = False, act: Optional[str] = None) -> torch.Tensor:
    """``silu(x @ Wg.T) * (x @ Wu.T)``, the front half of a gated MLP, for a bf16 `x`
    [..., in_features] and two [out_features, in_features] weights stored as elements
    [gate_offset, ...) and [up_offset, ...) of the MXFP4-packed layer `packed` (as in
    `mxfp4_linear`; the offsets are independent multiples of 32, in any order).

    GPU: one kernel on the current stream reads x once and both weights where they
    lie; the two products are `mxfp4_linear`'s sums (with equal `split_k` bit for
    bit its f32 results) and stay in the MFMA accumulators, ``(g / (1 + expf(-g))) * u``
    is evaluated in f32 and only the result is written, rounded once. `split_k`
    as in `mxfp4_linear`; `row_tiles` (0 = chosen from the shape, 1 or 2): the pairs
    of a gate and an up tile a wave feeds from one x fragment.
    CPU: the host reference dequantizes both ranges, then
    ``F.silu(F.linear(x, wg)) * F.linear(x, wu)`` - in f32 for an f32 result, in bf16
    (what plain bf16 weights get, op for op) for a bf16 one.
    `out` (GPU only) as in `mxfp4_linear`. `tiled` as in `mxfp4_linear`: the gated
    kernel for many rows, whose g and u are bit for bit the tiled linear's f32 results.
    `act="mxfp8"` as in `mxfp4_linear` (quantize, then the gated kernel of
    mxfp4_mx.hip: two launches): g and u are bit for bit the f32 results of
    `mxfp4_linear(..., act="mxfp8")`, with its handling of +-inf, NaN and 0xFF scale
    bytes; the epilogue is the same. CPU: x^, wg^ and wu^ in f32, the expression above
    in f32; a bf16 result is that rounded once."""
    _check_tiled(tiled, split_k, row_tiles)
    _check_act(act, split_k, row_tiles)
    if out is not None:
        out_dtype = out.dtype
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"x must be {torch.bfloat16}, got {x.dtype}")
    n, k = int(out_features), int(in_features)
    if n <= 0 or n % 16 or k <= 0 or k % _MX_BLOCK:
        raise ValueError("out_features must be a positive multiple of 16 and in_features of 32")
    if x.dim() < 1 or x.shape[-1] != k or x.numel() == 0:
        raise ValueError(f"x must be [..., {k}] with at least one row, got {tuple(x.shape)}")
    if x.device != packed.device:
        raise ValueError("x and packed must be on the same device")
    if not 0 <= split_k <= 16:
        raise ValueError("split_k must be in 0..16")
    if row_tiles not in (0, 1, 2) or (row_tiles and n // 16 % row_tiles):
        raise ValueError("row_tiles must be 0, 1 or 2 and divide out_features / 16")
    _check_packed_layer(packed, src_bytes, chunk_bytes)
    _check_range(src_bytes, gate_offset, n * k)
    _check_range(src_bytes, up_offset, n * k)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, k)
    if not x.is_cuda:
        if out is not None:
            raise ValueError("out is for GPU tensors")
        wg = mxfp4_unpack_range(packed, src_bytes, chunk_bytes, gate_offset, n * k).view(n, k)
        wu = mxfp4_unpack_range(packed, src_bytes, chunk_bytes, up_offset, n * k).view(n, k)
        if act is not None:
            x2, wg, wu = _mxfp8_values(*mxfp8_quantize_rows(x2)), wg.float(), wu.float()
        elif out_dtype == torch.float32:
            x2, wg, wu = x2.float(), wg.float(), wu.float()
        y = torch.nn.functional.silu(torch.nn.functional.linear(x2, wg)) * torch.nn.functional.linear(x2, wu)
        return y.to(out_dtype).view(*lead, n)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if x2.data_ptr() % 16:
        x2 = x2.clone()
    m = x2.shape[0]
    if out is None:
        y = torch.empty(m, n, dtype=out_dtype, device=x.device)
    else:
        y = out
        if y.device != x.device or tuple(y.shape) != (m, n) or y.stride(1) != 1 or y.stride(0) < n:
            raise ValueError(f"out must be [{m}, {n}] on x's device with unit stride along rows")
    if act is not None:
        xq, xs = mxfp8_quantize_rows(x2)
        _core.mxfp4_swiglu_mx(packed.data_ptr(), src_bytes, chunk_bytes, gate_offset, up_offset, xq.data_ptr(),
                              xs.data_ptr(), m, n, k, y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, _stream())
        return y if out is not None else y.view(*lead, n)
    if tiled:
        _core.mxfp4_swiglu_tiled(packed.data_ptr(), src_bytes, chunk_bytes, gate_offset, up_offset, x2.data_ptr(), m, n,
                                 k, y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, _stream())
        return y if out is not None else y.view(*lead, n)
    _core.mxfp4_swiglu(packed.data_ptr(), src_bytes, chunk_bytes, gate_offset, up_offset, x2.data_ptr(), m, n, k,
                       y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, split_k, row_tiles, _stream())
    return y if out is not None else y.view(*lead, n)


def _packed_swiglu(fmt: str, x: torch.Tensor, packed: torch.Tensor, out_features: int, in_features: int,
                   src_bytes: int, chunk_bytes: int, block: int, gate_offset: int, up_offset: int,
                   out_dtype: torch.dtype, split_k: int, row_tiles: int, out: Optional[torch.Tensor],
                   tiled: bool = False) -> torch.Tensor:
    """`mxfp4_swiglu`'s checks and routes for the "mxfp6" and the "fp8" layer format."""
    _check_tiled(tiled, split_k, row_tiles)
    if out is not None:
        out_dtype = out.dtype
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"x must be {torch.bfloat16}, got {x.dtype}")
    n, k = int(out_features), int(in_features)
    if n <= 0 or n % 16 or k <= 0 or k % 32:
        raise ValueError("out_features must be a positive multiple of 16 and in_features of 32")
    if x.dim() < 1 or x.shape[-1] != k or x.numel() == 0:
        raise ValueError(f"x must be [..., {k}] with at least one row, got {tuple(x.shape)}")
    if x.device != packed.device:
        raise ValueError("x and packed must be on the same device")
    if not 0 <= split_k <= 16:
        raise ValueError("split_k must be in 0..16")
    if row_tiles not in (0, 1, 2) or (row_tiles and n // 16 % row_tiles):
        raise ValueError("row_tiles must be 0, 1 or 2 and divide out_features / 16")
    if fmt == "fp8":
        _check_fp8_layer(packed, src_bytes, chunk_bytes, block)
    else:
        _check_mxfp6_layer(packed, src_bytes, chunk_bytes)
    _check_range(src_bytes, gate_offset, n * k)
    _check_range(src_bytes, up_offset, n * k)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, k)
    if not x.is_cuda:
        if out is not None:
            raise ValueError("out is for GPU tensors")
        if fmt == "fp8":
            wg = fp8_unpack_range(packed, src_bytes, chunk_bytes, gate_offset, n * k, block).view(n, k)
            wu = fp8_unpack_range(packed, src_bytes, chunk_bytes, up_offset, n * k, block).view(n, k)
        else:
            wg = mxfp6_unpack_range(packed, src_bytes, chunk_bytes, gate_offset, n * k).view(n, k)
            wu = mxfp6_unpack_range(packed, src_bytes, chunk_bytes, up_offset, n * k).view(n, k)
        if out_dtype == torch.float32:
            x2, wg, wu = x2.float(), wg.float(), wu.float()
        y = torch.nn.functional.silu(torch.nn.functional.linear(x2, wg)) * torch.nn.functional.linear(x2, wu)
        return y.view(*lead, n)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if x2.data_ptr() % 16:
        x2 = x2.clone()
    m = x2.shape[0]
    if out is None:
        y = torch.empty(m, n, dtype=out_dtype, device=x.device)
    else:
        y = out
        if y.device != x.device or tuple(y.shape) != (m, n) or y.stride(1) != 1 or y.stride(0) < n:
            raise ValueError(f"out must be [{m}, {n}] on x's device with unit stride along rows")
    if tiled and fmt == "fp8":
        _core.fp8_swiglu_tiled(packed.data_ptr(), src_bytes, chunk_bytes, block, gate_offset, up_offset, x2.data_ptr(),
                               m, n, k, y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, _stream())
    elif tiled:
        _core.mxfp6_swiglu_tiled(packed.data_ptr(), src_bytes, chunk_bytes, gate_offset, up_offset, x2.data_ptr(), m, n,
                                 k, y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, _stream())
    elif fmt == "fp8":
        _core.fp8_swiglu(packed.data_ptr(), src_bytes, chunk_bytes, block, gate_offset, up_offset, x2.data_ptr(), m, n,
                         k, y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, split_k, row_tiles, _stream())
    else:
        _core.mxfp6_swiglu(packed.data_ptr(), src_bytes, chunk_bytes, gate_offset, up_offset, x2.data_ptr(), m, n, k,
                           y.data_ptr(), y.stride(0), out_dtype == torch.bfloat16, split_k, row_tiles, _stream())
    return y if out is not None else y.view(*lead, n)


def mxfp6_swiglu(x: torch.Tensor, packed: torch.Tensor, out_features: int, in_features: int, *, src_bytes: int,
                 chunk_bytes: int, gate_offset: int, up_offset: int, out_dtype: torch.dtype = torch.bfloat16,
                 split_k: int = 0, row_tiles: int = 0, out: Optional[torch.Tensor] = None,
                 tiled: bool = False) -> torch.Tensor:
    """``silu(x @ Wg.T) * (x @ Wu.T)``, the front half of a gated MLP, for a bf16 `x`
    [..., in_features] and two [out_features, in_features] weights stored as elements
    [gate_offset, ...) and [up_offset, ...) of the MXFP6-packed layer `packed` (as in
    `mxfp6_linear`; the offsets are independent multiples of 32, in any order).

    GPU: one kernel on the current stream reads x once and both weights where they
    lie; the two products are `mxfp6_linear`'s sums (with equal `split_k` bit for
    bit its f32 results) and stay in the MFMA accumulators, ``(g / (1 + expf(-g))) * u``
    is evaluated in f32 and only the result is written, rounded once. `split_k`,
    `row_tiles` (pairs of a gate and an up tile per wave: 0, 1 or 2) and `out` as in
    `mxfp4_swiglu`.
    CPU: the host reference dequantizes both ranges, then
    ``F.silu(F.linear(x, wg)) * F.linear(x, wu)`` - in f32 for an f32 result, in bf16
    (op for op what two `mxfp6_linear` calls and the torch epilogue do) for a bf16 one.
    `tiled` as in `mxfp6_linear`: the gated kernel for many rows, whose g and u are bit
    for bit the tiled linear's f32 results."""
    return _packed_swiglu("mxfp6", x, packed, out_features, in_features, src_bytes, chunk_bytes, 32, gate_offset,
                          up_offset, out_dtype, split_k, row_tiles, out, tiled)


def fp8_swiglu(x: torch.Tensor, packed: torch.Tensor, out_features: int, in_features: int, *, src_bytes: int,
               chunk_bytes: int, gate_offset: int, up_offset: int, block: int = 128,
               out_dtype: torch.dtype = torch.bfloat16, split_k: int = 0, row_tiles: int = 0,
               out: Optional[torch.Tensor] = None, tiled: bool = False) -> torch.Tensor:
    """`mxfp6_swiglu` for the fp8-packed layer `packed` with one scale per `block` elements
    (as in `fp8_linear`): the products are `fp8_linear`'s sums, bit for bit with equal
    `split_k`. The offsets are multiples of 32, not of `block`. `tiled`: fp8_tiled.hip's
    gated kernel."""
    return _packed_swiglu("fp8", x, packed, out_features, in_features, src_bytes, chunk_bytes, block, gate_offset,
                          up_offset, out_dtype, split_k, row_tiles, out, tiled)


_ATTN_D = (32, 64, 128)
_ATTN_MAX_CAPACITY = 1 << 20


def _check_caches(k_cache: torch.Tensor, v_cache: torch.Tensor) -> Tuple[int, int, int, int]:
    """(B, kv_heads, capacity, d) of a pair of KV caches, checked."""
    for name, c in (("k_cache", k_cache), ("v_cache", v_cache)):
        if c.dtype != torch.bfloat16:
            raise ValueError(f"{name} must be {torch.bfloat16}, got {c.dtype}")
        if c.dim() != 4 or c.numel() == 0:
            raise ValueError(f"{name} must be [B, kv_heads, capacity, d], got {tuple(c.shape)}")
        if not c.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if c.is_cuda and c.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")
    if k_cache.shape != v_cache.shape or k_cache.device != v_cache.device:
        raise ValueError("k_cache and v_cache must have one shape and one device")
    b, kvh, cap, d = k_cache.shape
    if d not in _ATTN_D:
        raise ValueError(f"head_dim must be one of {_ATTN_D}, got {d}")
    if cap > _ATTN_MAX_CAPACITY:
        raise ValueError(f"capacity must be at most {_ATTN_MAX_CAPACITY} positions, got {cap}")
    return b, kvh, cap, d


def _check_index(t: torch.Tensor, name: str, b: int, device: torch.device) -> None:
    if t.dtype != torch.int32:
        raise ValueError(f"{name} must be {torch.int32}, got {t.dtype}")
    if tuple(t.shape) != (b,) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [{b}] tensor, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name} must be on the caches' device")


def _rows(t: torch.Tensor, name: str, b: int, n: int, device: torch.device) -> torch.Tensor:
    """`t` as bf16 rows [b, n] with unit stride along the row and any row stride: the view
    itself where it allows that (a last-dimension slice of a merged projection), else a copy."""
    if t.dtype != torch.bfloat16:
        raise ValueError(f"{name} must be {torch.bfloat16}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name} must be on the caches' device")
    if t.numel() != b * n or t.dim() < 1 or t.shape[-1] != n:
        raise ValueError(f"{name} must be [{b}, ..., {n}] with {b} rows, got {tuple(t.shape)}")
    lead = [i for i in range(t.dim() - 1) if t.shape[i] != 1]
    if t.stride(-1) == 1 and len(lead) <= 1:
        ld = t.stride(lead[0]) if lead else n
        if ld >= n:
            return t.as_strided((b, n), (ld, 1))
    return t.reshape(b, n).contiguous()


def rope_append(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
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
    host). CPU: plain torch."""
    b, kvh, cap, d = _check_caches(k_cache, v_cache)
    dev = k_cache.device
    _check_index(pos, "pos", b, dev)
    for name, t in (("cos", cos), ("sin", sin)):
        if t.dtype != torch.float32 or tuple(t.shape) != (cap, d) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous f32 [{cap}, {d}] tensor on the caches' device")
    if q.dim() < 1 or q.shape[-1] <= 0 or q.shape[-1] % d:
        raise ValueError(f"q must be [B, ..., heads * {d}], got {tuple(q.shape)}")
    heads = q.shape[-1] // d
    if heads % kvh:
        raise ValueError(f"heads ({heads}) must be a multiple of kv_heads ({kvh})")
    if heads + 2 * kvh > 65535:
        raise ValueError("heads + 2 * kv_heads must fit a grid dimension (65535)")
    q2, k2, v2 = _rows(q, "q", b, heads * d, dev), _rows(k, "k", b, kvh * d, dev), _rows(v, "v", b, kvh * d, dev)
    if not dev.type == "cuda":
        ok = (pos >= 0) & (pos < cap)
        p = pos.clamp(0, cap - 1).long()
        c, s = cos[p][:, None, :], sin[p][:, None, :]  # [B, 1, d]

        def rot(x, nh):
            x = x.reshape(b, nh, d).float()
            return (x * c + torch.cat([-x[..., d // 2:], x[..., : d // 2]], -1) * s).to(torch.bfloat16)

        q_out = torch.where(ok[:, None, None], rot(q2, heads), torch.zeros((), dtype=torch.bfloat16))
        rows = ok.nonzero().flatten()
        k_cache[rows, :, p[rows]] = rot(k2, kvh)[rows]
        v_cache[rows, :, p[rows]] = v2.reshape(b, kvh, d)[rows]
        return q_out
    q_out = torch.empty(b, heads, d, dtype=torch.bfloat16, device=dev)
    _core.attn_rope_append(q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0), v2.data_ptr(), v2.stride(0),
                           pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), b, heads, kvh, d, cap, q_out.data_ptr(),
                           k_cache.data_ptr(), v_cache.data_ptr(), _stream())
    return q_out


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor, *,
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
    although the quotient would be finite."""
    b, kvh, cap, d = _check_caches(k_cache, v_cache)
    dev = k_cache.device
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if q.dtype != torch.bfloat16:
        raise ValueError(f"q must be {torch.bfloat16}, got {q.dtype}")
    if q.device != dev:
        raise ValueError("q must be on the caches' device")
    if q.dim() != 3 or q.shape[0] != b or q.shape[2] != d or q.shape[1] < 1:
        raise ValueError(f"q must be [{b}, heads, {d}], got {tuple(q.shape)}")
    heads = q.shape[1]
    if heads % kvh:
        raise ValueError(f"heads ({heads}) must be a multiple of kv_heads ({kvh})")
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
            kk = k_cache[i, :, :n].float().repeat_interleave(g, dim=0)  # [heads, n, d]
            vv = v_cache[i, :, :n].float().repeat_interleave(g, dim=0)
            s = torch.einsum("hd,hnd->hn", q[i].float(), kk) / d ** 0.5
            y[i] = torch.einsum("hn,hnd->hd", torch.softmax(s, -1), vv)
        return y.view(b, heads * d).to(out_dtype)
    if not q.is_contiguous():
        q = q.contiguous()
    if q.data_ptr() % 16:
        q = q.clone()
    nbytes = _core.attn_decode_workspace_bytes(b, heads, kvh, d, cap, max_len)
    if nbytes < 0 or b * heads > 0x7FFFFFFF:
        raise ValueError("the batch is too large for one launch")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    y = torch.empty(b, heads * d, dtype=out_dtype, device=dev)
    _core.attn_decode(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), lens.data_ptr(), b, heads, kvh, d, cap,
                      max_len, ws.data_ptr(), nbytes, y.data_ptr(), out_dtype == torch.bfloat16, _stream())
    return y
