"""Host reference of the MXFP6 wire format (csrc/core/mxfp6.cc) against an independent numpy
reference of the rules in core/mxfp6.h, in integers and float64 only: the e2m3 value table, the
scale formula on the f32 bits of the block's finite amax, a nearest-value search with ties to
the even code, and the 6-bit little-endian packing. Every comparison is exact equality. The
gfx950 kernels are checked against the host codec (and, on the exhaustive inputs, against this
reference) in test_gpu_mxfp6.py."""
import numpy as np
import pytest

from distributed_llm_dissemination_amd import _core

MiB = 1 << 20
KiB = 1 << 10
# magnitude of m = 0..31: (m & 7) / 8 below 8, else (1 + (m & 7) / 8) * 2^((m >> 3) - 1)
MAG = np.array([(m & 7) / 8 if m < 8 else (1 + (m & 7) / 8) * 2.0 ** ((m >> 3) - 1) for m in range(32)])
TIES = tuple(((MAG[:-1] + MAG[1:]) / 2).tolist())  # the 31 midpoints of neighbouring magnitudes


# ---------------------------------------------------------------- the reference

def ref_scale_exp(amax_bf16):
    """E from the bf16 bits of a block's finite amax (the rule is stated on its f32 bits)."""
    ab = amax_bf16.astype(np.int64) << 16
    ef, mant = ab >> 23, ab & 0x7FFFFF
    e = ef - 127 - 2 + (mant > 0x700000)
    e = np.where(ef == 0, -126, e)
    e = np.where(ab == 0, 0, e)
    return np.clip(e, -126, 125)


def codes_to_bytes(code):
    """[blocks, 32] codes -> [blocks, 24] bytes: element i at bits [6i, 6i + 6) of the block read
    as one little-endian integer (four codes fill 24 bits = three bytes)."""
    c = np.asarray(code, dtype=np.uint32).reshape(-1, 8, 4)
    v = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(-1, 24)


def bytes_to_codes(q):
    b = np.asarray(q, dtype=np.uint8).reshape(-1, 8, 3).astype(np.uint32)
    v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return np.stack([(v >> (6 * k)) & 63 for k in range(4)], -1).reshape(-1, 32)


def ref_pack(bits):
    """bf16 bit patterns (uint16, a multiple of 32) -> (q uint8 [3n/4], scales uint8 [n/32])."""
    b = np.asarray(bits, dtype=np.uint16).reshape(-1, 32).astype(np.uint32)
    a = b & 0x7FFF
    nan = (a > 0x7F80).any(1)
    e = ref_scale_exp(np.where(a < 0x7F80, a, 0).max(1))
    # |x| * 2^-E in float64: exact (an 8-bit significand and an exponent within +-260)
    x = (np.where(a < 0x7F80, a, 0) << 16).astype(np.uint32).view(np.float32).astype(np.float64)
    x[a >= 0x7F80] = np.inf
    y = np.minimum(np.ldexp(x, -e[:, None]), 7.5)
    d = np.abs(y[..., None] - MAG)
    cand = d == d.min(-1, keepdims=True)
    even = cand & (np.arange(32) % 2 == 0)
    code = np.where(even.any(-1), even.argmax(-1), cand.argmax(-1)).astype(np.uint32) | ((b >> 15) << 5)
    q = codes_to_bytes(code)
    q[nan] = 0
    scales = np.where(nan, 0xFF, e + 127).astype(np.uint8)
    return q.reshape(-1), scales


def ref_unpack(q, scales):
    """(q uint8 [3n/4], scales uint8 [n/32]) -> bf16 bit patterns uint16 [n]."""
    code = bytes_to_codes(q)
    s = np.asarray(scales, dtype=np.uint8).astype(np.int64)
    v = np.where(code & 32, -1.0, 1.0) * MAG[code & 31] * np.ldexp(1.0, s - 127)[:, None]
    with np.errstate(over="ignore"):
        out = (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)  # exact; beyond bf16's range: inf
    fin = (out & 0x7FFF) < 0x7F80
    assert np.array_equal(out_f64(out)[fin], v[fin])  # no bit was dropped
    out[s == 0xFF] = 0x7FC0
    return out.reshape(-1)


def out_f64(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ---------------------------------------------------------------- inputs

def bf16_bits(values):
    """bf16 bit patterns of values that are exactly representable in bf16."""
    f = np.asarray(values, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32)
    assert not (u & 0xFFFF).any()
    assert np.array_equal(f.astype(np.float64), np.asarray(values, dtype=np.float64))
    return (u >> 16).astype(np.uint16)


def all_patterns():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def permuted_patterns():
    return all_patterns()[np.random.default_rng(20240607).permutation(65536)]


def handmade_blocks():
    blocks = []

    def block(head, fill=0):
        v = np.full(32, fill, dtype=np.uint16)
        v[: len(head)] = head
        blocks.append(v)

    block([], 0x0000)                                   # all zero
    block([], 0x8000)                                   # all -0
    block([], 0x7FC0)                                   # all NaN
    block([0xFFFF, 0x7F81], 0x7FC0)                     # other NaN patterns
    block(np.r_[bf16_bits([1, -2, 3.5, 0.1015625]), [0x7FC1]], 0x3F80)  # one NaN among finite values
    block([0x7F80, 0xFF80] * 16)                        # all +-inf
    block([0x7F80])                                     # +inf alone
    block(np.r_[[0x7F80, 0xFF80], bf16_bits([1, -3, 0.25, 100])])  # inf beside finite values
    block(np.arange(1, 33))                             # only subnormals (E = -126)
    block(np.r_[np.arange(0x60, 0x80), ] | 0x8000)      # negative subnormals, the largest ones
    for k in (-126, -125, -10, 0, 7, 124, 125):
        top = bf16_bits([7.5 * 2.0**k])[0]
        rest = bf16_bits([v * 2.0**k for v in (-5.5, 3.25, 0.125, -0.375, 1, 2.75, 4.5, -7, 0.0625, 6.75, -1.9375)])
        block(np.r_[[top], rest])                       # amax exactly 7.5 * 2^k
        block(np.r_[[top + 1], rest])                   # one ulp above (E = k + 1; capped at 125)
        block(np.r_[[top | 0x8000], rest])
    block(np.r_[[0x7F7F, 0xFF7F, 0x7F70, 0x7F6F, 0x7F00, 0x7E80], bf16_bits([1, -1])])  # bf16 max: E capped
    for e in (-126, -125, -124, -3, 0, 5, 125):
        for s in (1, -1):                               # all 31 tie points of one sign at scale E
            block(np.r_[bf16_bits([7.5 * 2.0**e]), bf16_bits([s * t * 2.0**e for t in TIES])])
    block(bf16_bits([-0.1015625, 0.1015625, 1]))        # -0.1 keeps its sign
    return np.concatenate(blocks)


CASES = {"natural": all_patterns, "permuted": permuted_patterns, "handmade": handmade_blocks}


def host_pack(bits):
    """The host codec on one chunk: (q, scales)."""
    n = len(bits)
    chunk = -(-2 * n // 4096) * 4096
    packed = np.frombuffer(_core.mxfp6_pack_layer_host(bits.tobytes(), chunk), dtype=np.uint8)
    assert len(packed) == n // 32 * 25
    return packed[: n // 32 * 24], packed[n // 32 * 24:]


def host_unpack(q, scales):
    n = len(scales) * 32
    chunk = -(-2 * n // 4096) * 4096
    out = _core.mxfp6_unpack_layer_host(np.concatenate([q, scales]).tobytes(), 2 * n, chunk)
    return np.frombuffer(out, dtype=np.uint16)


# ---------------------------------------------------------------- tests

def test_reference_rules():
    """The reference itself on the values the format's description names."""
    assert MAG.tolist() == [0, .125, .25, .375, .5, .625, .75, .875, 1, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
                            2, 2.25, 2.5, 2.75, 3, 3.25, 3.5, 3.75, 4, 4.5, 5, 5.5, 6, 6.5, 7, 7.5]
    assert len(TIES) == 31
    assert ref_scale_exp(bf16_bits([0, 7.5, 7.53125, 3.75, 1, 2.0**-130, (2 - 2.0**-7) * 2.0**127,
                                    1.875 * 2.0**127])).tolist() == [0, 0, 1, -1, -2, -126, 125, 125]
    assert [_core.mxfp6_scale_exp(int(b) << 16) for b in bf16_bits([0, 7.5, 7.53125, 3.75, 1, 2.0**-130,
                                                                    (2 - 2.0**-7) * 2.0**127, 1.875 * 2.0**127])] == \
        [0, 0, 1, -1, -2, -126, 125, 125]
    # element 0 is the low 6 bits of byte 0; a code may straddle two bytes
    assert codes_to_bytes(np.r_[[63], np.zeros(31, int)])[0, :2].tolist() == [63, 0]
    assert codes_to_bytes(np.r_[[0, 63], np.zeros(30, int)])[0, :3].tolist() == [0xC0, 0x0F, 0]
    assert codes_to_bytes(np.r_[np.zeros(31, int), [63]])[0, 21:].tolist() == [0, 0, 0xFC]
    x = bf16_bits([7.5] + [s * t for t in TIES[:7] for s in (1, -1)] + [-0.1015625] + [0] * 16)
    q, s = ref_pack(x)
    codes = bytes_to_codes(q).reshape(-1)
    assert s.tolist() == [127]
    # 0.0625 -> 0, 0.1875 -> 2 (0.25), 0.3125 -> 2, 0.4375 -> 4, ...: ties to the even code; -0.1 -> -0.125
    assert codes[:16].tolist() == [31, 0, 32, 2, 34, 2, 34, 4, 36, 4, 36, 6, 38, 6, 38, 33]


@pytest.mark.parametrize("case", list(CASES))
def test_host_pack_matches_reference(case):
    bits = CASES[case]()
    q, s = host_pack(bits)
    qr, sr = ref_pack(bits)
    assert np.array_equal(s, sr)
    assert np.array_equal(q, qr)
    assert s[s != 0xFF].min() >= 1 and s[s != 0xFF].max() <= 252
    assert not q.reshape(-1, 24)[s == 0xFF].any()


@pytest.mark.parametrize("case", list(CASES))
def test_host_unpack_matches_reference(case):
    q, s = ref_pack(CASES[case]())
    out = host_unpack(q, s)
    assert np.array_equal(out, ref_unpack(q, s))
    assert not (((out & 0x7FFF) == 0x7F80).any())  # nothing packed unpacks to inf
    assert np.array_equal((out & 0x7FFF) > 0x7F80, np.repeat(s == 0xFF, 32))


def test_handmade_blocks_pack_as_described():
    bits = handmade_blocks()
    q, s = host_pack(bits)
    codes = bytes_to_codes(q)
    assert s[0] == 127 and not codes[0].any()                  # zeros: E = 0
    assert s[1] == 127 and (codes[1] == 32).all()              # -0 keeps its sign
    assert s[2] == s[3] == s[4] == 0xFF                        # a NaN anywhere marks the block
    assert s[5] == 127 and codes[5].tolist() == [31, 63] * 16  # no finite value: E = 0, inf saturates
    assert s[6] == 127 and codes[6, 0] == 31
    assert s[7] == 127 + 4 and codes[7, :2].tolist() == [31, 63]  # amax 100 <= 7.5 * 2^4
    assert s[8] == s[9] == 1                                   # subnormal amax: E = -126
    last = codes[-1]
    # amax 1: E = -2, so -0.1 * 4 = -0.40625 -> -0.375 (code 3 with the sign kept), 1 * 4 -> code 24
    assert s[-1] == 125 and last[:3].tolist() == [35, 3, 24]


def every_code_position_and_scale():
    """256 * 64 blocks: block (s, r) has scale byte s and code (r + j) % 64 at position j, so every
    code occurs in every position under every scale byte: 64 x 32 x 256 elements."""
    r = np.arange(64)[:, None]
    code = (r + np.arange(32)) % 64
    q = np.tile(codes_to_bytes(code), (256, 1))
    s = np.repeat(np.arange(256), 64).astype(np.uint8)
    return q.reshape(-1), s


def test_host_unpack_every_code_position_and_scale_byte():
    q, s = every_code_position_and_scale()
    codes = bytes_to_codes(q)
    assert len(s) * 32 == 64 * 32 * 256
    seen = np.unique((s.astype(np.int64)[:, None] * 32 + np.arange(32)) * 64 + codes)
    assert len(seen) == 64 * 32 * 256
    out = host_unpack(q, s)
    assert np.array_equal(out, ref_unpack(q, s))
    o = out.reshape(256, 64, 32)
    assert not ((o[:253] & 0x7FFF) >= 0x7F80).any()            # bytes 0..252: always finite
    assert ((o[253:255] & 0x7FFF) == 0x7F80).any()             # 253, 254: inf beyond bf16's range
    assert (o[255] == 0x7FC0).all()                            # 0xFF: NaN whatever q holds


def test_sizes():
    ps, ss = _core.mxfp6_packed_size, _core.mxfp6_source_size
    # 24 + 1 bytes per 32 elements: 25/64 of the source bytes
    assert ps(2 * MiB + 64, MiB) == 2 * (384 * KiB + 16 * KiB) + 25
    assert ps(64 * MiB, 64 * MiB) == 25 * MiB
    for src, chunk in [(3 * MiB, MiB), (3 * MiB + 4096, MiB), (64, MiB), (64 * 1031, 4096), (MiB + 64, 4096)]:
        assert ps(src, chunk) == sum(min(chunk, src - o) * 25 // 64 for o in range(0, src, chunk))
        assert ss(ps(src, chunk), chunk) == src
    for bad in (24, 26, 25 * 64 + 1, ps(MiB, MiB) + 5):
        with pytest.raises(RuntimeError, match="packed mxfp6"):
            ss(bad, MiB)
    with pytest.raises(RuntimeError, match="64 B"):
        _core.mxfp6_pack_layer_host(bytes(96), 4096)
    with pytest.raises(RuntimeError, match="1024"):
        _core.mxfp6_pack_layer_host(bytes(128), 1000)


SRC, CHUNK = 64 * 1031, 4096  # 16 full chunks of 64 blocks and a tail of 7: an odd block count


@pytest.fixture(scope="module")
def layer():
    bits = np.frombuffer(_core.fill_random_host(SRC, 11), dtype=np.uint16).copy()
    bits[(bits & 0x7FFF) > 0x7F80] &= 0xBFFF  # random bits hold NaNs in one block of eight: keep a few only
    bits[40] = 0x7FC0                          # one NaN block in chunk 0
    bits[SRC // 2 - 3] = 0xFFC1                # and the last block of the tail
    packed = np.frombuffer(_core.mxfp6_pack_layer_host(bits.tobytes(), CHUNK), dtype=np.uint8)
    whole = np.concatenate([ref_unpack(*ref_pack(bits[o // 2: (o + min(CHUNK, SRC - o)) // 2]))
                            for o in range(0, SRC, CHUNK)])
    return bits, packed, whole


def test_layer_layout_is_per_chunk(layer):
    """A layer with a tail chunk: every packed chunk is [q][scales] of its own source chunk."""
    bits, packed, whole = layer
    pc = CHUNK * 25 // 64
    assert len(packed) == 16 * pc + 7 * 25
    for c, off in enumerate(range(0, SRC, CHUNK)):
        part = bits[off // 2: (off + min(CHUNK, SRC - off)) // 2]
        q, s = ref_pack(part)
        got = packed[c * pc: c * pc + len(q) + len(s)]
        assert np.array_equal(got, np.concatenate([q, s])), c
    out = np.frombuffer(_core.mxfp6_unpack_layer_host(packed.tobytes(), SRC, CHUNK), dtype=np.uint16)
    assert np.array_equal(out, whole)
    assert (whole[32:64] == 0x7FC0).all() and (whole[-32:] == 0x7FC0).all()


# (offset, count): inside a block; starting and ending inside a code that straddles two bytes
# (elements 1, 2 and 5 of a block); a whole block; across a chunk edge (2048 elements per chunk);
# the tail chunk (starts at element 32768, 224 elements); its last, odd block; everything; nothing
RANGES = [(7, 1), (1, 1), (33, 2), (2, 4), (5, 30), (32, 32), (2040, 20), (2047, 2), (2048 * 3 - 1, 2048 + 2),
          (32768 + 5, 200), (32768 + 192 + 1, 31), (32768 + 223, 1), (0, SRC // 2), (SRC // 2, 0), (500, 100)]


def test_unpack_range_matches_reference_slice(layer):
    _, packed, whole = layer
    total = SRC // 2
    for off, n in RANGES:
        out = np.full(n + 1, 0xA5A5, dtype=np.uint16)
        _core.mxfp6_unpack_range_host(packed.ctypes.data, packed.size, SRC, CHUNK, off, n, out.ctypes.data)
        assert np.array_equal(out[:n], whole[off: off + n]) and out[n] == 0xA5A5, (off, n)
    with pytest.raises(RuntimeError, match="outside the layer"):
        _core.mxfp6_unpack_range_host(packed.ctypes.data, packed.size, SRC, CHUNK, total - 31, 32, 0)
    with pytest.raises(RuntimeError, match="smaller"):
        _core.mxfp6_unpack_range_host(packed.ctypes.data, packed.size - 1, SRC, CHUNK, 0, 32, 0)


def test_ops_cpu_route_is_the_host_codec(layer):
    import torch

    from distributed_llm_dissemination_amd import ops

    bits, packed, whole = layer
    x = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    assert ops.mxfp6_packed_size(SRC, CHUNK) == len(packed)
    assert np.array_equal(ops.mxfp6_pack_layer(x, CHUNK).numpy(), packed)
    q, s = ops.mxfp6_pack(x[:2048])
    assert np.array_equal(np.concatenate([q.numpy(), s.numpy()]), packed[: 2048 // 32 * 25])
    y = ops.mxfp6_unpack(q, s)
    assert np.array_equal(y.view(torch.int16).numpy().view(np.uint16), whole[:2048])
    p = torch.from_numpy(packed.copy())
    for off, n in [(0, SRC // 2), (2048 - 32, 96), (32768 + 192, 32), (64, 0)]:
        got = ops.mxfp6_unpack_range(p, SRC, CHUNK, off, n)
        assert got.dtype == torch.bfloat16 and got.shape == (n,)
        assert np.array_equal(got.view(torch.int16).numpy().view(np.uint16), whole[off: off + n]), (off, n)
    for kw in [dict(elem_offset=16, n=32), dict(elem_offset=0, n=48), dict(elem_offset=SRC // 2 - 32, n=64),
               dict(elem_offset=-32, n=32), dict(elem_offset=0, n=32, chunk_bytes=1000),
               dict(elem_offset=0, n=32, src_bytes=SRC + 64), dict(elem_offset=0, n=32, src_bytes=SRC + 2)]:
        a = dict(src_bytes=SRC, chunk_bytes=CHUNK)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.mxfp6_unpack_range(p, a["src_bytes"], a["chunk_bytes"], a["elem_offset"], a["n"])
    with pytest.raises(ValueError, match="bfloat16"):
        ops.mxfp6_pack(x.float())
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.mxfp6_pack(x[:48])
    with pytest.raises(ValueError, match="one byte per 24"):
        ops.mxfp6_unpack(q, s[:-1])
    with pytest.raises(ValueError, match="uint8"):
        ops.mxfp6_unpack(q.to(torch.int32), s)


# ---------------------------------------------------------------- accuracy of the three formats

def _to_bf16_bits(x64):
    """float64 -> nearest bf16 (ties to even), as bit patterns."""
    u = x64.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def test_quantization_error_is_in_fp8s_class(capsys):
    """2^20 bf16 values from N(0, 0.02^2), seed 0, through the host codecs of the three formats:
    relative RMS error of the dequantized values. A float64 model of the formats gave 1.18e-1
    for MXFP4, 2.66e-2 for fp8 and 2.82e-2 for MXFP6 (ratios 0.24 and 1.06); the bounds say
    'MXFP6 is in fp8's class and far from MXFP4's', not a rate."""
    n = 1 << 20
    bits = _to_bf16_bits(np.random.default_rng(0).normal(0.0, 0.02, n))
    x = out_f64(bits)
    src = bits.tobytes()

    def rel_rms(deq_bytes):
        y = out_f64(np.frombuffer(deq_bytes, dtype=np.uint16))
        return float(np.sqrt(((y - x) ** 2).sum() / (x ** 2).sum()))

    err = {
        "mxfp4": rel_rms(_core.mxfp4_unpack_layer_host(_core.mxfp4_pack_layer_host(src, 2 * n), 2 * n, 2 * n)),
        "fp8_block128": rel_rms(_core.fp8_unpack_layer_host(_core.fp8_pack_layer_host(src, 2 * n, 128), 2 * n, 2 * n, 128)),
        "mxfp6": rel_rms(_core.mxfp6_unpack_layer_host(_core.mxfp6_pack_layer_host(src, 2 * n), 2 * n, 2 * n)),
    }
    with capsys.disabled():
        print("\nrelative RMS quantization error, 2^20 values of N(0, 0.02^2):",
              ", ".join(f"{k} {v:.4e}" for k, v in err.items()),
              f"; mxfp6/mxfp4 {err['mxfp6'] / err['mxfp4']:.3f}, mxfp6/fp8 {err['mxfp6'] / err['fp8_block128']:.3f}")
    assert err["mxfp6"] < 0.5 * err["mxfp4"]
    assert err["mxfp6"] < 1.25 * err["fp8_block128"]
