"""Host reference of the MXFP4 wire format (csrc/core/mxfp4.cc) against an independent numpy
reference of the rules in core/mxfp4.h: the e2m1 value table, the scale formula on the f32 bits
of the block's finite amax, and a nearest-value search with ties to the even code. Every
comparison is exact equality. The gfx950 kernels are checked against the host codec (and, on
the exhaustive inputs, against this reference) in test_gpu_mxfp4.py."""
import numpy as np
import pytest

from distributed_llm_dissemination_amd import _core

MiB = 1 << 20
KiB = 1 << 10
MAG = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


# ---------------------------------------------------------------- the reference

def ref_scale_exp(amax_bf16):
    """E from the bf16 bits of a block's finite amax (the rule is stated on its f32 bits)."""
    ab = amax_bf16.astype(np.int64) << 16
    ef, mant = ab >> 23, ab & 0x7FFFFF
    e = ef - 127 - 2 + (mant > 0x400000)
    e = np.where(ef == 0, -126, e)
    e = np.where(ab == 0, 0, e)
    return np.clip(e, -126, 125)


def ref_pack(bits):
    """bf16 bit patterns (uint16, a multiple of 32) -> (q uint8 [n/2], scales uint8 [n/32])."""
    b = np.asarray(bits, dtype=np.uint16).reshape(-1, 32).astype(np.uint32)
    a = b & 0x7FFF
    nan = (a > 0x7F80).any(1)
    e = ref_scale_exp(np.where(a < 0x7F80, a, 0).max(1))
    with np.errstate(all="ignore"):
        x = (a << 16).astype(np.uint32).view(np.float32)  # |x|
        y = np.minimum(x * np.ldexp(np.float32(1), -e).astype(np.float32)[:, None], np.float32(6))
        d = np.abs(y.astype(np.float64)[..., None] - MAG)  # exact in f64
    cand = d == d.min(-1, keepdims=True)
    even = cand & (np.arange(8) % 2 == 0)
    code = np.where(even.any(-1), even.argmax(-1), cand.argmax(-1)).astype(np.uint32) | ((b >> 15) << 3)
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    q[nan] = 0
    scales = np.where(nan, 0xFF, e + 127).astype(np.uint8)
    return q.reshape(-1), scales


def ref_unpack(q, scales):
    """(q uint8 [n/2], scales uint8 [n/32]) -> bf16 bit patterns uint16 [n]."""
    q = np.asarray(q, dtype=np.uint8)
    code = np.stack([q & 15, q >> 4], -1).reshape(-1, 32)
    s = np.asarray(scales, dtype=np.uint8).astype(np.int64)
    v = np.where(code & 8, -1.0, 1.0) * MAG[code & 7] * np.ldexp(1.0, s - 127)[:, None]
    with np.errstate(over="ignore"):
        out = (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)  # exact; beyond bf16's range: inf
    out[s == 0xFF] = 0x7FC0
    return out.reshape(-1)


# ---------------------------------------------------------------- inputs

def bf16_bits(values):
    """bf16 bit patterns of values that are exactly representable in bf16."""
    f = np.asarray(values, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32)
    assert not (u & 0xFFFF).any()
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
    block(np.r_[[0x7F80, 0xFF80], bf16_bits([1, -3, 0.25, 100])])  # inf beside finite values
    block(np.arange(1, 33))                             # only subnormals (E = -126)
    block(np.r_[np.arange(0x60, 0x80), ] | 0x8000)      # negative subnormals, the largest ones
    for k in (-126, -125, -10, 0, 7, 124, 125):
        top = bf16_bits([6.0 * 2.0**k])[0]
        rest = bf16_bits([v * 2.0**k for v in (-5.5, 3.25, 0.125, -0.375, 1, 2.75, 4.5, -6)])
        block(np.r_[[top], rest])                       # amax exactly 6 * 2^k
        block(np.r_[[top + 1], rest])                   # one ulp above (E = k + 1; capped at 125)
        block(np.r_[[top | 0x8000], rest])
    block(np.r_[[0x7F7F, 0xFF7F, 0x7F40, 0x7F3F, 0x7F00, 0x7E80], bf16_bits([1, -1])])  # bf16 max: E capped
    for e in (-126, -125, -124, -3, 0, 5, 125):
        pts = [s * t * 2.0**e for t in TIES for s in (1, -1)]
        near = [s * t * 2.0**e for t in (1.0, 3.0) for s in (1, -1)]
        block(np.r_[bf16_bits([6.0 * 2.0**e]), bf16_bits(pts), bf16_bits(near)])  # every tie point at scale E
    block(bf16_bits([-0.1015625, 0.1015625, 1]))         # -0.1 keeps its sign: code 8
    return np.concatenate(blocks)


CASES = {"natural": all_patterns, "permuted": permuted_patterns, "handmade": handmade_blocks}


def host_pack(bits):
    """The host codec on one chunk: (q, scales)."""
    n = len(bits)
    src = 2 * n
    chunk = -(-src // 4096) * 4096
    packed = np.frombuffer(_core.mxfp4_pack_layer_host(bits.tobytes(), chunk), dtype=np.uint8)
    assert len(packed) == n // 2 + n // 32
    return packed[: n // 2], packed[n // 2:]


def host_unpack(q, scales):
    n = 2 * len(q)
    chunk = -(-2 * n // 4096) * 4096
    out = _core.mxfp4_unpack_layer_host(np.concatenate([q, scales]).tobytes(), 2 * n, chunk)
    return np.frombuffer(out, dtype=np.uint16)


# ---------------------------------------------------------------- tests

def test_reference_rules():
    """The reference itself on the values the format's description names."""
    assert ref_scale_exp(bf16_bits([0, 6, 6.03125, 3, 1, 2.0**-130, (2 - 2.0**-7) * 2.0**127, 1.5 * 2.0**127])).tolist() == \
        [0, 0, 1, -1, -2, -126, 125, 125]
    x = bf16_bits([6] + [s * t for t in TIES for s in (1, -1)] + [-0.1015625] + [0] * 16)
    q, s = ref_pack(x)
    codes = np.stack([q & 15, q >> 4], -1).reshape(-1)
    assert s.tolist() == [127]
    assert codes[:16].tolist() == [7, 0, 8, 2, 10, 2, 10, 4, 12, 4, 12, 6, 14, 6, 14, 8]


@pytest.mark.parametrize("case", list(CASES))
def test_host_pack_matches_reference(case):
    bits = CASES[case]()
    q, s = host_pack(bits)
    qr, sr = ref_pack(bits)
    assert np.array_equal(s, sr)
    assert np.array_equal(q, qr)
    assert s[s != 0xFF].min() >= 1 and s[s != 0xFF].max() <= 252


@pytest.mark.parametrize("case", list(CASES))
def test_host_unpack_matches_reference(case):
    q, s = ref_pack(CASES[case]())
    out = host_unpack(q, s)
    assert np.array_equal(out, ref_unpack(q, s))
    assert not (((out & 0x7FFF) == 0x7F80).any())  # nothing packed unpacks to inf
    assert np.array_equal((out & 0x7FFF) > 0x7F80, np.repeat(s == 0xFF, 32))


def every_code_and_scale():
    """65536 blocks: block b has scale byte b % 256 and q bytes (b // 256 + 16 i + j) % 256, so
    every (q byte, scale byte) pair occurs. 1 MiB of q."""
    b = np.arange(65536)
    q = ((b // 256)[:, None] + np.arange(16) * 16 + (b % 16)[:, None]) % 256
    return q.astype(np.uint8).reshape(-1), (b % 256).astype(np.uint8)


def test_host_unpack_every_code_and_scale_byte():
    q, s = every_code_and_scale()
    pairs = np.unique(q.reshape(-1, 16).astype(np.int64) * 256 + s[:, None])
    assert len(pairs) == 65536
    assert np.array_equal(host_unpack(q, s), ref_unpack(q, s))


def test_sizes():
    ps, ss = _core.mxfp4_packed_size, _core.mxfp4_source_size
    # n/2 + n/32 bytes for the n = chunk / 2 elements of a chunk: 17/64 of the source bytes
    assert ps(2 * MiB + 64, MiB) == 2 * (256 * KiB + 16 * KiB) + 17
    assert ps(4 * MiB + 64, 2 * MiB) == 2 * (512 * KiB + 32 * KiB) + 17
    assert ps(64 * MiB, 64 * MiB) == 17 * MiB
    for src, chunk in [(3 * MiB, MiB), (3 * MiB + 4096, MiB), (64, MiB), (64 * 1031, 4096), (MiB + 64, 4096)]:
        assert ps(src, chunk) == sum(min(chunk, src - o) * 17 // 64 for o in range(0, src, chunk))
        assert ss(ps(src, chunk), chunk) == src
    for bad in (16, 18, 17 * 64 + 1, ps(MiB, MiB) + 5):
        with pytest.raises(RuntimeError, match="packed mxfp4"):
            ss(bad, MiB)
    with pytest.raises(RuntimeError, match="64 B"):
        _core.mxfp4_pack_layer_host(bytes(96), 4096)


def test_layer_layout_is_per_chunk():
    """A layer with a tail chunk: every packed chunk is [q][scales] of its own source chunk."""
    src, chunk = 64 * 1031, 4096
    bits = np.frombuffer(_core.fill_random_host(src, 11), dtype=np.uint16)
    packed = np.frombuffer(_core.mxfp4_pack_layer_host(bits.tobytes(), chunk), dtype=np.uint8)
    pc = chunk * 17 // 64
    for c, off in enumerate(range(0, src, chunk)):
        part = bits[off // 2: (off + min(chunk, src - off)) // 2]
        q, s = ref_pack(part)
        got = packed[c * pc: c * pc + len(q) + len(s)]
        assert np.array_equal(got, np.concatenate([q, s])), c
    out = np.frombuffer(_core.mxfp4_unpack_layer_host(packed.tobytes(), src, chunk), dtype=np.uint16)
    assert np.array_equal(out, np.concatenate(
        [ref_unpack(*ref_pack(bits[o // 2: (o + min(chunk, src - o)) // 2])) for o in range(0, src, chunk)]))
