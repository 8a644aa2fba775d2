"""The gfx950 fp8 kernels (csrc/kernels/fp8.hip, the fused check in crc32c.hip) against the numpy
reference and the inputs of test_fp8_host.py, and against the host codec (csrc/core/fp8.cc): exact
equality of every byte, no tolerances. Every scale exponent from -126 to 120, every block size,
every code at every scale, the amax in every lane of its group."""
import functools

import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import ops

from test_fp8_host import (BLOCKS, CASES, assert_bf16_equal, chunked_image, every_code_and_scale, host_pack,
                           host_unpack, out_of_format, ref_pack, ref_unpack)

pytestmark = pytest.mark.gpu

KiB = 1 << 10


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits_tensor(bits):
    return _dev(np.asarray(bits, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def _np(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _assert_codes_equal(got, want, bits):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), [(int(i), hex(bits[i]), hex(got[i]), hex(want[i])) for i in bad[:16]])


# ---------------------------------------------------------------- pack

@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("block", BLOCKS)
def test_pack_matches_reference(gpu, block, case):
    """Scales bit for bit and codes byte for byte, NaN codes and signed zeros included."""
    bits = CASES[case](block)
    q, s = ops.fp8_pack(_bits_tensor(bits), block)
    qr, sr = ref_pack(bits, block)
    assert np.array_equal(_np(s).view(np.uint32), sr.view(np.uint32))
    _assert_codes_equal(_np(q), qr, bits)


@pytest.mark.parametrize("block", BLOCKS)
def test_pack_chunks_matches_host_layout(gpu, block):
    """The ladder image cut on an 8 KiB source-chunk grid (the last chunk is short): the kernel's
    packed layer equals the host codec's byte for byte."""
    bits = CASES["ladder"](block)
    size, chunk = 2 * len(bits), 8 * KiB
    assert size % chunk and size > chunk
    got = ops.fp8_pack_layer(_bits_tensor(bits), chunk, block)
    want = gpu.fp8_pack_layer_host(bits.tobytes(), chunk, block)
    assert got.numel() == gpu.fp8_packed_size(size, chunk, block) == len(want)
    assert _np(got).tobytes() == want
    assert want == chunked_image(*ref_pack(bits, block), block, chunk)


def _partial_counts(block):
    k = 1
    while not (block * k // 8 > 256 and (block * k // 8) % 256):
        k += 2
    return [1, k]


@pytest.mark.parametrize("block,k", [(b, k) for b in BLOCKS for k in _partial_counts(b)])
def test_pack_partial_wave_and_workgroup(gpu, block, k):
    """n = block: one block in one partial wave (block 512: exactly one wave); n = block * k with
    more than one workgroup and a last one that is partly inactive. The writes end where they must."""
    n = block * k
    bits = np.frombuffer(gpu.fill_random_host(2 * n, 5 + block), dtype=np.uint16)
    ns = 4 * (n // block)
    guard = torch.full((n + 32 + ns + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    x = _bits_tensor(bits)
    q, s = ops.fp8_pack(x, block)
    gpu.fp8_pack(x.data_ptr(), n, guard.data_ptr(), guard.data_ptr() + n + 32, block, 0)
    torch.cuda.synchronize()
    qr, sr = ref_pack(bits, block)
    assert np.array_equal(_np(q), qr) and np.array_equal(_np(s).view(np.uint32), sr.view(np.uint32))
    g = _np(guard)
    assert np.array_equal(g[:n], qr) and (g[n: n + 32] == 0xA5).all()
    assert g[n + 32: n + 32 + ns].tobytes() == sr.tobytes() and (g[n + 32 + ns:] == 0xA5).all()


# ---------------------------------------------------------------- unpack

SOURCES = ["every_code_and_scale"] + list(CASES)


@functools.lru_cache(maxsize=None)
def _unpack_case(source, block):
    """(q, scales, exact mask, ref_unpack of it): computed once per input, left unchanged."""
    if source == "every_code_and_scale":
        q, s, exact = every_code_and_scale(block)
    else:
        q, s = ref_pack(CASES[source](block), block)
        exact = np.ones(len(q), dtype=bool)
    want = ref_unpack(q, s, block)
    for a in (q, s, exact, want):
        a.setflags(write=False)
    return q, s, exact, want


def _check(got, exact, want):
    assert_bf16_equal(got.view(np.uint16)[exact], want[exact])


def _chunk_crcs(gpu, image, pchunk):
    return [gpu.crc32c(image[o: o + pchunk]) for o in range(0, len(image), pchunk)]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("block", BLOCKS)
def test_unpack_matches_reference(gpu, block, source):
    """The stand-alone kernel: bit for bit (any NaN matches any NaN)."""
    q, s, exact, want = _unpack_case(source, block)
    y = ops.fp8_unpack(_dev(q), _dev(s), block)
    _check(_np(y), exact, want)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("block", BLOCKS)
def test_fused_single_chunk_matches_reference(gpu, block, source):
    """fp8_verify_unpack on one chunk [q][scales]: the q/scale boundary is wherever the input ends
    (off the 16 KiB segment grid for every input but the 65 536 patterns)."""
    q, s, exact, want = _unpack_case(source, block)
    size = 2 * len(q)
    chunk = -(-size // 4096) * 4096
    image = q.tobytes() + s.tobytes()
    out = torch.full((len(q) + 64,), -1, dtype=torch.int16, device="cuda")
    p = _dev(np.frombuffer(image, dtype=np.uint8))
    crcs = gpu.fp8_verify_unpack(p.data_ptr(), size, chunk, block, out.data_ptr())
    assert crcs == [gpu.crc32c(image)]
    got = out.cpu().numpy()
    _check(got[: len(q)], exact, want)
    assert (got[len(q):] == -1).all()


@pytest.mark.parametrize("cus", [0, 1])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("block", BLOCKS)
def test_fused_chunk_grid_matches_reference(gpu, block, source, cus):
    """fp8_verify_unpack on an 8 KiB source-chunk grid (a short last chunk wherever the input is no
    multiple of 4096 elements), sized for every CU and for one."""
    q, s, exact, want = _unpack_case(source, block)
    size, chunk = 2 * len(q), 8 * KiB
    image = chunked_image(q, s, block, chunk)
    assert len(image) == gpu.fp8_packed_size(size, chunk, block)
    out = torch.full((len(q) + 64,), -1, dtype=torch.int16, device="cuda")
    p = _dev(np.frombuffer(image, dtype=np.uint8))
    crcs = gpu.fp8_verify_unpack(p.data_ptr(), size, chunk, block, out.data_ptr(), cus=cus)
    assert crcs == _chunk_crcs(gpu, image, chunk // 2 + chunk // 2 // block * 4)
    got = out.cpu().numpy()
    _check(got[: len(q)], exact, want)
    assert (got[len(q):] == -1).all()
    if cus == 0:  # the ops form, on the caller's stream
        y, c = ops.fp8_verify_unpack(p, size, chunk, block)
        assert ops.crc32c_values(c) == crcs
        _check(_np(y), exact, want)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("block", BLOCKS)
def test_fused_batch_matches_reference(gpu, block, source):
    """fp8_verify_unpack_batch: the input cut into up to crc32c_batch_max independent chunks of
    mixed sizes (one block, a few blocks, more than a 16 KiB segment, the rest)."""
    q, s, exact, want = _unpack_case(source, block)
    nmax, nb = gpu.crc32c_batch_max(), len(q) // block
    cuts, at = [0], 0
    for i in range(nmax - 1):
        at += [1, 3, 16 * KiB // block + 1, 2, 5 * KiB // block + 1][i % 5]
        if at >= nb:
            break
        cuts.append(at)
    cuts.append(nb)
    pieces = [(cuts[i] * block, cuts[i + 1] * block) for i in range(len(cuts) - 1)]
    images = [q[a:b].tobytes() + s[a // block: b // block].tobytes() for a, b in pieces]
    dev = [_dev(np.frombuffer(im, dtype=np.uint8)) for im in images]
    outs, crcs = ops.fp8_verify_unpack_chunks([(d, 2 * (b - a)) for d, (a, b) in zip(dev, pieces)], block)
    assert ops.crc32c_values(crcs) == [gpu.crc32c(im) for im in images]
    _check(np.concatenate([_np(y) for y in outs]), exact, want)


@pytest.mark.parametrize("block", BLOCKS)
def test_out_of_format_codes_agree(gpu, block):
    """Codes +-0x78..0x7E at E = 120 (256 * 2^120 and more: beyond bf16) are never written by pack
    and their value is unspecified (core/fp8.h); the host codec, the stand-alone kernel and the
    fused kernel still give the same bits."""
    q, s = out_of_format(block)
    host = host_unpack(q, s, block)
    y = ops.fp8_unpack(_dev(q), _dev(s), block)
    assert_bf16_equal(_np(y), host)
    image = q.tobytes() + s.tobytes()
    f, c = ops.fp8_verify_unpack(_dev(np.frombuffer(image, dtype=np.uint8)), 2 * len(q), 4096, block)
    assert ops.crc32c_values(c) == [gpu.crc32c(image)]
    assert_bf16_equal(_np(f), host)


def test_nan_codes_unpack_to_the_same_bits(gpu):
    """Codes 0x7F and 0xFF at the lowest, the unit and the highest scale: host codec, stand-alone
    kernel and fused kernel write the same NaN bits, 0xFFC0 (core/fp8.h), not just some NaN."""
    block = 32
    q = np.tile(np.array([0x7F, 0xFF, 0x38, 0xFF, 0x7F, 0xB8, 0x00, 0x7F], dtype=np.uint8), 3 * block // 8)
    s = np.array([2.0**-126, 1.0, 2.0**120], dtype=np.float32)
    host = host_unpack(q, s, block)
    assert set(host[(q & 0x7F) == 0x7F].tolist()) == {0xFFC0}
    y = _np(ops.fp8_unpack(_dev(q), _dev(s), block)).view(np.uint16)
    assert y.tolist() == host.tolist()
    f, _ = ops.fp8_verify_unpack(_dev(np.frombuffer(q.tobytes() + s.tobytes(), dtype=np.uint8)), 2 * len(q), 4096, block)
    assert _np(f).view(np.uint16).tolist() == host.tolist()


def test_host_pack_equals_kernel_on_random_bit_patterns(gpu):
    """Random payload bytes as bf16 (NaNs of both signs, +-inf, the top binade): host codec and
    kernel give the same bytes, NaN codes and the signs of underflowed values included."""
    bits = np.frombuffer(gpu.fill_random_host(1 << 20, 3), dtype=np.uint16)
    for block in BLOCKS:
        q, s = ops.fp8_pack(_bits_tensor(bits), block)
        hq, hs = host_pack(bits, block)
        assert _np(s).tobytes() == hs.tobytes()
        _assert_codes_equal(_np(q), hq, bits)
