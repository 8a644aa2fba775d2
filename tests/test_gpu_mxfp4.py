"""The gfx950 MXFP4 kernels (csrc/kernels/mxfp4.hip, the fused check in crc32c.hip) against
the host codec (csrc/core/mxfp4.cc) and the numpy reference of test_mxfp4_host.py: exact
equality of every byte, no tolerances. Then one-GPU sessions with --pack mxfp4."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import ops
from distributed_llm_dissemination_amd.models.catalog import make_workload
from distributed_llm_dissemination_amd.parallel.runtime import Runtime

from test_mxfp4_host import CASES, every_code_and_scale, host_pack, ref_pack, ref_unpack

pytestmark = pytest.mark.gpu

MiB = 1 << 20


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits_tensor(bits):
    return _dev(bits.view(np.int16)).view(torch.bfloat16)


def _np(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _random_bits(n, seed, gpu):
    return np.frombuffer(gpu.fill_random_host(2 * n, seed), dtype=np.uint16)


# ---------------------------------------------------------------- pack

@pytest.mark.parametrize("case", list(CASES))
def test_pack_matches_reference(gpu, case):
    bits = CASES[case]()
    q, s = ops.mxfp4_pack(_bits_tensor(bits))
    qr, sr = ref_pack(bits)
    assert np.array_equal(_np(s), sr)
    assert np.array_equal(_np(q), qr)
    hq, hs = host_pack(bits)
    assert np.array_equal(hq, qr) and np.array_equal(hs, sr)


@pytest.mark.parametrize("n", [32, 32 * 257])
def test_pack_partial_wave_and_workgroup(gpu, n):
    """n = 32: one block in one partial wave; n = 32 * 257: a last workgroup that is partly inactive."""
    bits = _random_bits(n, 5, gpu)
    guard = torch.full((n // 2 + 32 + n // 32 + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    x = _bits_tensor(bits)
    q, s = ops.mxfp4_pack(x)
    gpu.mxfp4_pack(x.data_ptr(), n, guard.data_ptr(), guard.data_ptr() + n // 2 + 32, 0)  # writes end where they must
    torch.cuda.synchronize()
    qr, sr = ref_pack(bits)
    assert np.array_equal(_np(q), qr) and np.array_equal(_np(s), sr)
    g = _np(guard)
    assert np.array_equal(g[: n // 2], qr) and (g[n // 2: n // 2 + 32] == 0xA5).all()
    assert np.array_equal(g[n // 2 + 32: n // 2 + 32 + n // 32], sr) and (g[n // 2 + 32 + n // 32:] == 0xA5).all()


LAYERS = [(3 * MiB + 4096, MiB), (64 * 1031, 4096)]


@pytest.fixture(scope="module")
def layers(gpu):
    """Per (size, chunk): the source bits, the host-packed image and its host unpack (computed once)."""
    out = {}
    for size, chunk in LAYERS + [(64, 4096)]:
        raw = gpu.fill_random_host(size, 17 + size % 251)
        packed = gpu.mxfp4_pack_layer_host(raw, chunk)
        out[size, chunk] = (raw, packed, gpu.mxfp4_unpack_layer_host(packed, size, chunk))
    return out


@pytest.mark.parametrize("size,chunk", LAYERS)
def test_pack_chunks_matches_host_layout(gpu, layers, size, chunk):
    raw, packed, _ = layers[size, chunk]
    x = _dev(np.frombuffer(raw, dtype=np.int16)).view(torch.bfloat16)
    got = ops.mxfp4_pack_layer(x, chunk)
    assert got.numel() == gpu.mxfp4_packed_size(size, chunk) == len(packed)
    assert _np(got).tobytes() == packed


# ---------------------------------------------------------------- unpack

def test_unpack_every_code_and_scale_byte(gpu):
    """65536 blocks (1 MiB of q) holding every (q byte, scale byte) pair: bf16-subnormal results
    (scale bytes 0 and 1), overflow (253, 254) and NaN blocks (0xFF) included."""
    q, s = every_code_and_scale()
    y = ops.mxfp4_unpack(_dev(q), _dev(s))
    assert np.array_equal(_np(y).view(np.uint16), ref_unpack(q, s))


@pytest.mark.parametrize("case", list(CASES))
def test_unpack_of_packed_patterns(gpu, case):
    q, s = ref_pack(CASES[case]())
    y = ops.mxfp4_unpack(_dev(q), _dev(s))
    assert np.array_equal(_np(y).view(np.uint16), ref_unpack(q, s))


# ---------------------------------------------------------------- fused verify + unpack

def _chunk_crcs(gpu, packed, pchunk):
    return [gpu.crc32c(packed[o: o + pchunk]) for o in range(0, len(packed), pchunk)]


@pytest.mark.parametrize("cus", [0, 32])
@pytest.mark.parametrize("size,chunk", LAYERS + [(64, 4096)])
def test_fused_verify_unpack_layer(gpu, layers, size, chunk, cus):
    """CRC32C of each packed chunk and the bf16 layer in one pass; (64 * 1031, 4096) puts the
    q/scale boundary off the 1 KiB and 16 KiB grids, 64 B is one block (packed length 17)."""
    _, packed, want = layers[size, chunk]
    p = _dev(np.frombuffer(packed, dtype=np.uint8))
    out = torch.full((size // 2 + 64,), -1, dtype=torch.int16, device="cuda")
    crcs = gpu.mxfp4_verify_unpack(p.data_ptr(), size, chunk, out.data_ptr(), 0, cus)
    assert crcs == _chunk_crcs(gpu, packed, chunk * 17 // 64)
    got = out.cpu().numpy()
    assert got[: size // 2].tobytes() == want and (got[size // 2:] == -1).all()
    # the stand-alone unpack kernel agrees chunk by chunk
    for c, off in enumerate(range(0, size, chunk)):
        n = min(chunk, size - off) // 2
        base = c * (chunk * 17 // 64)
        y = ops.mxfp4_unpack(p[base: base + n // 2].clone(), p[base + n // 2: base + n // 2 + n // 32].clone())
        assert _np(y).tobytes() == want[off: off + 2 * n]
    # ops form on the caller's stream
    y, c = ops.mxfp4_verify_unpack(p, size, chunk)
    assert ops.crc32c_values(c) == crcs and _np(y).tobytes() == want


def _mixed_chunks(gpu):
    lens = [64, 4096, 64 * 1031, MiB, 192, 64 * 257, 2 * MiB, 64 * 1024, 128, 640, MiB + 64, 4096 * 3, 64 * 255,
            16384 * 4, 64 * 4097, 320]
    chunks = []
    for i, n in enumerate(lens):
        raw = gpu.fill_random_host(n, 100 + i)
        packed = gpu.mxfp4_pack_layer_host(raw, 4 * MiB)
        chunks.append((n, packed, gpu.mxfp4_unpack_layer_host(packed, n, 4 * MiB)))
    return chunks


def test_fused_batch_of_mixed_chunks(gpu):
    chunks = _mixed_chunks(gpu)
    assert len(chunks) == gpu.crc32c_batch_max() == 16
    dev = [_dev(np.frombuffer(p, dtype=np.uint8)) for _, p, _ in chunks]
    outs, crcs = ops.mxfp4_verify_unpack_chunks([(d, n) for d, (n, _, _) in zip(dev, chunks)])
    assert ops.crc32c_values(crcs) == [gpu.crc32c(p) for _, p, _ in chunks]
    for y, (_, _, want) in zip(outs, chunks):
        assert _np(y).tobytes() == want


def test_fused_detects_corruption_in_the_scale_region(gpu, layers):
    size, chunk = LAYERS[0]
    _, packed, _ = layers[size, chunk]
    pchunk = chunk * 17 // 64
    want = _chunk_crcs(gpu, packed, pchunk)
    bad = bytearray(packed)
    victim = 1 * pchunk + chunk // 4 + 777  # a scale byte of chunk 1
    bad[victim] ^= 0x10
    p = _dev(np.frombuffer(bytes(bad), dtype=np.uint8))
    out = torch.empty(size // 2, dtype=torch.bfloat16, device="cuda")
    got = gpu.mxfp4_verify_unpack(p.data_ptr(), size, chunk, out.data_ptr())
    assert got[1] != want[1] and got[1] == gpu.crc32c(bytes(bad[pchunk: 2 * pchunk]))
    assert [g for i, g in enumerate(got) if i != 1] == [w for i, w in enumerate(want) if i != 1]


# ---------------------------------------------------------------- sessions

@pytest.mark.parametrize("tier,store", [("host", "packed"), ("device", "packed"), ("host", "bf16")])
def test_mxfp4_packed_session(gpu, tier, store):
    """--pack mxfp4 on one GPU: bf16 sources are packed on the copy stream while staging; the HBM
    slot holds the packed image the manifest was computed on; the fused verify+unpack restores
    the bf16 layer. The engine counts staged bytes at the source (bf16) and verified bytes on
    the packed grid, so a fully verified session has bytes_verified == packed_size(bytes_staged)."""
    size, L = 3 * MiB + 4096, 3
    cfg = make_workload(1, L, size, tier=tier, chunk_bytes=MiB)
    rt = Runtime(cfg, 0, engine="rccl", chunk_bytes=MiB, registry={0: "127.0.0.1:0"}, pack="mxfp4", store=store)
    try:
        assert rt.pack_block == 32 and rt.slot_sizes[0] == gpu.mxfp4_packed_size(size, MiB)
        images = {l: rt.layer_bytes(l) for l in range(L)}  # after materialize: the packed image
        staged = L if tier == "host" else 0
        for _ in range(2):
            res = rt.run(1, timeout=60)
            assert res.ok, res.error
            assert res.engine_stats["verify_failures"] == 0
            assert res.engine_stats["bytes_staged"] == staged * size
            assert res.engine_stats["bytes_verified"] == staged * gpu.mxfp4_packed_size(size, MiB)
            for l in range(L):
                assert rt.layer_bytes(l) == images[l]
                want = gpu.mxfp4_unpack_layer_host(images[l], size, MiB)
                assert rt.unpacked_layer_bytes(l) == want
                if store == "bf16":
                    t = rt.layer_tensor(l, unpacked=True)
                    assert t.is_cuda and t.numel() == size and t.data_ptr() == rt.engine.unpacked_ptr(l)
                    assert t.cpu().numpy().tobytes() == want
    finally:
        rt.close()


# ---------------------------------------------------------------- ops wrappers

def test_ops_roundtrip_on_the_callers_stream(gpu):
    bits = CASES["permuted"]()
    x = _bits_tensor(bits)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        q, s = ops.mxfp4_pack(x)
        y = ops.mxfp4_unpack(q.view(torch.float4_e2m1fn_x2), s.view(torch.float8_e8m0fnu))
    st.synchronize()
    assert q.dtype == torch.uint8 and q.numel() == 32768 and s.dtype == torch.uint8 and s.numel() == 2048
    assert np.array_equal(_np(y).view(np.uint16), ref_unpack(*ref_pack(bits)))


def test_ops_reject_bad_inputs(gpu):
    x = torch.zeros(64 + 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="bfloat16"):
        ops.mxfp4_pack(x[:64].float())
    with pytest.raises(ValueError, match="aligned"):
        ops.mxfp4_pack(x[1:65])
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.mxfp4_pack(x[:48])
    with pytest.raises(ValueError, match="one byte per 16"):
        ops.mxfp4_unpack(torch.zeros(32, dtype=torch.uint8, device="cuda"), torch.zeros(3, dtype=torch.uint8, device="cuda"))
