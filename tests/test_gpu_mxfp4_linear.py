"""The gfx950 W4A16 linear (csrc/kernels/mxfp4_linear.hip, ops.mxfp4_linear): bf16 activations
times MXFP4 weights read in place from a packed layer, against the numpy reference of
test_mxfp4_linear_host.py (ref_unpack per chunk of the layer, sliced to the parameter, float64
matmul). Exact inputs are compared for equality, random ones against a bound derived from f32
accumulation; then a session whose forward pass runs from the packed HBM slot."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import ops
from distributed_llm_dissemination_amd.models.catalog import make_workload
from distributed_llm_dissemination_amd.models.weights import (PRESETS, PackedParam, decoder_forward, flatten,
                                                             layer_nbytes, random_layer)
from distributed_llm_dissemination_amd.parallel.runtime import Runtime

from test_mxfp4_linear_host import (bf16_tensor_bits, bits_to_f64, chunk_table, handmade_image, int_x, ref_layer_bits,
                                    ref_weight, scale_index)

pytestmark = pytest.mark.gpu

KiB = 1 << 10


def _linear(x, img, n, k, total, chunk, off=0, **kw):
    p = img if torch.is_tensor(img) else torch.from_numpy(img).cuda()
    return ops.mxfp4_linear(x.cuda(), p, n, k, src_bytes=2 * total, chunk_bytes=chunk, elem_offset=off, **kw)


# Every value of M in {1, 5, 16, 17, 64, 65} (a partial tile, the second and the fifth
# accumulator tile: 65 takes a second pass), N in {16, 48, 528} and K in {32, 96, 128, 160,
# 1056} (the K tail alone, a main loop alone, both). split_k 0 is the launcher's choice; the
# others force K slices that leave waves without a step (K = 160 has one step of 128: 15 of 16
# waves are empty and the last one takes the tail; 8 steps over 5 or 3 slices split unevenly).
EXACT = [
    (1, 16, 32, 0), (5, 48, 96, 0), (16, 528, 128, 0), (17, 48, 160, 0), (64, 16, 1056, 0), (65, 528, 1056, 0),
    (1, 528, 1056, 0), (65, 48, 32, 0), (17, 528, 96, 0), (64, 48, 128, 0), (16, 16, 1056, 1),
    (5, 48, 160, 16), (17, 16, 1056, 5), (64, 48, 1056, 3), (1, 16, 128, 4),
    # wide layers, where a wave feeds 2 row tiles (from 256 tiles on) or 4 (from 1024 on, up to
    # 32 rows of x) from one x fragment
    (5, 8192, 160, 0), (64, 8192, 160, 0), (65, 8192, 128, 2), (16, 4128, 160, 0), (17, 4128, 1056, 0),
    (1, 8192, 1056, 8), (17, 16384, 160, 0), (64, 16384, 96, 0), (1, 16384, 128, 0),
]


@pytest.mark.parametrize("m,n,k,split_k,row_tiles", [(5, 64, 160, 0, 4), (17, 64, 1056, 3, 4), (32, 128, 96, 2, 4),
                                                      (64, 32, 160, 0, 2), (65, 96, 1056, 5, 2), (1, 32, 32, 0, 2),
                                                      (33, 64, 128, 0, 4)])
def test_exact_with_several_row_tiles_per_wave(gpu, m, n, k, split_k, row_tiles):
    """The wide-layer paths at small sizes: 2 or 4 row tiles per wave forced (beyond 32 rows of x,
    4 becomes 2), 1024-B chunks so that the tiles of one wave lie in different chunks."""
    off, chunk = 32 * 7, 1024
    total = off + n * k
    img = handmade_image(total, chunk, m + n + k)
    x, xf = int_x(m, k, 11 + m)
    want = xf @ ref_weight(img, total, chunk, off, n, k).T
    y = _linear(x, img, n, k, total, chunk, off, out_dtype=torch.float32, split_k=split_k, row_tiles=row_tiles)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), want)
    with pytest.raises(ValueError, match="row_tiles"):
        _linear(x, img, n, k, total, chunk, off, row_tiles=3)


@pytest.mark.parametrize("m,n,k,split_k", EXACT)
def test_exact_on_integer_inputs(gpu, m, n, k, split_k):
    """x: integers in [-8, 8]; W: random codes with scale bytes in {126, 127, 128}, so every
    product is a multiple of 2^-2 and |sum| <= 1056 * 96 < 2^24 * 2^-2: every partial sum, in any
    order, is exact in f32, and the f32 output equals the reference. Random codes make W
    asymmetric: a transposed or permuted fragment map cannot pass. 64 KiB chunks with the
    parameter at element 32 * 3 of a layer that goes on behind it."""
    off, chunk = 32 * 3, 64 * KiB
    total = off + n * k + 64
    img = handmade_image(total, chunk, 1000 * m + n + k)
    x, xf = int_x(m, k, m + 7 * k)
    want = xf @ ref_weight(img, total, chunk, off, n, k).T
    y = _linear(x, img, n, k, total, chunk, off, out_dtype=torch.float32, split_k=split_k)
    assert y.dtype == torch.float32 and y.shape == (m, n)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), want)


# (chunk bytes, element offset, elements behind the parameter)
LAYOUTS = {
    "rows straddle 1024-B chunks": (1024, 32 * 7, 32 * 5),
    "last rows in a short tail chunk": (1024, 32 * 7, 0),
    "the same parameter at 64 KiB": (64 * KiB, 32 * 7, 0),
    "64 KiB chunks crossed mid-row": (64 * KiB, 32 * 1021, 32),
}


@pytest.mark.parametrize("m,n,k", [(5, 48, 96), (17, 528, 160), (16, 48, 1056)])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_exact_across_chunk_layouts(gpu, layout, m, n, k):
    """K = 96 at 1024-B chunks (512 elements) starting at element 224: chunk boundaries fall
    inside rows and inside 128-element steps; with nothing behind the parameter its last rows
    lie in the layer's short tail chunk."""
    chunk, off, behind = LAYOUTS[layout]
    total = off + n * k + behind
    if layout == "last rows in a short tail chunk":
        assert 0 < total % (chunk // 2) < k * 4
    img = handmade_image(total, chunk, 77 + k)
    x, xf = int_x(m, k, 5 + m)
    want = xf @ ref_weight(img, total, chunk, off, n, k).T
    for split_k in (0, 2):
        y = _linear(x, img, n, k, total, chunk, off, out_dtype=torch.float32, split_k=split_k)
        assert np.array_equal(y.cpu().numpy().astype(np.float64), want), split_k


@pytest.fixture(scope="module")
def random_case(gpu):
    """Per (m, n, k): x ~ N(0, 1) in bf16, W ~ N(0, 1/k) packed by ops.mxfp4_pack_layer (4 KiB
    chunks), the f32 and bf16 outputs, and the float64 reference with its error bound."""
    out = {}
    g = torch.Generator().manual_seed(12)
    for m, n, k in [(5, 48, 160), (64, 528, 1056), (17, 16, 1056), (1, 528, 128)]:
        x = torch.randn(m, k, generator=g).to(torch.bfloat16)
        w = (torch.randn(n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
        total = n * k
        packed = ops.mxfp4_pack_layer(w.view(-1).cuda(), 4096)
        img = packed.cpu().numpy()
        sb = np.concatenate([img[so: so + c // 32] for _, c, _, so in chunk_table(total, 4096)])
        assert sb.min() >= 100 and sb.max() <= 140  # far from bf16-subnormal weights
        wf = ref_weight(img, total, 4096, 0, n, k)
        xf = bits_to_f64(bf16_tensor_bits(x)).reshape(m, k)
        y32 = _linear(x, packed, n, k, total, 4096, out_dtype=torch.float32)
        y16 = _linear(x, packed, n, k, total, 4096)
        out[m, n, k] = dict(x=x, packed=packed, total=total, want=xf @ wf.T, bound=k * 2.0 ** -23 * (np.abs(xf) @ np.abs(wf).T),
                            y32=y32, y16=y16)
    return out


@pytest.mark.parametrize("m,n,k", [(5, 48, 160), (64, 528, 1056), (17, 16, 1056), (1, 528, 128)])
def test_random_within_f32_accumulation_error(gpu, random_case, m, n, k):
    """bf16 x bf16 products are exact in f32 and each of the K additions errs by at most one
    unit roundoff of the running sum, itself at most sum |x w|: |y - y_ref| <= K 2^-23 sum_k
    |x_k w_k| per element (2^-23 allows truncating instead of nearest internal rounding)."""
    c = random_case[m, n, k]
    err = np.abs(c["y32"].cpu().numpy().astype(np.float64) - c["want"])
    print("max err / bound", float((err / c["bound"]).max()))
    assert (err <= c["bound"]).all()


@pytest.mark.parametrize("m,n,k", [(5, 48, 160), (64, 528, 1056)])
def test_bf16_output_is_the_rounded_f32_output(gpu, random_case, m, n, k):
    c = random_case[m, n, k]
    assert c["y16"].dtype == torch.bfloat16
    assert np.array_equal(bf16_tensor_bits(c["y16"]), bf16_tensor_bits(c["y32"].to(torch.bfloat16)))  # nearest even


@pytest.mark.parametrize("m,n,k", [(17, 16, 1056), (64, 528, 1056)])
def test_deterministic(gpu, random_case, m, n, k):
    """Equal bits from call to call, split-K reduction included (16 rows of 1056: 8 slices)."""
    c = random_case[m, n, k]
    assert gpu.mxfp4_linear_slices(m, n, k) > 1
    for _ in range(2):
        again = _linear(c["x"], c["packed"], n, k, c["total"], 4096, out_dtype=torch.float32)
        assert torch.equal(again.view(torch.int32), c["y32"].view(torch.int32))


def test_nan_block_poisons_only_its_row(gpu):
    m, n, k, chunk, off = 17, 48, 160, 1024, 32 * 7
    total = off + n * k
    img = handmade_image(total, chunk, 9)
    x, _ = int_x(m, k, 3)
    clean = _linear(x, img, n, k, total, chunk, off, out_dtype=torch.float32).cpu()
    for r, blk in [(21, 0), (47, 4), (0, 3)]:  # blocks of the main loop and of the K tail
        bad = img.copy()
        bad[scale_index(total, chunk, off + r * k + 32 * blk)] = 0xFF
        y = _linear(x, bad, n, k, total, chunk, off, out_dtype=torch.float32).cpu()
        assert torch.isnan(y[:, r]).all()
        keep = [c for c in range(n) if c != r]
        assert torch.equal(y[:, keep].view(torch.int32), clean[:, keep].view(torch.int32))
        y16 = _linear(x, bad, n, k, total, chunk, off).cpu()
        assert torch.isnan(y16[:, r]).all() and not torch.isnan(y16[:, keep]).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("split_k", [1, 4])
def test_writes_only_its_output(gpu, dtype, split_k):
    """M = 5 is padded to a 16-row tile by masking: with y a view into a 0xA5-filled buffer and a
    row stride larger than N, every byte outside y[:M, :N] is unchanged."""
    m, n, k, chunk = 5, 48, 1056, 1024
    total = n * k
    img = handmade_image(total, chunk, 31)
    x, xf = int_x(m, k, 32)
    es = 2 if dtype == torch.bfloat16 else 4
    ld, lead = 80, 3 * 80 + 8
    buf = torch.full(((lead + (m + 3) * ld) * es,), 0xA5, dtype=torch.uint8, device="cuda")
    y = buf.view(dtype)[lead: lead + m * ld].view(m, ld)[:, :n]
    got = _linear(x, img, n, k, total, chunk, out=y, split_k=split_k)
    assert got.data_ptr() == y.data_ptr()
    want = torch.from_numpy(xf @ ref_weight(img, total, chunk, 0, n, k).T).to(dtype)
    assert torch.equal(y.cpu(), want)
    mask = torch.ones(buf.numel() // es, dtype=torch.bool)
    mask[lead: lead + m * ld].view(m, ld)[:, :n] = False
    outside = buf.cpu().view(-1, es)[mask]
    assert outside.numel() and bool((outside == 0xA5).all())


def test_unpack_range_on_the_gpu(gpu):
    """ops.mxfp4_unpack_range through the unpack kernel, one launch per chunk the range touches."""
    total = 512 * 5 + 96
    for chunk in (1024, 64 * KiB):
        img = handmade_image(total, chunk, 3, scales=tuple(range(0, 253)))
        img[scale_index(total, chunk, 512 + 40)] = 0xFF
        whole = ref_layer_bits(img, total, chunk)
        p = torch.from_numpy(img).cuda()
        for off, n in [(0, total), (32 * 7, 96 * 4), (512 * 4 + 480, 128), (512 + 32, 32), (64, 0)]:
            got = ops.mxfp4_unpack_range(p, 2 * total, chunk, off, n)
            assert got.is_cuda and np.array_equal(bf16_tensor_bits(got), whole[off: off + n]), (chunk, off, n)


def test_rejects_bad_gpu_arguments(gpu):
    total, chunk = 48 * 96, 1024
    p = torch.from_numpy(handmade_image(total, chunk, 1)).cuda()
    x = torch.zeros(5, 96, dtype=torch.bfloat16, device="cuda")
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk)
    with pytest.raises(ValueError, match="same device"):
        ops.mxfp4_linear(x.cpu(), p, 48, 96, **kw)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.mxfp4_linear(x, torch.cat([p, p])[1: 1 + p.numel()], 48, 96, **kw)
    with pytest.raises(ValueError, match="out must be"):
        ops.mxfp4_linear(x, p, 48, 96, out=torch.empty(5, 32, device="cuda"), **kw)
    with pytest.raises(ValueError, match="outside"):
        ops.mxfp4_linear(x, p, 64, 96, **kw)
    with pytest.raises(RuntimeError):  # the launcher checks again on its own
        gpu.mxfp4_linear(p.data_ptr(), 2 * total, chunk, 32, x.data_ptr(), 5, 48, 96, p.data_ptr(), 48, False, 0, 0, 0)


def test_forward_from_the_packed_hbm_slot(gpu):
    """rccl engine, `tiny`, 2 layers, 64 KiB chunks, --pack mxfp4 --store packed: the packed
    parameters alias the layer's HBM slot, no bf16 image exists, and the forward pass on the GPU
    from the packed bytes agrees with the CPU pass on the dequantized parameters."""
    spec = PRESETS["tiny"]
    size = layer_nbytes(spec)
    blobs = {l: flatten(random_layer(spec, 7 + l), spec) for l in range(2)}
    cfg = make_workload(1, 2, size, tier="host", chunk_bytes=64 * KiB)
    rt = Runtime(cfg, 0, engine="rccl", chunk_bytes=64 * KiB, registry={0: "127.0.0.1:0"}, pack="mxfp4",
                 store="packed", layer_source=lambda l, n: blobs[l])
    try:
        res = rt.run(1, timeout=60)
        assert res.ok, res.error
        x = torch.randn(1, 16, spec.hidden, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
        for l in range(2):
            p = rt.layer_params(l, spec, packed=True)
            assert rt.engine.unpacked_ptr(l) == 0  # no bf16 image
            for v in p.values():
                assert isinstance(v, PackedParam) and v.packed.is_cuda
                assert v.packed.data_ptr() == rt.engine.device_ptr(l) and v.packed.numel() == rt.slot_sizes[l]
            host = gpu.mxfp4_unpack_layer_host(rt.layer_bytes(l), size, 64 * KiB)
            for name, v in p.items():
                d = v.dequantize()
                assert d.is_cuda
                first = 2 * v.elem_offset
                assert d.cpu().view(-1).view(torch.uint8).numpy().tobytes() == host[first: first + 2 * d.numel()], name
            y = decoder_forward(x.cuda(), p, spec).float().cpu()
            y0 = decoder_forward(x, {k: v.dequantize().cpu() for k, v in p.items()}, spec).float()
            rel = float((y - y0).norm() / y0.norm())
            print("layer", l, "relative error", rel)
            assert rel < 2e-2
    finally:
        rt.close()
