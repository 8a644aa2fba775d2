"""The gfx950 W6A16 linear (csrc/kernels/mxfp6_linear.hip, ops.mxfp6_linear): bf16 activations
times e2m3 weights read in place from an MXFP6-packed layer, against the numpy reference of
test_mxfp6_linear_host.py (ref_unpack per chunk of the layer, sliced to the parameter, float64
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

from test_mxfp6_linear_host import (bf16_tensor_bits, bits_to_f64, block_index, handmade_image, int_x, prove_exact_ints,
                                    ref_weight)

pytestmark = pytest.mark.gpu

KiB = 1 << 10


def _linear(x, img, n, k, total, chunk, off=0, **kw):
    p = img if torch.is_tensor(img) else torch.from_numpy(img).cuda()
    return ops.mxfp6_linear(x.cuda(), p, n, k, src_bytes=2 * total, chunk_bytes=chunk, elem_offset=off, **kw)


def _exact(m, n, k, total, chunk, off, seed, **kw):
    """x: integers in [-8, 8]; W: every e2m3 code, every block with its own scale byte from
    {126, 127, 128}: multiples of 2^-4 of magnitude at most 15. prove_exact_ints shows on the
    reference that every partial sum, in any order, is exact in f32, so the f32 output equals the
    float64 reference. Random codes and per-block scales make W asymmetric: a transposed fragment
    map, a wrong k permutation or a wrong scale index cannot pass."""
    assert total % 32 == 0 and off + n * k <= total
    img = handmade_image(total, chunk, seed)
    x, xf = int_x(m, k, seed + 1)
    wf = ref_weight(img, total, chunk, off, n, k)
    prove_exact_ints(xf, wf)
    y = _linear(x, img, n, k, total, chunk, off, out_dtype=torch.float32, **kw)
    assert y.dtype == torch.float32 and y.shape == (m, n)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), xf @ wf.T)


# (m, n, k, split_k, block of the layer at which the parameter starts). M in {1, 5, 16, 17, 64, 65}
# (a partial tile, the second and the fifth accumulator tile: 65 takes a second pass), N in
# {16, 48, 528} and K in {32, 96, 128, 160, 1056}: the K tail alone (32, 96), a main loop alone
# (128), both (160, 1056). split_k 0 is the launcher's choice; the others force K slices that leave
# waves without a step (K = 128 and 160 have one step of 128: with 16 slices 15 waves are empty and
# the last one takes the tail; 8 steps over 5 or 3 slices split unevenly). At an odd block the
# codes of every lane are 8-B and not 16-B aligned where K / 32 is even, and alternate row by row
# where it is odd; at an even block it is the other way round.
EXACT = [
    (1, 16, 32, 0, 3), (5, 48, 96, 0, 3), (65, 48, 32, 0, 4), (17, 528, 96, 0, 3), (16, 16, 96, 1, 4),
    (16, 528, 128, 0, 3), (64, 48, 128, 0, 4), (1, 16, 128, 16, 3), (5, 16, 128, 3, 3), (17, 48, 128, 0, 4),
    (17, 48, 160, 0, 3), (5, 48, 160, 16, 4), (64, 16, 1056, 0, 3), (65, 528, 1056, 0, 3), (1, 528, 1056, 0, 4),
    (17, 16, 1056, 5, 3), (64, 48, 1056, 3, 4), (16, 16, 1056, 1, 3), (65, 528, 160, 5, 3), (1, 48, 160, 5, 4),
    # wide layers, where a wave feeds 2 row tiles (from 256 tiles on) or 4 (from 1024 on, up to
    # 32 rows of x) from one x fragment
    (5, 8192, 160, 0, 3), (64, 8192, 160, 0, 4), (65, 8192, 128, 0, 3), (16, 4128, 160, 0, 3),
    (17, 4128, 1056, 0, 4), (1, 8192, 1056, 0, 3),
]


@pytest.mark.parametrize("m,n,k,split_k,first", EXACT)
def test_exact_on_integer_inputs(gpu, m, n, k, split_k, first):
    """64 KiB chunks with the parameter at block 3 (odd) or 4 (even) of a layer that goes on behind it."""
    off = 32 * first
    _exact(m, n, k, off + n * k + 64, 64 * KiB, off, 1000 * m + n + k, split_k=split_k)


@pytest.mark.parametrize("m,n,k,split_k,row_tiles", [(5, 64, 160, 0, 4), (17, 64, 1056, 3, 4), (32, 128, 96, 2, 4),
                                                      (64, 32, 160, 0, 2), (65, 96, 1056, 5, 2), (1, 32, 32, 0, 2),
                                                      (33, 64, 128, 0, 4)])
def test_exact_with_several_row_tiles_per_wave(gpu, m, n, k, split_k, row_tiles):
    """The wide-layer paths at small sizes: 2 or 4 row tiles per wave forced (beyond 32 rows of x,
    4 becomes 2), 1024-B chunks (16 blocks) so that the tiles of one wave lie in different chunks."""
    off, chunk = 32 * 7, 1024
    if k > 32:
        assert 16 * k >= chunk // 2  # tiles are 16 rows apart: a chunk or more
    _exact(m, n, k, off + n * k, chunk, off, m + n + k, split_k=split_k, row_tiles=row_tiles)


# (chunk bytes, element offset, elements behind the parameter)
LAYOUTS = {
    "rows straddle 1024-B chunks": (1024, 32 * 7, 32 * 5),
    "last rows in a short tail chunk of an odd block count": (1024, 32 * 7, 0),
    "tail chunk of a single block": (1024, 32 * 1, 0),
    "64 KiB chunk edge crossed mid-row": (64 * KiB, 32 * 1021, 32),
}


@pytest.mark.parametrize("m,n,k", [(5, 48, 96), (17, 528, 160), (16, 48, 1056)])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_exact_across_chunk_layouts(gpu, layout, m, n, k):
    """1024-B chunks hold 16 blocks (512 elements), the smallest the format allows: starting at
    element 224, chunk boundaries fall inside rows and inside 128-element steps. With nothing
    behind the parameter its last rows lie in the layer's tail chunk, of 7 blocks (its scale bytes
    are then 8-B and not 16-B aligned) or, starting at element 32, of one block. A 64 KiB chunk
    edge lies 96 elements into row 0: inside its first 128-element step where K > 96."""
    chunk, off, behind = LAYOUTS[layout]
    total = off + n * k + behind
    tail_blocks = total % (chunk // 2) // 32
    if layout == "last rows in a short tail chunk of an odd block count":
        assert tail_blocks % 2 == 1 and tail_blocks > 1
    if layout == "tail chunk of a single block":
        assert tail_blocks == 1
    if layout == "64 KiB chunk edge crossed mid-row" and k > 96:  # K = 96: row 0 ends at the edge
        assert off < 32 * KiB < off + min(k, 128)
    for split_k in (0, 2):
        _exact(m, n, k, total, chunk, off, 77 + k, split_k=split_k)


SHAPES = [(5, 48, 160), (64, 528, 1056), (17, 16, 1056), (1, 528, 128)]


@pytest.fixture(scope="module")
def random_case(gpu):
    """Per (m, n, k): x ~ N(0, 1) in bf16, W ~ N(0, 1/k) packed by ops.mxfp6_pack_layer (4 KiB
    chunks), the f32 output, and the float64 reference with its error bound."""
    out = {}
    g = torch.Generator().manual_seed(12)
    for m, n, k in SHAPES:
        x = torch.randn(m, k, generator=g).to(torch.bfloat16)
        w = (torch.randn(n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
        total = n * k
        packed = ops.mxfp6_pack_layer(w.view(-1).cuda(), 4096)
        wf = ref_weight(packed.cpu().numpy(), total, 4096, 0, n, k)  # exact in bf16 for every scale byte pack writes
        xf = bits_to_f64(bf16_tensor_bits(x)).reshape(m, k)
        y32 = _linear(x, packed, n, k, total, 4096, out_dtype=torch.float32)
        out[m, n, k] = dict(x=x, packed=packed, total=total, want=xf @ wf.T,
                            bound=k * 2.0 ** -23 * (np.abs(xf) @ np.abs(wf).T), y32=y32)
    return out


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_random_within_f32_accumulation_error(gpu, random_case, m, n, k):
    """bf16 x bf16 products are exact in f32 and each of the K additions errs by at most one
    unit roundoff of the running sum, itself at most sum |x w|: |y - y_ref| <= K 2^-23 sum_k
    |x_k w_k| per element (2^-23 allows truncating instead of nearest internal rounding)."""
    c = random_case[m, n, k]
    err = np.abs(c["y32"].cpu().numpy().astype(np.float64) - c["want"])
    print((m, n, k), "max err / bound", float((err / c["bound"]).max()))
    assert (err <= c["bound"]).all()


@pytest.mark.parametrize("m,n,k,split_k", [(5, 48, 160, 1), (64, 528, 1056, 4), (17, 16, 1056, 8)])
def test_bf16_output_is_the_rounded_f32_output(gpu, random_case, m, n, k, split_k):
    c = random_case[m, n, k]
    y32 = _linear(c["x"], c["packed"], n, k, c["total"], 4096, out_dtype=torch.float32, split_k=split_k)
    y16 = _linear(c["x"], c["packed"], n, k, c["total"], 4096, split_k=split_k)
    assert y16.dtype == torch.bfloat16
    assert np.array_equal(bf16_tensor_bits(y16), bf16_tensor_bits(y32.to(torch.bfloat16)))  # nearest even


@pytest.mark.parametrize("m,n,k", [(17, 16, 1056), (64, 528, 1056)])
def test_deterministic(gpu, random_case, m, n, k):
    """Equal bits from call to call, split-K reduction included."""
    c = random_case[m, n, k]
    assert gpu.mxfp6_linear_slices(m, n, k) > 1
    for _ in range(2):
        again = _linear(c["x"], c["packed"], n, k, c["total"], 4096, out_dtype=torch.float32)
        assert torch.equal(again.view(torch.int32), c["y32"].view(torch.int32))


def test_nan_blocks_poison_only_their_row(gpu):
    """Scale byte 0xFF (whatever the codes are): every output of that weight row is NaN for every
    row of x, zeros of x included; all other columns keep the bits of the clean run."""
    m, n, k, chunk, off = 17, 48, 160, 1024, 32 * 7
    total = off + n * k
    img = handmade_image(total, chunk, 9)
    x, xf = int_x(m, k, 3)
    assert (xf == 0).any()
    clean = _linear(x, img, n, k, total, chunk, off, out_dtype=torch.float32).cpu()
    clean16 = _linear(x, img, n, k, total, chunk, off).cpu()
    assert not torch.isnan(clean).any()
    # K = 160: blocks 0..3 of a row run in the main loop, block 4 in the K tail
    for r, b in [(21, 1), (47, 4), (0, 3)]:
        bad = img.copy()
        bad[block_index(total, chunk, off + r * k + 32 * b)[1]] = 0xFF
        keep = [c for c in range(n) if c != r]
        for split_k in (0, 2):
            y = _linear(x, bad, n, k, total, chunk, off, out_dtype=torch.float32, split_k=split_k).cpu()
            assert torch.isnan(y[:, r]).all()
            assert torch.equal(y[:, keep].view(torch.int32), clean[:, keep].view(torch.int32))
            y16 = _linear(x, bad, n, k, total, chunk, off, split_k=split_k).cpu()
            assert torch.isnan(y16[:, r]).all()
            assert torch.equal(y16[:, keep].view(torch.int16), clean16[:, keep].view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("split_k", [1, 4])
def test_writes_only_its_output(gpu, dtype, split_k):
    """M = 5 is padded to a 16-row tile by masking: with y a view into a 0xA5-filled buffer and a
    row stride larger than N, every byte outside y[:M, :N] is unchanged."""
    m, n, k, chunk = 5, 48, 1056, 4096
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


def test_rejects_bad_gpu_arguments(gpu):
    chunk = 4096
    total = 48 * 96
    p = torch.from_numpy(handmade_image(total, chunk, 1)).cuda()
    x = torch.zeros(5, 96, dtype=torch.bfloat16, device="cuda")
    y = torch.empty(5, 48, dtype=torch.float32, device="cuda")
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk)
    ops.mxfp6_linear(x, p, 48, 96, **kw)
    with pytest.raises(ValueError, match="same device"):
        ops.mxfp6_linear(x.cpu(), p, 48, 96, **kw)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.mxfp6_linear(x, torch.cat([p, p])[8: 8 + p.numel()], 48, 96, **kw)
    with pytest.raises(ValueError, match="out must be"):
        ops.mxfp6_linear(x, p, 48, 96, out=torch.empty(5, 32, device="cuda"), **kw)
    with pytest.raises(ValueError, match="outside"):
        ops.mxfp6_linear(x, p, 64, 96, **kw)
    # the launcher checks again on its own: (packed, src_bytes, src_chunk, elem_off, x, m, n, k, y, ldy, ...)
    gpu.mxfp6_linear(p.data_ptr(), 2 * total, chunk, 0, x.data_ptr(), 5, 48, 96, y.data_ptr(), 48, False, 0, 0, 0)
    for a in [dict(chunk=4096 + 256), dict(chunk=512), dict(chunk=0), dict(packed=p.data_ptr() + 8),
              dict(x=x.data_ptr() + 8), dict(y=y.data_ptr() + 2), dict(off=32), dict(off=16), dict(n=64), dict(n=40),
              dict(off=-32), dict(src=2 * total + 32), dict(src=0), dict(k=80), dict(ldy=32), dict(split_k=17),
              dict(row_tiles=3), dict(row_tiles=2)]:
        with pytest.raises(RuntimeError):
            gpu.mxfp6_linear(a.get("packed", p.data_ptr()), a.get("src", 2 * total), a.get("chunk", chunk),
                             a.get("off", 0), a.get("x", x.data_ptr()), 5, a.get("n", 48), a.get("k", 96),
                             a.get("y", y.data_ptr()), a.get("ldy", a.get("n", 48)), False, a.get("split_k", 0),
                             a.get("row_tiles", 0), 0)
    torch.cuda.synchronize()


def test_forward_from_the_packed_hbm_slot(gpu, monkeypatch):
    """rccl engine, `tiny`, 2 layers, 64 KiB chunks, --pack mxfp6 --store packed: the packed
    parameters alias the layer's HBM slot, no bf16 image exists, decoder_forward on the GPU makes
    5 mxfp6_linear calls per layer (q/k/v as one, o, gate, up, down) and agrees with the CPU pass
    on the dequantized parameters."""
    spec = PRESETS["tiny"]
    size = layer_nbytes(spec)
    blobs = {l: flatten(random_layer(spec, 7 + l), spec) for l in range(2)}
    cfg = make_workload(1, 2, size, tier="host", chunk_bytes=64 * KiB)
    rt = Runtime(cfg, 0, engine="rccl", chunk_bytes=64 * KiB, registry={0: "127.0.0.1:0"}, pack="mxfp6",
                 store="packed", layer_source=lambda l, n: blobs[l])
    calls = {"linear": 0}
    linear = ops.mxfp6_linear

    def count_linear(*a, **kw):
        calls["linear"] += 1
        return linear(*a, **kw)

    try:
        res = rt.run(1, timeout=60)
        assert res.ok, res.error
        x = torch.randn(1, 16, spec.hidden, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
        for l in range(2):
            p = rt.packed_layer_params(l, spec)
            assert rt.engine.unpacked_ptr(l) == 0  # no bf16 image
            for v in p.values():
                assert isinstance(v, PackedParam) and v.packed.is_cuda and (v.fmt, v.block) == ("mxfp6", 32)
                assert v.packed.data_ptr() == rt.engine.device_ptr(l) and v.packed.numel() == rt.slot_sizes[l]
            with monkeypatch.context() as mp:
                mp.setattr(ops, "mxfp6_linear", count_linear)
                calls["linear"] = 0
                y = decoder_forward(x.cuda(), p, spec).float().cpu()
                assert calls["linear"] == 5
            assert rt.engine.unpacked_ptr(l) == 0
            y0 = decoder_forward(x, {k: v.dequantize().cpu() for k, v in p.items()}, spec).float()
            rel = float((y - y0).norm() / y0.norm())
            print("layer", l, "relative error", rel)
            assert rel < 2e-2
    finally:
        rt.close()
