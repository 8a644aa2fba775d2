"""The gfx950 fused gated MLP (csrc/kernels/mxfp4_swiglu.hip, ops.mxfp4_swiglu): silu(x Wg^T) *
(x Wu^T) with both weights read in place from one MXFP4-packed layer, against the numpy reference
of test_mxfp4_linear_host.py (float64 matmuls on ref_weight, silu(g) * u in float64), and
decoder_forward's fused routes in a session whose layers stay packed in HBM.

On the integer inputs g and u are exact in f32 (see test_gpu_mxfp4_linear.py), so every error is
the epilogue's, y = (g / (1 + expf(-g))) * u in f32, and is bounded per element by the regime of g:

  g >= 18     1 + expf(-g) rounds to 1 (expf(-18) = 1.5e-8 < 2^-24): y == f32(g) * f32(u) exactly.
              exp(g) / (1 + exp(g)) instead is inf / inf = NaN from g = 89 on.
  g <= -104   expf(-g) is +inf: y == 0 (either sign), not NaN.
  otherwise   |y - ref| <= 4 2^-23 |ref| + 2^-100 max(1, |u|): expf within 1 ulp gives at most
              2^-23 (weighted by e / (1 + e) < 1), the add, the divide and the multiply 2^-24 each,
              2.5 2^-23 in all; the rest is room for a reciprocal-multiply. The absolute term only
              covers results in the f32-subnormal range, for g below about -87.
"""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import ops
from distributed_llm_dissemination_amd.models.catalog import make_workload
from distributed_llm_dissemination_amd.models.weights import (PRESETS, PackedParam, decoder_forward, flatten,
                                                             layer_nbytes, random_layer)
from distributed_llm_dissemination_amd.parallel.runtime import Runtime

from test_mxfp4_linear_host import (bf16_tensor_bits, bits_to_f64, handmade_image, int_x, ref_weight, scale_index)

pytestmark = pytest.mark.gpu

KiB = 1 << 10


def _swiglu(x, img, n, k, total, chunk, gate, up, **kw):
    p = img if torch.is_tensor(img) else torch.from_numpy(img).cuda()
    return ops.mxfp4_swiglu(x.cuda(), p, n, k, src_bytes=2 * total, chunk_bytes=chunk, gate_offset=gate, up_offset=up,
                            **kw)


def _linear(x, img, n, k, total, chunk, off, **kw):
    p = img if torch.is_tensor(img) else torch.from_numpy(img).cuda()
    return ops.mxfp4_linear(x.cuda(), p, n, k, src_bytes=2 * total, chunk_bytes=chunk, elem_offset=off, **kw)


def mixed_bound(ref, u):
    return 4 * 2.0 ** -23 * np.abs(ref) + 2.0 ** -100 * np.maximum(1.0, np.abs(u))


def silu_mul(g, u):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g)) * u


def regimes(g):
    hi, lo = g >= 18, g <= -104
    return hi, lo, ~(hi | lo)


def check_exact_regimes(y32, g, u):
    """The three checks of the module docstring for exact g and u (float64 arrays); returns the
    worst error / bound of the middle regime."""
    y = y32.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == g.shape
    hi, lo, mid = regimes(g)
    assert np.array_equal(y[hi], (g.astype(np.float32) * u.astype(np.float32))[hi])
    assert not np.isnan(y[lo]).any() and (y[lo] == 0).all()
    err, bound = np.abs(y.astype(np.float64) - silu_mul(g, u))[mid], mixed_bound(silu_mul(g, u), u)[mid]
    worst = float((err / bound).max()) if mid.any() else 0.0
    assert (err <= bound).all(), worst
    return worst


def exact_case(m, n, k, chunk, gate, up, total, seed):
    img = handmade_image(total, chunk, seed)
    x, xf = int_x(m, k, seed + 1)
    return img, x, xf @ ref_weight(img, total, chunk, gate, n, k).T, xf @ ref_weight(img, total, chunk, up, n, k).T


# M in {1, 5, 17, 64, 65} (a partial tile, the second and the fifth accumulator tile: 65 takes a
# second pass), N in {16, 48, 528}, K in {32, 96, 160, 1056} (the K tail alone, a main loop alone,
# both). split_k 0 is the launcher's choice; the others force K slices that leave waves without a
# step (K = 160: one step of 128, 15 of 16 waves empty and the last takes the tail; 8 steps over 5
# or 3 slices split unevenly). row_tiles counts pairs per wave: 2 is forced at N = 32 and 64 (where
# the gate and up tiles of one wave lie 2 and 4 tiles apart), and chosen at N = 8192; beyond 32
# rows of x it becomes 1.
EXACT = [
    (1, 16, 32, 0, 0), (5, 48, 96, 0, 0), (17, 48, 160, 16, 0), (64, 528, 1056, 0, 0), (64, 528, 32, 0, 1),
    (65, 528, 1056, 5, 0), (64, 16, 1056, 3, 0), (1, 528, 1056, 0, 0), (17, 528, 96, 0, 1), (65, 48, 160, 0, 1),
    (5, 16, 160, 16, 1), (17, 528, 1056, 3, 1), (64, 528, 160, 16, 0),
    (5, 32, 160, 0, 2), (17, 64, 1056, 5, 2), (32, 32, 1056, 3, 2), (64, 64, 96, 0, 2), (1, 64, 32, 0, 2),
    (5, 8192, 160, 0, 0),
]


@pytest.mark.parametrize("m,n,k,split_k,row_tiles", EXACT)
def test_exact_on_integer_inputs(gpu, m, n, k, split_k, row_tiles):
    """x: integers in [-8, 8]; W: random codes with scale bytes in {126, 127, 128}: g and u are
    exact multiples of 2^-2 in any summation order. 64 KiB chunks, gate at element 32 * 3, up
    behind it after a gap of 64 elements, the layer going on behind both."""
    chunk, gate = 64 * KiB, 32 * 3
    up = gate + n * k + 64
    total = up + n * k + 64
    img, x, g, u = exact_case(m, n, k, chunk, gate, up, total, 1000 * m + n + k)
    hi, lo, mid = regimes(g)
    if (m, n) == (64, 528):  # every regime is exercised, by the reference alone
        assert min(hi.mean(), lo.mean(), mid.mean()) >= 0.01, (hi.mean(), lo.mean(), mid.mean())
    y = _swiglu(x, img, n, k, total, chunk, gate, up, out_dtype=torch.float32, split_k=split_k, row_tiles=row_tiles)
    assert y.dtype == torch.float32 and y.shape == (m, n)
    print("regimes hi/lo/mid", int(hi.sum()), int(lo.sum()), int(mid.sum()), "worst err / bound",
          check_exact_regimes(y, g, u))


def test_equal_offsets(gpu):
    """gate and up may be the same parameter: y = silu(g) * g."""
    m, n, k, chunk, off = 17, 48, 160, 1024, 32 * 7
    total = off + n * k
    img, x, g, _ = exact_case(m, n, k, chunk, off, off, total, 13)
    check_exact_regimes(_swiglu(x, img, n, k, total, chunk, off, off, out_dtype=torch.float32), g, g)


# (chunk bytes, gate offset, up offset, elements behind the later parameter) for an [n, k] pair
LAYOUTS = {
    "up adjacent behind gate": lambda nk: (1024, 32 * 7, 32 * 7 + nk, 32 * 5),
    "up before gate with a gap": lambda nk: (1024, 32 * 7 + nk + 32 * 3, 32 * 7, 32 * 5),
    "last rows of up in a short tail chunk": lambda nk: (1024, 32 * 7, 32 * 7 + nk, 0),
    "64 KiB chunks crossed mid-row": lambda nk: (64 * KiB, 32 * 1021, 32 * 1021 + nk, 32),
}


@pytest.mark.parametrize("m,n,k", [(5, 48, 96), (17, 528, 160), (16, 48, 1056)])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_exact_across_chunk_layouts(gpu, layout, m, n, k):
    """1024-B chunks (512 elements) with the parameters from element 224 on: chunk edges fall
    inside rows and inside 128-element steps, and the gate and up tiles of one wave lie in
    different chunks."""
    chunk, gate, up, behind = LAYOUTS[layout](n * k)
    total = max(gate, up) + n * k + behind
    if layout == "last rows of up in a short tail chunk":
        assert 0 < total % (chunk // 2) < k * 4
    img, x, g, u = exact_case(m, n, k, chunk, gate, up, total, 77 + k)
    for split_k in (0, 2):
        check_exact_regimes(_swiglu(x, img, n, k, total, chunk, gate, up, out_dtype=torch.float32, split_k=split_k), g, u)


RANDOM = [(5, 48, 160, 1), (64, 528, 1056, 4), (1, 528, 128, 1), (64, 528, 1056, 8), (5, 48, 160, 16)]


@pytest.fixture(scope="module")
def random_case(gpu):
    """Per (m, n, k): x ~ N(0, 1) in bf16 and gate and up weights ~ N(0, 1/k), one behind the other
    in a layer packed by ops.mxfp4_pack_layer (4 KiB chunks), with the chosen-slices f32 and bf16
    results."""
    out = {}
    gen = torch.Generator().manual_seed(12)
    for m, n, k in sorted({c[:3] for c in RANDOM}):
        x = torch.randn(m, k, generator=gen).to(torch.bfloat16)
        w = (torch.randn(2 * n, k, generator=gen) / k ** 0.5).to(torch.bfloat16)
        total = 2 * n * k
        packed = ops.mxfp4_pack_layer(w.view(-1).cuda(), 4096)
        out[m, n, k] = dict(x=x, packed=packed, total=total,
                            y32=_swiglu(x, packed, n, k, total, 4096, 0, n * k, out_dtype=torch.float32),
                            y16=_swiglu(x, packed, n, k, total, 4096, 0, n * k))
    return out


@pytest.mark.parametrize("m,n,k,split_k", RANDOM)
def test_epilogue_on_the_linear_kernels_sums(gpu, random_case, m, n, k, split_k):
    """The K-partition contract: with the same forced split_k, g and u inside the kernel are the
    bits of two f32 mxfp4_linear calls, so against silu(g) * u of those (float64) only the
    epilogue's error is left, within the mixed bound of the module docstring."""
    c = random_case[m, n, k]
    a = (c["x"], c["packed"], n, k, c["total"], 4096)
    g = _linear(*a, 0, out_dtype=torch.float32, split_k=split_k).cpu().numpy().astype(np.float64)
    u = _linear(*a, n * k, out_dtype=torch.float32, split_k=split_k).cpu().numpy().astype(np.float64)
    y = _swiglu(*a, 0, n * k, out_dtype=torch.float32, split_k=split_k).cpu().numpy().astype(np.float64)
    ref = silu_mul(g, u)
    err, bound = np.abs(y - ref), mixed_bound(ref, u)
    print("worst err / bound", float((err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize("m,n,k", [(5, 48, 160), (64, 528, 1056)])
def test_bf16_output_is_the_rounded_f32_output(gpu, random_case, m, n, k):
    c = random_case[m, n, k]
    assert c["y16"].dtype == torch.bfloat16
    assert np.array_equal(bf16_tensor_bits(c["y16"]), bf16_tensor_bits(c["y32"].to(torch.bfloat16)))  # nearest even


def test_deterministic(gpu, random_case):
    """Equal bits from call to call, split-K reduction included."""
    m, n, k = 64, 528, 1056
    c = random_case[m, n, k]
    assert gpu.mxfp4_swiglu_slices(m, n, k) > 1
    for _ in range(3):
        again = _swiglu(c["x"], c["packed"], n, k, c["total"], 4096, 0, n * k, out_dtype=torch.float32)
        assert torch.equal(again.view(torch.int32), c["y32"].view(torch.int32))


def test_nan_block_poisons_only_its_column(gpu):
    """A 0xFF scale byte in row r of either weight: y[:, r] is NaN, every other column keeps its bits."""
    m, n, k, chunk, gate = 17, 48, 160, 1024, 32 * 7
    up = gate + n * k
    total = up + n * k
    img = handmade_image(total, chunk, 9)
    x, _ = int_x(m, k, 3)
    clean = _swiglu(x, img, n, k, total, chunk, gate, up, out_dtype=torch.float32).cpu()
    assert not torch.isnan(clean).any()
    for off in (gate, up):
        for r, blk in [(21, 0), (47, 4), (0, 3)]:  # blocks of the main loop and of the K tail
            bad = img.copy()
            bad[scale_index(total, chunk, off + r * k + 32 * blk)] = 0xFF
            y = _swiglu(x, bad, n, k, total, chunk, gate, up, out_dtype=torch.float32).cpu()
            assert torch.isnan(y[:, r]).all()
            keep = [c for c in range(n) if c != r]
            assert torch.equal(y[:, keep].view(torch.int32), clean[:, keep].view(torch.int32))
            y16 = _swiglu(x, bad, n, k, total, chunk, gate, up).cpu()
            assert torch.isnan(y16[:, r]).all() and not torch.isnan(y16[:, keep]).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("split_k", [1, 4])
def test_writes_only_its_output(gpu, dtype, split_k):
    """M = 5 is padded to a 16-row tile by masking: with y a view into a 0xA5-filled buffer and a
    row stride larger than N, every byte outside y[:M, :N] is unchanged."""
    m, n, k, chunk = 5, 48, 1056, 1024
    total = 2 * n * k
    img, x, g, u = exact_case(m, n, k, chunk, 0, n * k, total, 31)
    es = 2 if dtype == torch.bfloat16 else 4
    ld, lead = 80, 3 * 80 + 8
    buf = torch.full(((lead + (m + 3) * ld) * es,), 0xA5, dtype=torch.uint8, device="cuda")
    y = buf.view(dtype)[lead: lead + m * ld].view(m, ld)[:, :n]
    got = _swiglu(x, img, n, k, total, chunk, 0, n * k, out=y, split_k=split_k)
    assert got.data_ptr() == y.data_ptr()
    y32 = _swiglu(x, img, n, k, total, chunk, 0, n * k, out_dtype=torch.float32, split_k=split_k)
    check_exact_regimes(y32, g, u)
    assert np.array_equal(y.cpu().contiguous().view(torch.uint8).numpy(), y32.to(dtype).cpu().view(torch.uint8).numpy())
    mask = torch.ones(buf.numel() // es, dtype=torch.bool)
    mask[lead: lead + m * ld].view(m, ld)[:, :n] = False
    outside = buf.cpu().view(-1, es)[mask]
    assert outside.numel() and bool((outside == 0xA5).all())


def test_rejects_bad_gpu_arguments(gpu):
    n, k, chunk = 48, 96, 1024
    total = 2 * n * k
    p = torch.from_numpy(handmade_image(total, chunk, 1)).cuda()
    x = torch.zeros(5, k, dtype=torch.bfloat16, device="cuda")
    y = torch.empty(5, n, dtype=torch.float32, device="cuda")
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk, gate_offset=0, up_offset=n * k)
    ops.mxfp4_swiglu(x, p, n, k, **kw)
    with pytest.raises(ValueError, match="same device"):
        ops.mxfp4_swiglu(x.cpu(), p, n, k, **kw)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.mxfp4_swiglu(x, torch.cat([p, p])[1: 1 + p.numel()], n, k, **kw)
    with pytest.raises(ValueError, match="out must be"):
        ops.mxfp4_swiglu(x, p, n, k, out=torch.empty(5, 32, device="cuda"), **kw)
    with pytest.raises(ValueError, match="outside"):
        ops.mxfp4_swiglu(x, p, n, k, **{**kw, "up_offset": n * k + 32})

    def launch(gate, up, row_tiles=0):  # the launcher checks again on its own
        gpu.mxfp4_swiglu(p.data_ptr(), 2 * total, chunk, gate, up, x.data_ptr(), 5, n, k, y.data_ptr(), n, False, 0,
                         row_tiles, 0)

    launch(0, n * k)
    for args in [(16, n * k), (0, n * k + 16), (n * k + 32, 0), (0, n * k + 32), (-32, 0), (0, n * k, 3), (0, n * k, 2)]:
        with pytest.raises(RuntimeError):
            launch(*args)


def test_fused_forward_from_the_packed_hbm_slot(gpu, monkeypatch):
    """rccl engine, `tiny`, 2 layers, 64 KiB chunks, --pack mxfp4 --store packed: decoder_forward
    on the packed slot makes 4 weight launches (q/k/v as one mxfp4_linear, o, swiglu, down), the
    merged q/k/v is as accurate as three calls, and the fused pass is no further from the float32
    pass on the dequantized weights than the unfused one (it rounds strictly less often; 10 % for
    the other summation order of the merged q/k/v)."""
    spec = PRESETS["tiny"]
    size = layer_nbytes(spec)
    blobs = {l: flatten(random_layer(spec, 7 + l), spec) for l in range(2)}
    cfg = make_workload(1, 2, size, tier="host", chunk_bytes=64 * KiB)
    rt = Runtime(cfg, 0, engine="rccl", chunk_bytes=64 * KiB, registry={0: "127.0.0.1:0"}, pack="mxfp4",
                 store="packed", layer_source=lambda l, n: blobs[l])
    calls = {"linear": 0, "swiglu": 0}
    linear, swiglu = ops.mxfp4_linear, ops.mxfp4_swiglu

    def count_linear(*a, **kw):
        calls["linear"] += 1
        return linear(*a, **kw)

    def count_swiglu(*a, **kw):
        calls["swiglu"] += 1
        return swiglu(*a, **kw)

    try:
        res = rt.run(1, timeout=60)
        assert res.ok, res.error
        x = torch.randn(1, 16, spec.hidden, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
        for l in range(2):
            p = rt.layer_params(l, spec, packed=True)
            assert all(isinstance(v, PackedParam) and v.packed.is_cuda for v in p.values())
            # q, k and v as one [h + 2 kv, h] weight against three calls, both against float64
            wq, wk, wv = p["q_proj"], p["k_proj"], p["v_proj"]
            nq, nk, kk = wq.shape[0], wk.shape[0], wq.shape[1]
            h = x[0].cuda()
            kw = dict(src_bytes=wq.src_bytes, chunk_bytes=wq.chunk_bytes, out_dtype=torch.float32)
            one = ops.mxfp4_linear(h, wq.packed, nq + 2 * nk, kk, elem_offset=wq.elem_offset, **kw).cpu().numpy()
            three = np.concatenate([ops.mxfp4_linear(h, w.packed, w.shape[0], kk, elem_offset=w.elem_offset, **kw)
                                    .cpu().numpy() for w in (wq, wk, wv)], axis=1)
            wf = np.concatenate([bits_to_f64(bf16_tensor_bits(w.dequantize())).reshape(w.shape) for w in (wq, wk, wv)])
            xf = bits_to_f64(bf16_tensor_bits(x[0])).reshape(16, kk)
            want, bound = xf @ wf.T, kk * 2.0 ** -23 * (np.abs(xf) @ np.abs(wf).T)
            assert (np.abs(one.astype(np.float64) - want) <= bound).all()
            assert (np.abs(three.astype(np.float64) - want) <= bound).all()
            # the passes
            with monkeypatch.context() as mp:
                mp.setattr(ops, "mxfp4_linear", count_linear)
                mp.setattr(ops, "mxfp4_swiglu", count_swiglu)
                calls.update(linear=0, swiglu=0)
                y = decoder_forward(x.cuda(), p, spec, fuse=True).float().cpu()
                assert calls == {"linear": 3, "swiglu": 1}
                calls.update(linear=0, swiglu=0)
                y1 = decoder_forward(x.cuda(), p, spec, fuse=False).float().cpu()
                assert calls == {"linear": 7, "swiglu": 0}
            y0 = decoder_forward(x.float(), {k: v.dequantize().cpu().float() for k, v in p.items()}, spec)
            rel, rel1 = float((y - y0).norm() / y0.norm()), float((y1 - y0).norm() / y0.norm())
            print("layer", l, "relative error fused", rel, "unfused", rel1)
            assert rel <= 1.1 * rel1
    finally:
        rt.close()
