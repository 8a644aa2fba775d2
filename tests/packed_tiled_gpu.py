"""Test bodies shared by test_gpu_mxfp6_tiled.py and test_gpu_fp8_tiled.py: the many-row kernels of
the MXFP6 and fp8 formats (csrc/kernels/mxfp6_tiled.hip, fp8_tiled.hip; ops.*_linear and
ops.*_swiglu with tiled=True), case for case what test_gpu_mxfp4_tiled.py asks of the MXFP4 pair, on
each format's own numpy reference through the `Fmt` of packed_swiglu_gpu.py. A plain module; BM and
BN come from the bindings, so the cases follow the kernels.

Two contracts are tested here and nowhere else. Batch invariance: y[m][n] depends only on row m of
x and row n of W - one row alone, a prefix of the rows, a window of the weight rows and the parts of
a merged q/k/v launch all carry the bits of the full call. Agreement with the decode kernel: the
tiled f32 result is the untiled op's with split_k=1, bit for bit (one accumulator per element that
takes the same products in the same order, MXFP6's masked tail groups included).

Every tolerance is an existing derived bound: equality on integer inputs (Fmt.prove_exact_ints),
K 2^-23 sum |x w| on random ones (test_gpu_mxfp6_linear.py), the epilogue's three regimes and
mixed_bound (test_gpu_mxfp4_swiglu.py), check A of decoder_packed_reference.py."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.weights import decoder_forward

import decoder_packed_reference as dp
import test_mxfp6_linear_host as m6
from packed_swiglu_gpu import Fmt, exact_case
from test_gpu_mxfp4_swiglu import check_exact_regimes, mixed_bound, silu_mul

KiB = 1 << 10


def tile(f):
    return _core.fp8_tiled_tile() if f.name == "fp8" else _core.mxfp6_tiled_tile()


def linear(f, x, img, n, k, total, chunk, off=0, **kw):
    return f.linear(x, img, n, k, total, chunk, off, tiled=True, **kw)


def swiglu(f, x, img, n, k, total, chunk, gate, up, **kw):
    return f.swiglu(x, img, n, k, total, chunk, gate, up, tiled=True, **kw)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def ref_weight(f, img, total, chunk, off, n, k):
    return f.layer_f64(img, total, chunk)[off: off + n * k].reshape(n, k)


def exact_list(bm, bn):
    """M in {1, 17, BM - 1, BM, BM + 1, 2 BM + 5} (a partial first tile, the last row of a tile, a
    second tile of one row, a third of five), N in {16, 48, BN + 16, 528} (one wave's tile, three
    waves, a second workgroup of one tile, several), K in {32, 96, 128, 160, 1056} (the K tail
    alone, one step alone, a step and a tail, eight steps and a tail); every value appears, and one
    wide layer."""
    return [
        (1, 16, 32), (1, 48, 1056), (1, 528, 128), (1, bn + 16, 160), (17, 16, 96), (17, 48, 128), (17, 528, 160),
        (17, bn + 16, 1056), (bm - 1, 16, 160), (bm - 1, 48, 32), (bm - 1, bn + 16, 128), (bm - 1, 528, 96),
        (bm, 16, 1056), (bm, 48, 96), (bm, bn + 16, 32), (bm, 528, 160), (bm + 1, 16, 128), (bm + 1, 48, 160),
        (bm + 1, bn + 16, 96), (bm + 1, 528, 1056), (2 * bm + 5, 16, 32), (2 * bm + 5, bn + 16, 160),
        (2 * bm + 5, 528, 128), (17, 4128, 96),
    ]


def exact_on_integer_inputs(f, m, n, k, off):
    """64 KiB chunks, the parameter at element `off` of a layer that goes on 64 elements behind it
    (padded to whole scale blocks). Fmt.prove_exact_ints shows on the reference that every partial
    sum, in any order, is exact in f32: the f32 output equals the float64 matmul."""
    chunk = 64 * KiB
    total = f.padded(off + n * k + 64)
    img = f.image(total, chunk, 1000 * m + n + k)
    x, xf = m6.int_x(m, k, m + 7 * k)
    wf = ref_weight(f, img, total, chunk, off, n, k)
    f.prove_exact_ints(xf, wf)
    y = linear(f, x, img, n, k, total, chunk, off, out_dtype=torch.float32)
    assert y.dtype == torch.float32 and y.shape == (m, n)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), xf @ wf.T)


def exact_across_chunk_layouts(f, chunk, off, behind, m, n, k, image_is_all):
    """`image_is_all`: a tail-chunk layout, in which the packed tensor is exactly the image, with
    nothing behind the last block read."""
    total = f.padded(off + n * k + behind)
    img = f.image(total, chunk, 77 + k)
    x, xf = m6.int_x(m, k, 5 + m)
    wf = ref_weight(f, img, total, chunk, off, n, k)
    f.prove_exact_ints(xf, wf)
    p = torch.from_numpy(img).cuda()
    if image_is_all:
        assert behind == 0 and 0 < total % (chunk // 2) and p.numel() == img.size
    y = linear(f, x, p, n, k, total, chunk, off, out_dtype=torch.float32)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), xf @ wf.T)


def random_shapes(bm):
    return [(5, 48, 160), (bm + 1, 528, 1056), (2 * bm + 5, 528, 1056)]


def random_case(f):
    """Per (m, n, k): x ~ N(0, 1) in bf16 and two [n, k] weights ~ N(0, 1/k), one behind the other
    in a layer packed by ops.*_pack_layer (4 KiB chunks); the tiled f32 and bf16 results for the
    first weight, and the float64 reference with its error bound. Computed once per format and
    left unchanged."""
    out = {}
    g = torch.Generator().manual_seed(12)
    for m, n, k in random_shapes(tile(f)[0]):
        x = torch.randn(m, k, generator=g).to(torch.bfloat16)
        w = (torch.randn(2 * n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
        total = 2 * n * k
        assert total % f.block == 0
        packed = f.pack_layer(w.view(-1).cuda(), 4096)
        wf = ref_weight(f, packed.cpu().numpy(), total, 4096, 0, n, k)
        xf = m6.bits_to_f64(m6.bf16_tensor_bits(x)).reshape(m, k)
        out[m, n, k] = dict(x=x, packed=packed, total=total, want=xf @ wf.T,
                            bound=k * 2.0 ** -23 * (np.abs(xf) @ np.abs(wf).T),
                            y32=linear(f, x, packed, n, k, total, 4096, out_dtype=torch.float32),
                            y16=linear(f, x, packed, n, k, total, 4096))
    return out


def random_within_f32_accumulation_error(f, c):
    """|y - y_ref| <= K 2^-23 sum_k |x_k w_k| per element, as test_gpu_mxfp6_linear.py derives it;
    the bf16 output is the f32 output rounded to nearest even, bit for bit."""
    err = np.abs(c["y32"].cpu().numpy().astype(np.float64) - c["want"])
    print(f.id, "max err / bound", float((err / c["bound"]).max()))
    assert (err <= c["bound"]).all()
    assert c["y16"].dtype == torch.bfloat16
    assert np.array_equal(m6.bf16_tensor_bits(c["y16"]), m6.bf16_tensor_bits(c["y32"].to(torch.bfloat16)))


def inv(f, cases):
    m, n, k = random_shapes(tile(f)[0])[2]
    return m, n, k, cases[m, n, k]


def one_row_alone_gives_the_bits_of_the_full_call(f, cases):
    bm = tile(f)[0]
    m, n, k, c = inv(f, cases)
    for r in (0, 15, 16, bm - 1, bm, 2 * bm + 4):
        alone = linear(f, c["x"][r: r + 1], c["packed"], n, k, c["total"], 4096, out_dtype=torch.float32)
        assert same_bits(alone, c["y32"][r: r + 1]), r
    head = linear(f, c["x"][: bm + 1], c["packed"], n, k, c["total"], 4096, out_dtype=torch.float32)
    assert same_bits(head, c["y32"][: bm + 1])


def a_window_of_weight_rows_gives_its_columns(f, cases):
    """Rows [BN - 16, BN + 32) of W as a parameter of their own (N = 48, the offset moved by
    (BN - 16) K): other waves, another workgroup, the same bits."""
    bn = tile(f)[1]
    m, n, k, c = inv(f, cases)
    part = linear(f, c["x"], c["packed"], 48, k, c["total"], 4096, off=(bn - 16) * k, out_dtype=torch.float32)
    assert same_bits(part, c["y32"][:, bn - 16: bn + 32])


def merged_qkv_equals_three_calls(f, cases):
    m, n, k, c = inv(f, cases)
    col = 0
    for rows in (256, 144, 128):
        alone = linear(f, c["x"], c["packed"], rows, k, c["total"], 4096, off=col * k, out_dtype=torch.float32)
        assert same_bits(alone, c["y32"][:, col: col + rows]), col
        col += rows
    assert col == n


def deterministic(f, cases):
    m, n, k, c = inv(f, cases)
    for _ in range(3):
        assert same_bits(linear(f, c["x"], c["packed"], n, k, c["total"], 4096, out_dtype=torch.float32), c["y32"])


def agrees_with_the_decode_kernel(f, cases):
    """One accumulator per element and the decode kernel's K order: the tiled f32 results are the
    untiled op's with split_k=1 bit for bit, for the linear and for the gated pair. A difference
    means a K order or a tail form that is not the decode kernel's."""
    m, n, k, c = inv(f, cases)
    a = (c["x"], c["packed"], n, k, c["total"], 4096)
    assert same_bits(f.linear(*a, 0, out_dtype=torch.float32, split_k=1), c["y32"])
    for gate, up in ((0, n * k), (n * k, 0)):
        assert same_bits(f.swiglu(*a, gate, up, out_dtype=torch.float32, split_k=1),
                         swiglu(f, *a, gate, up, out_dtype=torch.float32))


# ---------------------------------------------------------------- gated

def gated_list(bm, bn):
    """(m, n, k, layout): "up first" has gate_off > up_off, "equal" one parameter for both."""
    return [(1, 16, 160, "gate first"), (1, bn + 16, 1056, "up first"), (bm + 1, 16, 1056, "up first"),
            (bm + 1, bn + 16, 160, "gate first"), (bm + 1, bn + 16, 96, "equal"), (1, 16, 32, "equal"),
            (bm + 1, 528, 128, "up first")]


def gated_exact_on_integer_inputs(f, m, n, k, layout):
    """g and u are exact in f32 on these inputs, so the result is held to the epilogue's three
    regimes of test_gpu_mxfp4_swiglu.py (g * u exactly from g = 18 on, 0 below -104, the mixed
    bound between). 64 KiB chunks, the parameters 64 elements apart."""
    chunk, first = 64 * KiB, 32 * 3
    second = first + n * k + 64
    gate, up = {"gate first": (first, second), "up first": (second, first), "equal": (first, first)}[layout]
    total = f.padded(second + n * k + 64)
    img, x, g, u = exact_case(f, m, n, k, chunk, gate, up, total, 1000 * m + n + k)
    y = swiglu(f, x, img, n, k, total, chunk, gate, up, out_dtype=torch.float32)
    print(f.id, "worst err / bound", check_exact_regimes(y, g, u))
    # and g, u themselves: the tiled linear on the same rows is exact
    for off, want in ((gate, g), (up, u)):
        got = linear(f, x, img, n, k, total, chunk, off, out_dtype=torch.float32)
        assert np.array_equal(got.cpu().numpy().astype(np.float64), want)


def gated_epilogue_on_the_tiled_linears_sums(f, c, m, n, k, up_first):
    """g and u inside the gated kernel are the bits of two tiled f32 linears (one K order), so
    against silu(g) * u of those in float64 only the epilogue's error is left."""
    a = (c["x"], c["packed"], n, k, c["total"], 4096)
    gate, up = (n * k, 0) if up_first else (0, n * k)
    g = linear(f, *a, gate, out_dtype=torch.float32).cpu().numpy().astype(np.float64)
    u = linear(f, *a, up, out_dtype=torch.float32).cpu().numpy().astype(np.float64)
    y32 = swiglu(f, *a, gate, up, out_dtype=torch.float32)
    ref = silu_mul(g, u)
    err, bound = np.abs(y32.cpu().numpy().astype(np.float64) - ref), mixed_bound(ref, u)
    print(f.id, "worst err / bound", float((err / bound).max()))
    assert (err <= bound).all()
    y16 = swiglu(f, *a, gate, up)
    assert np.array_equal(m6.bf16_tensor_bits(y16), m6.bf16_tensor_bits(y32.to(torch.bfloat16)))
    assert same_bits(swiglu(f, *a, gate, up, out_dtype=torch.float32), y32)


# ---------------------------------------------------------------- special values

def nan_weight_poisons_only_its_column(f):
    m, n, k, chunk, gate = 17, 48, 160, 1024, 32 * 7
    up = gate + n * k
    total = f.padded(up + n * k)
    img = f.image(total, chunk, 9)
    x, _ = m6.int_x(m, k, 3)
    clean = linear(f, x, img, n, k, total, chunk, gate, out_dtype=torch.float32).cpu()
    clean_up = linear(f, x, img, n, k, total, chunk, up, out_dtype=torch.float32).cpu()
    clean_glu = swiglu(f, x, img, n, k, total, chunk, gate, up, out_dtype=torch.float32).cpu()
    assert not torch.isnan(clean).any() and not torch.isnan(clean_up).any() and not torch.isnan(clean_glu).any()
    for r, blk in [(21, 0), (47, 4), (0, 3)]:  # blocks of the main loop and of the K tail
        keep = [c for c in range(n) if c != r]
        for off in (gate, up):
            bad = img.copy()
            f.poison(bad, total, chunk, off + r * k + 32 * blk + 5)
            y = swiglu(f, x, bad, n, k, total, chunk, gate, up, out_dtype=torch.float32).cpu()
            assert torch.isnan(y[:, r]).all()
            assert same_bits(y[:, keep], clean_glu[:, keep])
        y = linear(f, x, bad, n, k, total, chunk, gate, out_dtype=torch.float32).cpu()  # `bad` is in up: clean
        assert same_bits(y, clean)
        y = linear(f, x, bad, n, k, total, chunk, up, out_dtype=torch.float32).cpu()
        assert torch.isnan(y[:, r]).all() and same_bits(y[:, keep], clean_up[:, keep])
        y16 = linear(f, x, bad, n, k, total, chunk, up).cpu()
        assert torch.isnan(y16[:, r]).all() and not torch.isnan(y16[:, keep]).any()


def non_finite_rows_of_x_as_the_untiled_op(f):
    bm = tile(f)[0]
    m, n, k, chunk = bm + 1, 48, 160, 1024
    total = n * k
    assert total % f.block == 0
    img = f.image(total, chunk, 21)
    x, _ = m6.int_x(m, k, 22)
    x[3, 7], x[5, 130], x[bm, 40] = float("inf"), float("-inf"), float("nan")
    x[20, 1], x[20, 150] = float("inf"), float("-inf")
    p = torch.from_numpy(img).cuda()
    y = linear(f, x, p, n, k, total, chunk, out_dtype=torch.float32).cpu()
    y0 = f.linear(x, p, n, k, total, chunk, 0, out_dtype=torch.float32).cpu()
    assert torch.equal(torch.isnan(y), torch.isnan(y0))
    assert torch.isnan(y[bm]).all() and torch.isinf(y[3]).any() and not torch.isnan(y[[0, 4, bm - 1]]).any()
    fin = ~torch.isnan(y)
    assert torch.equal(y[fin], y0[fin])  # +-inf and the exact sums of the other rows


# ---------------------------------------------------------------- addressing

def writes_only_its_output(f, dtype, gated):
    """M = BM + 1 leaves 15 rows of the second tile and N = 48 a wave and most of the column tile
    unused: with y a view into a 0xA5-filled buffer and a row stride larger than N, every byte
    outside y[:M, :N] is unchanged. x holds exactly M K elements."""
    m, n, k, chunk = tile(f)[0] + 1, 48, 160, 1024
    total = 2 * n * k
    assert total % f.block == 0
    img, x, g, u = exact_case(f, m, n, k, chunk, 0, n * k, total, 31)
    assert x.numel() == m * k
    es = 2 if dtype == torch.bfloat16 else 4
    ld, lead = 80, 3 * 80 + 8
    buf = torch.full(((lead + (m + 3) * ld) * es,), 0xA5, dtype=torch.uint8, device="cuda")
    y = buf.view(dtype)[lead: lead + m * ld].view(m, ld)[:, :n]
    if gated:
        got = swiglu(f, x, img, n, k, total, chunk, 0, n * k, out=y)
        want = swiglu(f, x, img, n, k, total, chunk, 0, n * k, out_dtype=torch.float32).to(dtype)
    else:
        got = linear(f, x, img, n, k, total, chunk, 0, out=y)
        want = torch.from_numpy(g).to(dtype).cuda()
    assert got.data_ptr() == y.data_ptr()
    assert same_bits(y.contiguous(), want)
    mask = torch.ones(buf.numel() // es, dtype=torch.bool)
    mask[lead: lead + m * ld].view(m, ld)[:, :n] = False
    outside = buf.cpu().view(-1, es)[mask]
    assert outside.numel() and bool((outside == 0xA5).all())


def rejects_bad_gpu_arguments(f):
    n, k, chunk = 64, 96, 1024
    total = 2 * n * k
    assert total % f.block == 0
    p = torch.from_numpy(f.image(total, chunk, 1)).cuda()
    x = torch.zeros(5, k, dtype=torch.bfloat16, device="cuda")
    y = torch.empty(5, n, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="split_k"):
        linear(f, x, p, n, k, total, chunk, split_k=2)
    with pytest.raises(ValueError, match="row_tiles"):
        swiglu(f, x, p, n, k, total, chunk, 0, n * k, row_tiles=2)
    with pytest.raises(ValueError, match="outside"):
        linear(f, x, p, n, k, total, chunk, off=n * k + 32)
    blk = (f.block,) if f.name == "fp8" else ()
    lin_t, glu_t = getattr(_core, f.name + "_linear_tiled"), getattr(_core, f.name + "_swiglu_tiled")
    lin_t(p.data_ptr(), 2 * total, chunk, *blk, 32, x.data_ptr(), 5, n, k, y.data_ptr(), n, False, 0)
    with pytest.raises(RuntimeError):  # the launcher checks again on its own
        lin_t(p.data_ptr(), 2 * total, chunk, *blk, 16, x.data_ptr(), 5, n, k, y.data_ptr(), n, False, 0)
    with pytest.raises(RuntimeError):
        glu_t(p.data_ptr(), 2 * total, chunk, *blk, 0, n * k + 16, x.data_ptr(), 5, n, k, y.data_ptr(), n, False, 0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the decoder layer

def decoder_forward_tiled(monkeypatch, spec_name, fmt_name):
    """BM + 1 rows as batch x seq through decoder_forward(fuse_gated=True, tiled=True): within check
    A's tolerance of the float64 reference (decoder_packed_reference.py; the tolerance comes from the
    bf16 floor, the CPU pass and plain torch on the GPU, nothing from a packed route), in 4 weight
    launches, all of them the tiled kernels'; without fuse_gated 5 tiled linears and no untiled one."""
    fmt, block, _ = dp.FORMATS[fmt_name]
    bm = tile(Fmt(fmt, block))[0]
    rows = next((b, (bm + 1) // b) for b in (3, 1) if (bm + 1) % b == 0)
    c = dp.case(spec_name, rows, fmt_name)
    assert c.batch * c.seq == bm + 1
    params = c.layer.packed_params("cuda")
    x = c.xt.cuda()
    ctl = decoder_forward(x, {k: v.cuda() for k, v in c.layer.dense.items()}, c.spec).float().cpu().numpy()
    calls = []
    lin, glu = fmt + "_linear", fmt + "_swiglu"
    for name in (lin, glu, lin + "_tiled", glu + "_tiled"):
        def counted(*a, _fn=getattr(_core, name), _name=name, **kw):
            calls.append(_name)
            return _fn(*a, **kw)
        monkeypatch.setattr(_core, name, counted)
    y = decoder_forward(x, params, c.spec, fuse_gated=True, tiled=True)
    torch.cuda.synchronize()
    assert calls == [lin + "_tiled", lin + "_tiled", glu + "_tiled", lin + "_tiled"]
    dp.check_a(c, y, "gpu fuse_gated tiled", dp.rel(ctl, c.y64), dp.row_rel(ctl, c.y64))
    del calls[:]
    y = decoder_forward(x, params, c.spec, tiled=True)
    torch.cuda.synchronize()
    assert calls == [lin + "_tiled"] * 5
    dp.check_a(c, y, "gpu tiled", dp.rel(ctl, c.y64), dp.row_rel(ctl, c.y64))
