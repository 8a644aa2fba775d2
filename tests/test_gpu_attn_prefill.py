"""ops.attn_prefill, ops.rope_append_seq (csrc/kernels/attn_prefill.hip) and decoder_forward(attn="mfma",
extend=) on the GPU. test_attn_prefill_host.py states the cases, the float64 reference, the bound and the
condition that makes the bound see a lost position.

1. Against float64, every case, f32 and bf16: within the bound, the bf16 result the f32 result rounded, no
   NaN; with T cut short the rows at positions >= T are zero and the others keep their bits.
   Measured on an MI355X: err / bound at most 0.41 in f32 and 0.56 in bf16 (the bound is not tightened to
   that); decoder_forward(attn="mfma") rows at most 0.56 of their tolerance.
2. Bit for bit, f32: a sequence alone; one pass against BK - 3 rows and then the rest with start advanced; T
   doubled with other garbage; K / V as strided slices of a merged-projection buffer; causality at j0.
3. rope_append_seq against `_rope` on the GPU, bit for bit, and nothing else of the caches touched.
4. decoder_forward(attn="mfma"), extend and a decoder_step behind it against the float64 ref_decoder.
5. Errors: ValueError before any launch.
6. A row of exactly one 32-position step has ops.attn_decode's bits (both take the step from attn_mma.h)."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import ops
from distributed_llm_dissemination_amd.ops.kernels import _kv_view

import test_attn_prefill_host as host
from attn_decode_cases import garbage
from test_attn_decode_host import ROPE_SHAPES
from test_decoder_reference import SPECS

pytestmark = pytest.mark.gpu
BQ, BK = host.BQ, host.BK


@pytest.fixture(scope="module", params=host.CASES, ids=host.case_id)
def batch(request, gpu):
    """Per case: the batch in HBM and its f32 result."""
    c = host.case(*request.param)
    q, k, v, start = (c[n].cuda() for n in ("q", "k", "v", "start"))
    y32 = ops.attn_prefill(q, k, v, start, out_dtype=torch.float32)
    torch.cuda.synchronize()
    return dict(c=c, s=request.param[2], q=q, k=k, v=v, start=start, y32=y32)


def same_bits(a, b):
    return np.array_equal(a.contiguous().view(torch.int32).cpu().numpy(), b.contiguous().view(torch.int32).cpu().numpy())


def test_attn_prefill_matches_float64(batch):
    c, y32 = batch["c"], batch["y32"]
    y16 = ops.attn_prefill(batch["q"], batch["k"], batch["v"], batch["start"])
    assert y32.dtype == torch.float32 and y16.dtype == torch.bfloat16 and tuple(y32.shape) == tuple(y16.shape) == c["y64"].shape
    w32, w16 = host.err_over_bound(y32, c, False), host.err_over_bound(y16, c, True)
    print(c["id"], "err / bound: f32", w32, "bf16", w16)
    assert w32 <= 1 and w16 <= 1
    assert torch.equal(y16, y32.to(torch.bfloat16))
    cut = BK + 5 + batch["s"] - 2  # T cut short: sequence 3's last two rows have no position
    yc = ops.attn_prefill(batch["q"], batch["k"][:, :, :cut], batch["v"][:, :, :cut], batch["start"], out_dtype=torch.float32)
    assert not yc[3, -2:].any() and same_bits(yc[:3], y32[:3]) and same_bits(yc[3, :-2], y32[3, :-2])


def test_alone_split_and_doubled_t_change_no_bit(batch):
    q, k, v, start, y32, s = (batch[n] for n in ("q", "k", "v", "start", "y32", "s"))
    for b in range(4):  # alone, in a cache of its own
        ya = ops.attn_prefill(q[b: b + 1], k[b: b + 1].clone(), v[b: b + 1].clone(), start[b: b + 1].clone(), out_dtype=torch.float32)
        assert same_bits(ya[0], y32[b]), b
    cut = min(BK - 3, s)  # the first BK - 3 rows, then the rest behind them
    parts = [ops.attn_prefill(q[:, :cut], k, v, start, out_dtype=torch.float32)]
    if cut < s:
        parts.append(ops.attn_prefill(q[:, cut:], k, v, start + cut, out_dtype=torch.float32))
    assert same_bits(torch.cat(parts, 1), y32)
    t_len = k.shape[2]
    k2, v2 = garbage((4, host.KVH, 2 * t_len, k.shape[3]), 41).cuda(), garbage((4, host.KVH, 2 * t_len, k.shape[3]), 42).cuda()
    for b, st in enumerate(host.STARTS):
        k2[b, :, : st + s], v2[b, :, : st + s] = k[b, :, : st + s], v[b, :, : st + s]
    assert same_bits(ops.attn_prefill(q, k2, v2, start, out_dtype=torch.float32), y32)


def test_merged_projection_slices_and_causality(batch):
    q, k, v, start, y32, s = (batch[n] for n in ("q", "k", "v", "start", "y32", "s"))
    _, kvh, t_len, d = k.shape
    nq, nk = q.shape[2] * d, kvh * d
    buf = garbage((4, t_len, nq + 2 * nk), 51).cuda()  # [B, T, (heads + 2 kv_heads) d], k and v where a projection puts them
    km = buf[..., nq: nq + nk].view(4, t_len, kvh, d).transpose(1, 2)
    vm = buf[..., nq + nk:].view(4, t_len, kvh, d).transpose(1, 2)
    km.copy_(k), vm.copy_(v)
    assert _kv_view(km) is km and km.stride(2) == nq + 2 * nk and not km.is_contiguous()
    assert same_bits(ops.attn_prefill(q, km, vm, start, out_dtype=torch.float32), y32)
    # other finite k and v at j0, the middle of tile 1 (or of tile 0 where the sequence ends before it)
    k3, v3 = k.clone(), v.clone()
    j0 = [BK + BK // 2 if st + s > BK + BK // 2 else min(BK // 2, st + s - 1) for st in host.STARTS]
    for b in range(4):
        k3[b, :, j0[b]], v3[b, :, j0[b]] = -k[b, :, j0[b]], v[b, :, j0[b]] + 1
    y3 = ops.attn_prefill(q, k3, v3, start, out_dtype=torch.float32)
    for b, st in enumerate(host.STARTS):
        first = max(j0[b] - st, 0)  # the first row that sees j0
        assert same_bits(y3[b, :first], y32[b, :first]), b
        assert all(not same_bits(y3[b, i], y32[b, i]) for i in range(first, s)), b


@pytest.mark.parametrize("d", [32, 64, 128])
def test_one_step_is_attn_decode_bit_for_bit(gpu, d):
    """Both kernels take their softmax step from attn_mma.h, so a row that needs exactly one 32-position step
    has attn_decode's bits: every length 1..32 (slot 0; the other two slots run through them in other orders),
    the query of the last position, f32. Decode's wave merge and chunk combine then multiply by exp2(0) = 1
    and add exact zeros, and both end in one f32 division by l. Behind a length the caches hold NaN and inf
    patterns, which neither kernel loads."""
    b, kvh, group, cap = 3, 2, 4, 64
    g = torch.Generator().manual_seed(d)
    q = torch.randn(b, kvh * group, d, generator=g).to(torch.bfloat16).cuda()
    k, v = (torch.randn(b, kvh, cap, d, generator=g).to(torch.bfloat16).cuda() for _ in range(2))
    gk, gv = garbage(k.shape, 61).cuda(), garbage(k.shape, 62).cuda()
    pos = torch.arange(cap, device="cuda")[None, None, :, None]
    for n in range(1, 33):
        lens = torch.tensor([n, 33 - n, (n + 10) % 32 + 1], dtype=torch.int32, device="cuda")
        valid = pos < lens[:, None, None, None]
        kc, vc = torch.where(valid, k, gk), torch.where(valid, v, gv)
        yd = ops.attn_decode(q, kc, vc, lens, out_dtype=torch.float32)
        yp = ops.attn_prefill(q[:, None], kc, vc, lens - 1, out_dtype=torch.float32)
        assert same_bits(yp[:, 0], yd), (d, n)


@pytest.mark.parametrize("merged", [True, False], ids=["merged", "separate"])
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=list(ROPE_SHAPES))
def test_rope_append_seq_is_rope_bit_for_bit(gpu, shape, merged):
    host.check_rope_append_seq(*ROPE_SHAPES[shape], "cuda", merged)


@pytest.mark.parametrize("route", ["plain", "mxfp4"])
@pytest.mark.parametrize("spec_name", SPECS, ids=list(SPECS))
def test_forward_mfma_matches_float64(gpu, spec_name, route):
    host.check_forward_mfma(route, spec_name, "cuda")


def test_errors_gpu(gpu):
    host.check_errors("cuda")
