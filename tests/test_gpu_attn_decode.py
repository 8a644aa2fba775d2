"""ops.rope_append, ops.attn_decode (csrc/kernels/attn_decode.hip) and decoder_step on the GPU.
attn_decode_cases.py states the inputs, the float64 reference and the bound, and
test_attn_decode_host.py shows on the reference alone that the inputs discriminate.

1. rope_append: q_out and the written K rows are `_rope` on the same device at pos, bit for bit, the V
   rows are v, every other byte of both caches is unchanged; for q/k/v as slices of one merged
   buffer and as three tensors; pos mixes 0, 1, capacity - 1, values between and one outside.
2. attn_decode against float64: d 32, 64, 128, groups 1, 2, 4, 8, 16, lengths 1, 2, C - 1, C, C + 1,
   2 C + 3 and 0 as one mixed batch, NaN and +-inf behind every length: within the bound in f32 and
   bf16, the bf16 result the f32 result rounded, the empty row zero, no NaN.
   Measured on an MI355X: err / bound at most 0.32 in f32 and 0.54 in bf16 (the bound is not tightened to that).
3. Invariance, bit for bit: a sequence alone, as any slot of the mixed batch, with the capacity
   doubled, with max_len at its minimum and at the capacity, with other garbage behind its length.
4. 64-bit addressing: caches [33, 1, 2^20, 64] (4.125 GiB each); sequence 32 is written by
   rope_append (and once at position 2^20 - 1) and attends as it does in a small cache.
5. decoder_step end to end: prefill of 5 positions, 4 steps, B = 3, `tiny` and `uneven`, plain bf16
   tensors, MXFP4 (also act="mxfp8"), MXFP6 and fp8 with fuse_gated: every step row within
   2 max(e16, d_ctl) of row t of the float64 reference over all 9 tokens, d_ctl the distance of
   decoder_forward on the GPU over the 9 tokens with the same parameters and flags - nothing in
   the tolerance comes from the step. lens advance to 9 (advance=False: unchanged); the prefill's
   cache rows are decoder_forward's own rotated k and v.
6. Errors: ValueError before any launch."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import ops
from distributed_llm_dissemination_amd.models import weights as W
from distributed_llm_dissemination_amd.models.weights import decoder_forward

import attn_decode_cases as ac
import decoder_packed_reference as dp
import test_attn_decode_host as host
from test_decoder_reference import SPECS

pytestmark = pytest.mark.gpu
C = ac.C


# ---------------------------------------------------------------- 1. rope_append

@pytest.mark.parametrize("merged", [True, False], ids=["merged", "separate"])
@pytest.mark.parametrize("shape", host.ROPE_SHAPES, ids=list(host.ROPE_SHAPES))
def test_rope_append_is_rope_bit_for_bit(gpu, shape, merged):
    host.check_rope_append(*host.ROPE_SHAPES[shape], "cuda", merged)


# ---------------------------------------------------------------- 2. and 3. attn_decode

@pytest.fixture(scope="module", params=ac.CASES, ids=ac.case_id)
def batch(request, gpu):
    """Per case: the mixed batch in HBM and its f32 and bf16 results."""
    seqs = ac.sequences(*request.param)
    q, kc, vc, lens = (t.cuda() for t in ac.caches(seqs))
    y32 = ops.attn_decode(q, kc, vc, lens, out_dtype=torch.float32)
    y16 = ops.attn_decode(q, kc, vc, lens)
    torch.cuda.synchronize()
    return dict(id=ac.case_id(request.param), seqs=seqs, q=q, kc=kc, vc=vc, lens=lens, y32=y32, y16=y16)


def test_attn_decode_matches_float64(batch):
    seqs, y32, y16 = batch["seqs"], batch["y32"], batch["y16"]
    assert y32.dtype == torch.float32 and y16.dtype == torch.bfloat16
    assert tuple(y32.shape) == tuple(y16.shape) == (len(seqs), seqs[0].heads * seqs[0].d)
    w32, w16 = ac.err_over_bound(y32, seqs, False), ac.err_over_bound(y16, seqs, True)
    print(batch["id"], "err / bound: f32", w32, "bf16", w16)
    assert w32 <= 1 and w16 <= 1
    assert np.array_equal(ac.to_bits(y16), ac.to_bits(y32.to(torch.bfloat16)))


def same_bits(a, b):
    return np.array_equal(a.contiguous().view(torch.int32).cpu().numpy(), b.contiguous().view(torch.int32).cpu().numpy())


def test_a_sequence_alone_is_its_slot_of_the_batch(batch):
    for b, s in enumerate(batch["seqs"]):
        q, kc, vc, lens = (t.cuda() for t in ac.caches([s], seed=11))
        assert same_bits(ops.attn_decode(q, kc, vc, lens, out_dtype=torch.float32)[0], batch["y32"][b]), (b, s.n)
    # and at any slot: the batch reversed
    order = list(range(len(batch["seqs"])))[::-1]
    q, kc, vc, lens = (t.cuda() for t in ac.caches([batch["seqs"][i] for i in order], seed=13))
    assert same_bits(ops.attn_decode(q, kc, vc, lens, out_dtype=torch.float32), batch["y32"][order])


def test_capacity_max_len_and_garbage_change_nothing(batch):
    seqs, y32 = batch["seqs"], batch["y32"]
    q, kc, vc, lens = (t.cuda() for t in ac.caches(seqs, capacity=2 * ac.CAPACITY, seed=21))  # other garbage too
    for max_len in (max(s.n for s in seqs), 2 * ac.CAPACITY, None):
        assert same_bits(ops.attn_decode(q, kc, vc, lens, max_len=max_len, out_dtype=torch.float32), y32), max_len
    assert same_bits(ops.attn_decode(batch["q"], batch["kc"], batch["vc"], batch["lens"], max_len=max(s.n for s in seqs),
                                     out_dtype=torch.float32), y32)
    for s in seqs:  # max_len at each sequence's own minimum
        if s.n:
            qa, ka, va, la = (t.cuda() for t in ac.caches([s], capacity=s.n, seed=23))
            b = seqs.index(s)
            assert same_bits(ops.attn_decode(qa, ka, va, la, max_len=s.n, out_dtype=torch.float32)[0], y32[b]), s.n


# ---------------------------------------------------------------- 4. 64-bit addressing

def test_addresses_beyond_4_gib(gpu):
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip(f"needs 16 GiB of free device memory, {free >> 30} GiB are free")
    B, kvh, cap, d, group = 33, 1, 1 << 20, 64, 4
    n = C + 1
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(n + 1, 1, (group + 2) * d, generator=g).to(torch.bfloat16).cuda()  # one more for the last position
    big_k = torch.empty(B, kvh, cap, d, dtype=torch.bfloat16, device="cuda")
    big_v = torch.empty(B, kvh, cap, d, dtype=torch.bfloat16, device="cuda")
    assert big_k.numel() * 2 == 33 << 27
    small_k = torch.empty(1, kvh, n + 2, d, dtype=torch.bfloat16, device="cuda")
    small_v = torch.empty(1, kvh, n + 2, d, dtype=torch.bfloat16, device="cuda")
    big_t, small_t = W._rope_tables(cap, d, 500000.0, "cuda"), W._rope_tables(n + 2, d, 500000.0, "cuda")
    outside = torch.full((B,), cap, dtype=torch.int32, device="cuda")  # every other sequence: nothing is written
    for t in range(n):
        y = rows[t]
        q, k, v = y[:, : group * d], y[:, group * d: (group + 1) * d], y[:, (group + 1) * d:]
        pos = outside.clone()
        pos[32] = t
        qb = ops.rope_append(q.expand(B, -1).contiguous(), k.expand(B, -1).contiguous(), v.expand(B, -1).contiguous(),
                             *big_t, big_k, big_v, pos)
        qs = ops.rope_append(q, k, v, *small_t, small_k, small_v, pos[32:33].clone())
        assert torch.equal(qb[32], qs[0])
    assert torch.equal(big_k[32, :, :n], small_k[0, :, :n]) and torch.equal(big_v[32, :, :n], small_v[0, :, :n])
    lens = torch.zeros(B, dtype=torch.int32, device="cuda")
    lens[32] = n
    yb = ops.attn_decode(qb, big_k, big_v, lens, max_len=n, out_dtype=torch.float32)
    ys = ops.attn_decode(qs, small_k, small_v, lens[32:33].clone(), max_len=n, out_dtype=torch.float32)
    assert same_bits(yb[32], ys[0]) and not yb[:32].any() and torch.isfinite(yb).all()
    # the last position of the last sequence: the highest address of the caches
    y = rows[n]
    q, k, v = y[:, : group * d], y[:, group * d: (group + 1) * d], y[:, (group + 1) * d:]
    pos = outside.clone()
    pos[32] = cap - 1
    ops.rope_append(q.expand(B, -1).contiguous(), k.expand(B, -1).contiguous(), v.expand(B, -1).contiguous(), *big_t,
                    big_k, big_v, pos)
    kf = k.float()
    want = (kf * big_t[0][cap - 1] + torch.cat([-kf[:, d // 2:], kf[:, : d // 2]], -1) * big_t[1][cap - 1]).to(torch.bfloat16)
    assert torch.equal(big_k[32, 0, cap - 1], want[0]) and torch.equal(big_v[32, 0, cap - 1], v[0])
    assert torch.equal(big_k[32, :, :n], small_k[0, :, :n])  # and nothing before it moved


# ---------------------------------------------------------------- 5. decoder_step

@pytest.fixture(scope="module", params=[(s, r) for s in SPECS for r in host.STEP_ROUTES], ids=lambda p: f"{p[0]}-{p[1]}")
def steps(request, gpu):
    spec_name, route = request.param
    c, p, kw = host.step_params(route, spec_name, "cuda")
    ys, cache = host.run_steps(c, p, kw, "cuda")
    ctl = decoder_forward(c.xt.cuda(), p, c.spec, **kw).float().cpu().numpy()  # the existing pass over all 9 tokens
    torch.cuda.synchronize()
    return dict(c=c, p=p, kw=kw, route=route, ys=ys, cache=cache, row_d_ctl=dp.row_rel(ctl, c.y64))


def test_decoder_step_matches_float64(steps):
    c = steps["c"]
    n = host.PREFILL + host.STEPS
    assert steps["cache"].lens.tolist() == [n] * host.STEP_B and steps["cache"].max_len == n
    print(c.id, steps["route"], "worst row d_ctl / worst row e16", steps["row_d_ctl"].max() / c.row_e16.max())
    row_tol = 2 * max(c.row_e16.max(), steps["row_d_ctl"].max())
    for i, y in enumerate(steps["ys"]):
        rows = dp.row_rel(y.float().cpu().numpy()[:, 0], c.y64[:, host.PREFILL + i])
        print(c.id, steps["route"], "step", i, "worst row dist / tolerance", rows.max() / row_tol)
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (host.STEP_B, 1, c.spec.hidden)
        assert (rows <= row_tol).all()


def test_advance_false_leaves_the_lengths(steps):
    ys, cache = host.run_steps(steps["c"], steps["p"], steps["kw"], "cuda", advance=False)
    assert all(torch.equal(a, b) for a, b in zip(ys, steps["ys"]))
    n = host.PREFILL + host.STEPS
    assert torch.equal(cache.k[:, :, :n], steps["cache"].k[:, :, :n]) and torch.equal(cache.v[:, :, :n], steps["cache"].v[:, :, :n])


@pytest.mark.parametrize("route", ["plain", "mxfp4"])
@pytest.mark.parametrize("spec_name", SPECS, ids=list(SPECS))
def test_prefill_rows_are_the_forward_pass_own_k_and_v(gpu, spec_name, route):
    host.check_prefill_rows(route, spec_name, "cuda")


# ---------------------------------------------------------------- 6. errors

def test_errors_gpu(gpu):
    host.check_errors("cuda")
