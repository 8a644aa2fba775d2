"""ops.attn_prefill on the GPU (csrc/kernels/attn_prefill.hip, attn_prefill_mxfp8.hip) on hand-made operands and
at its numeric extremes. test_gpu_attn_prefill.py holds random normals to a bound and launches to each other;
here every row reads out one position among all it may see. attn_prefill_readout.py states the inputs and why
their results are exact; test_attn_prefill_readout_host.py shows on float64 alone that they are, what they
cover, and that each mistake of the kernel's decomposition changes an expectation.

1. Causal one-hot read-outs, "near", "far" and "mid", at (d, group, KV heads) (32, 3, 1), (32, 16, 3), (64, 7, 2),
   (128, 1, 1), (128, 5, 3), (128, 12, 1), S 1 .. 2 BQ + 3 behind starts (0, 1, BK - 1, BK, BK + 5), T = start + S, T % BK
   == 0 and NaN and inf behind start + S: f32 y[b, i, h] is the V row at the read position bit for bit, the bf16
   result that row; with T cut 2 short the rows at positions >= T are zero and the others keep their bits. Through
   an MXFP8 cache (d 64, 128; NaN codes under scale bytes 0xFF behind start + S) the dequantized V row, and the bits
   of the bf16 kernel on the dequantized cache.
2. Every start 0 .. 2 BK + 1 in one batch, S = 35, "near" and "far": bit for bit.
3. Ties of 2 and 4 equal keys in one lane, two and four lane groups, the halves of a tile, two tiles in
   different LDS buffers, tile 0 and the diagonal step, the diagonal and its predecessor: the f32 sum of the V
   rows over their number, bit for bit, one launch per class and all as one.
4. The order of the maxima against float64: a key every row scores alike in every 32-position step, rising and
   falling by 3 natural units a step, rising by 120 (every alpha underflows to 0) and flat under a maximum in
   the row's own diagonal step: err / bound <= 1 in f32 and bf16, the bound 2^-7 sum p |v| (2^-9 |y64| more).
   Measured on an MI355X: err / bound at most 0.30 in f32 and 0.58 in bf16 (rising by 120: 0, the result is one
   V row; the bound is not tightened to that).
5. Extremes: one-hot scores of 2^122.8 (d 32) and 2^124 beside -2^125 (d 128) and bf16-subnormal V rows read out
   bit for bit; V at 2^100 and 2^-100 under a flat softmax within the float64 bound.
   Measured on an MI355X: err / bound at most 3.9e-6 in f32 and 0.25 in bf16 for both V magnitudes.
6. Non-finite operands as ops.attn_prefill's docstring states them, against a clean run: a NaN at K position j
   makes the rows at and behind j NaN in the query heads of that (sequence, KV head); +inf at V element (j, d0)
   makes d0 +inf in those rows and NaN in the rows before j whose wave still visits j's step
   (attn_prefill_readout.visiting_rows derives them from the kernel); a NaN code or a scale byte of 255 in an
   MXFP8 K or V acts as the NaN values it dequantizes to. Every other bit is the clean run's."""
import dataclasses

import numpy as np
import pytest
import torch

import attn_decode_cases as ac
import attn_prefill_readout as pr
import test_attn_prefill_readout_host as host

pytestmark = pytest.mark.gpu

ALL = host.EXACT + [("mx-" + n, t) for n, t in host.EXACT_MX]
READOUTS = [(n, t) for n, t in ALL if "ties" not in n]


# ---------------------------------------------------------------- 1., 2., 5. exact read-outs

@pytest.mark.parametrize("name,thunk", READOUTS, ids=[n for n, _ in READOUTS])
def test_every_row_and_head_reads_its_v_row(gpu, name, thunk):
    batch = thunk()
    y32 = host.check_exact(batch, "cuda", name)
    if name.endswith("near") and "starts" not in name:
        host.check_cut(batch, "cuda", y32)


# ---------------------------------------------------------------- 3. ties

TIES = [(c, False) for c in pr.TIE_SHAPES] + [(c, True) for c in pr.TIE_SHAPES if c[0] >= 64]  # MXFP8: d 64 and 128


@pytest.mark.parametrize("shape,mx", TIES, ids=[pr.case_id(c) + ("-mxfp8" if mx else "") for c, mx in TIES])
def test_ties_merge_exactly(gpu, shape, mx):
    b = pr.ties(*shape, mx)
    for i, name in enumerate(b.names):  # per class, so that a failure names the merge
        host.check_exact(b.only(i), "cuda", f"{pr.case_id(shape)} {name}")
    host.check_exact(b, "cuda", pr.case_id(shape))  # and as one launch


# ---------------------------------------------------------------- 4. the order of the maxima, 5. flat extremes

def hold(a, what):
    w32, w16, y32 = host.hold(a, "cuda", what)
    y16 = pr.run(a.batch, "cuda", torch.bfloat16)
    assert np.array_equal(ac.to_bits(y16), ac.to_bits(y32.to(torch.bfloat16)))


@pytest.mark.parametrize("case", pr.STAIR_CASES, ids=lambda c: "d%d-g%d" % c)
def test_staircases_match_float64(gpu, case):
    for variant in pr.STAIR_VARIANTS:
        hold(pr.staircase(*case, variant), f"d{case[0]}-g{case[1]} {variant}")


@pytest.mark.parametrize("shape", pr.EXTREME_SHAPES, ids=pr.case_id)
def test_flat_softmax_over_extreme_v_within_the_float64_bound(gpu, shape):
    hold(pr.extreme_v(*shape, 100), f"{pr.case_id(shape)} V at 2^100")
    hold(pr.extreme_v(*shape, -100), f"{pr.case_id(shape)} V at 2^-100")


# ---------------------------------------------------------------- 6. non-finite operands

J, D0 = 2 * pr.BK + 22, 17  # position (sequence 0: start BK + 5; tile 2, the step at 2 BK) and element


def _masks(batch, b, kv, j, dsel):
    """(behind, before) bool [B, S, heads, d]: element(s) dsel of the query heads of (b, kv) in the rows at and
    behind position j, and in the earlier rows whose wave still visits j's step."""
    st, s = int(batch.start[b]), batch.s
    behind, before = (np.zeros((len(batch.start), s, batch.heads, batch.d), dtype=bool) for _ in range(2))
    heads = slice(kv * batch.group, (kv + 1) * batch.group)
    behind[b, max(j - st, 0):, heads, dsel] = True
    rows = pr.visiting_rows(st, s, j)
    gap = j - (st + rows)  # a whole wave of rows before j's own, and its own rows before j: fewer than 63 positions
    assert len(rows) > pr.STEP and rows.max() == j - st - 1 and (gap > 0).all() and gap.max() < 2 * pr.STEP - 1
    before[b, rows, heads, dsel] = True
    return behind, before


def _y(batch, mx=None):
    y = pr.run(batch, "cuda", mx=mx)
    return y.cpu().numpy().reshape(len(batch.start), batch.s, batch.heads, batch.d)


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


@pytest.mark.parametrize("shape", pr.EXTREME_SHAPES, ids=pr.case_id)
def test_nan_in_k_and_inf_in_v_reach_the_rows_the_docstring_names(gpu, shape):
    b = pr.ordinary(*shape)
    kv = shape[2] - 1
    clean = _y(b)
    assert np.isfinite(clean).all()
    k = b.k.clone()
    k[0, kv, J, 5] = float("nan")
    y = _y(dataclasses.replace(b, k=k))
    behind, _ = _masks(b, 0, kv, J, slice(None))
    assert np.isnan(y[behind]).all() and np.array_equal(_bits(y)[~behind], _bits(clean)[~behind])
    v = b.v.clone()
    v[0, kv, J, D0] = float("inf")  # ordinary scores: every position a row sees has weight
    y = _y(dataclasses.replace(b, v=v))
    behind, before = _masks(b, 0, kv, J, D0)
    assert (y[behind] == np.inf).all() and np.isnan(y[before]).all()
    rest = ~(behind | before)
    assert np.array_equal(_bits(y)[rest], _bits(clean)[rest])


@pytest.mark.parametrize("what", ["k code", "k scale", "v code", "v scale"])
def test_nan_codes_and_scale_bytes_of_255_act_as_the_nan_they_dequantize_to(gpu, what):
    shape = pr.EXTREME_SHAPES[1]
    b = pr.ordinary(*shape, mx=True)
    kv = shape[2] - 1
    clean = _y(b)
    assert np.isfinite(clean).all() and np.array_equal(_bits(clean), _bits(_y(b, mx=False)))
    mx = [t.clone() for t in b.mx]
    k, v = b.k.clone(), b.v.clone()
    block = slice(32 * (D0 // 32), 32 * (D0 // 32) + 32)
    if what == "k code":
        mx[0][0, kv, J, D0], k[0, kv, J, D0], dsel = 0x7F, float("nan"), slice(None)
    elif what == "k scale":
        mx[1][0, kv, J, D0 // 32], k[0, kv, J, block], dsel = 0xFF, float("nan"), slice(None)
    elif what == "v code":
        mx[2][0, kv, J, D0], v[0, kv, J, D0], dsel = 0xFF, float("nan"), D0
    else:
        mx[3][0, kv, J, D0 // 32], v[0, kv, J, block], dsel = 0xFF, float("nan"), block
    bad = dataclasses.replace(b, k=k, v=v, mx=tuple(mx))
    y, y_bf16 = _y(bad), _y(bad, mx=False)
    behind, before = _masks(b, 0, kv, J, dsel)
    nan = behind if what[0] == "k" else behind | before
    assert np.isnan(y[nan]).all() and np.array_equal(_bits(y)[~nan], _bits(clean)[~nan])
    assert np.array_equal(np.isnan(y), np.isnan(y_bf16)) and np.array_equal(_bits(y)[~nan], _bits(y_bf16)[~nan])
