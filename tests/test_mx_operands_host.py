"""The hand-made MXFP8 operands of mx_operands.py on the CPU, on the reference alone: that numpy's
dequantization is the right one (a second, independent one agrees on every (code, scale byte)
pair), that every builder covers what its docstring names, that every exactness proof holds, and
that each defect a W4A8 kernel could have - flushed subnormals, the scale byte of another block,
the A operand read as 32 consecutive k per lane, a code that falls out of the three classes or into
two of them - changes the expectation wherever it should (one mutated-reference helper,
mx_operands.mutated_want). test_gpu_mxfp4_mx_extremes.py runs the same cases through the gfx950
kernels.

Also recorded here: where the host's weight route (bf16) differs from code * 2^(byte - 127)."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import ops
from distributed_llm_dissemination_amd.ops import kernels

import linear_extremes as le
import mx_operands as mo
import test_mxfp4_linear_host as mx
from mx_operands import BM, BN, KS, SWAPS
from test_gpu_mxfp4_linear import LAYOUTS
from test_mxfp4_mx_host import dequantize, host_quantize


def differs(a, b):
    """Elementwise a != b with NaN equal to NaN."""
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


@pytest.fixture(scope="module")
def cases():
    """Every case once, shared and never written to."""
    out = {}
    for k in KS:
        out["a", k], out["a mid", k] = mo.readout_a(k), mo.readout_a(k, mid=True)
        out["c", k], out["c2", k] = mo.association(k), mo.association(k, live=2)
        out["b", k] = mo.readout_b(k, "rows straddle 1024-B chunks")
    for k in (160, 288):
        out["d", k] = mo.boundaries(k)
    return out


# ---------------------------------------------------------------- the reference itself

def test_a_second_dequantization_agrees_on_every_pair():
    """numpy's code * 2^(byte - 127) against torch's float8_e4m3fn and ldexp (ops.kernels._mxfp8_values)
    on all 256 x 255 (code, scale byte) pairs: equal values (f32 holds every one below 2^128 exactly,
    the rest are inf in both once cast), NaN at the same places."""
    codes = np.repeat(np.arange(256, dtype=np.uint8)[None, :], 32, 0).T.copy()  # [256, 32]: row = code
    for byte in range(255):
        scales = np.full((256, 1), byte, dtype=np.uint8)
        want = dequantize(codes, scales)
        got = kernels._mxfp8_values(torch.from_numpy(codes), torch.from_numpy(scales)).numpy()
        assert got.dtype == np.float32
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(nan[:, 0], (np.arange(256) & 0x7F) == 0x7F)
        with np.errstate(over="ignore"):
            assert np.array_equal(got[~nan], want[~nan].astype(np.float32)), byte
        fin = ~nan & (np.abs(want) < mo.F32_TOP)
        assert np.array_equal(got[fin].astype(np.float64), want[fin]), byte


def test_the_finite_in_f32_restriction_leaves_out_only_what_it_says():
    """x: a code of exponent field f >= 8 is at least 2^(f - 7), so it reaches 2^128 under the f - 7
    bytes 255 - (f - 7) .. 254: 16 codes per field 8..14 and 14 of field 15, 16 (1 + .. + 7) + 14 * 8
    = 560 of the 254 * 255 pairs. w: 4 and 6 under byte 253 and 2, 3, 4, 6 under 254, both signs: 12
    of the 16 * 255. The builders lower exactly the elements that hold such a pair and every other
    pair stays as drawn."""
    codes = np.repeat(mo.CODES254[:, None], 32, 1)
    over = np.stack([np.abs(dequantize(codes, np.full((254, 1), b, dtype=np.uint8)))[:, 0] >= mo.F32_TOP
                     for b in range(255)], 1)  # [code, byte]
    formula = sum(16 * (f - 7) for f in range(8, 15)) + 14 * 8
    assert int(over.sum()) == formula == 560
    f = mo.field_of(mo.CODES254)
    assert np.array_equal(over.sum(1), np.where(f >= 8, f - 7, 0))
    nib = np.repeat(np.arange(16, dtype=np.uint8)[:, None], 32, 1)
    wover = np.stack([np.abs(mo.w_values(nib, np.full((16, 1), b, dtype=np.uint8)))[:, 0] >= mo.F32_TOP
                      for b in range(255)], 1)
    assert int(wover.sum()) == 2 * (2 + 4) == 12
    assert {(int(n), int(b)) for n, b in np.argwhere(wover)} == \
        {(s | n, 253) for s in (0, 8) for n in (6, 7)} | {(s | n, 254) for s in (0, 8) for n in (4, 5, 6, 7)}
    seen = 0
    for k in KS:
        c = mo.readout_a(k)
        raw, ch = c.extra["raw"], c.extra["restricted"]
        assert np.array_equal(ch, np.abs(dequantize(raw, c.scales)) >= mo.F32_TOP)
        assert np.array_equal(c.codes[~ch], raw[~ch]) and np.array_equal(c.codes[ch], raw[ch] - 0x40)
        seen += int(ch.sum())
        assert not mo.readout_a(k, mid=True).extra["restricted"].any()
        b = mo.readout_b(k, "rows straddle 1024-B chunks")
        raw, ch = b.extra["raw"], b.extra["restricted"]
        assert np.array_equal(ch, np.abs(mo.w_values(raw, b.extra["sb"])) >= mo.F32_TOP) and ch.any()
        assert np.array_equal(b.extra["nib"][~ch], raw[~ch])
    assert seen


def test_where_the_host_weight_route_differs():
    """ops.mxfp4_unpack_range (bf16) against code * 2^(byte - 127) on all 16 x 255 (nibble, scale byte)
    pairs. bf16 has f32's exponents and a code has two significant bits, so every value from 2^-128
    (0.5 under byte 0, a bf16 subnormal) up to 1.5 * 2^127 is held exactly; the pairs that differ are
    the 12 whose value reaches 2^128 - 4 and 6 under byte 253, 2, 3, 4 and 6 under byte 254, either
    sign - where bf16 gives +-inf. Byte 0xFF is NaN in both."""
    nib = np.repeat(np.arange(16, dtype=np.uint8)[:, None], 32, 1)  # [16, 32]: row = nibble
    diff = set()
    for byte in range(255):
        sb = np.full((16, 1), byte, dtype=np.uint8)
        img, total, offs = mo.weight_image([(nib, sb)], 1024, 0, 0, 1)
        got = ops.mxfp4_unpack_range(torch.from_numpy(img), 2 * total, 1024, 0, 16 * 32)
        got = mx.bits_to_f64(mx.bf16_tensor_bits(got)).reshape(16, 32)
        assert np.array_equal(got, mx.ref_weight(img, total, 1024, 0, 16, 32))
        want = mo.w_values(nib, sb)
        for n in np.nonzero((got != want).any(1))[0]:
            assert np.isinf(got[n]).all() and (np.sign(got[n]) == np.sign(want[n])).all()
            diff.add((int(n), byte))
    assert diff == {(s | n, 253) for s in (0, 8) for n in (6, 7)} | {(s | n, 254) for s in (0, 8) for n in (4, 5, 6, 7)}
    assert all(abs(float(mo.E2M1[n & 7])) * 2.0 ** (b - 127) >= mo.F32_TOP for n, b in diff)
    img, total, _ = mo.weight_image([(nib, np.full((16, 1), 0xFF, dtype=np.uint8))], 1024, 0, 0, 1)
    assert bool(torch.isnan(ops.mxfp4_unpack_range(torch.from_numpy(img), 2 * total, 1024, 0, 16 * 32).float()).all())


# ---------------------------------------------------------------- a. the A path

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mid", [False, True], ids=["0..254", "100..140"])
def test_a_covers_codes_lanes_pieces_and_scales(cases, k, mid):
    c = cases["a mid" if mid else "a", k]
    assert (c.m, c.n) == (BM + 1, k) and np.array_equal(c.want, c.xh[:, :k]) and np.array_equal(c.wf, np.eye(k))
    assert np.isfinite(c.want).all() and le.f32_representable(c.want)
    kk = np.arange(k)
    for lane in range(4):  # every code in every byte lane of a dword
        assert np.array_equal(np.unique(c.codes[:, kk % 4 == lane]), mo.CODES254)
    for p in range(8):     # every code in every 16-byte piece of a step, in every lane of it
        for lane in range(4):
            assert np.array_equal(np.unique(c.codes[:, ((kk % 128) // 16 == p) & (kk % 4 == lane)]), mo.CODES254), (p, lane)
        for r in range(16):  # every row position meets every piece with every class and a non-zero value
            part = c.codes[r::16][:, (kk % 128) // 16 == p]
            assert set(np.unique(mo.class_of(part[(part & 0x7F) != 0]))) == {0, 1, 2}, (r, p)
    s4 = mo._steps(c.scales)[:, : k // 128]  # the full steps; the tail below
    assert all((s4[:, :, i] != s4[:, :, j]).all() for i, j in SWAPS)
    tail = c.scales[:, 4 * (k // 128):].astype(int)
    assert tail.shape[1] == (k % 128) // 32 and all((tail[:, i] != tail[:, j]).all()
                                                    for i in range(tail.shape[1]) for j in range(i))
    if mid:
        assert c.scales.min() == 100 and c.scales.max() == 140
    else:
        assert set(range(248, 255)) | {0} <= set(np.unique(c.scales).tolist())
        sub = (c.want != 0) & (np.abs(c.want) < 2.0 ** -126)
        assert sub.any(1).sum() >= 16 and (np.abs(c.want) >= 2.0 ** 127).any()  # both ends of f32 are reached


def test_a_scale_bytes_range_over_all_255(cases):
    assert set(np.unique(np.concatenate([cases["a", k].scales.reshape(-1) for k in KS])).tolist()) == set(range(255))


@pytest.mark.parametrize("k", KS)
def test_a_discriminates(cases, k):
    c = cases["a", k]
    sub = (c.want != 0) & (np.abs(c.want) < 2.0 ** -126)
    assert np.array_equal(differs(mo.mutated_want(c, "flush"), c.want), sub) and sub.any()
    live = np.repeat(mo._steps(np.ones_like(c.scales)) == 1, 32, -1).reshape(c.m, -1, 4, 32)  # [m, step, block, 32]
    for i, j in SWAPS:  # every row changes, in every step that has block i
        d = differs(mo.mutated_want(c, "swap", (i, j)), c.want)
        pad = np.zeros((c.m, live.shape[1] * 128), dtype=bool)
        pad[:, :k] = d
        per_step = pad.reshape(c.m, -1, 4, 32).any(-1)
        s4 = mo._steps(c.scales)  # an absent block of the tail lends byte 127, which block i may carry itself
        assert np.array_equal(per_step[:, :, i], live[:, :, i, 0] & (s4[:, :, i] != s4[:, :, j])), (i, j)
        assert per_step[:, : k // 128, i].all()
        assert not per_step[:, :, [g for g in range(4) if g != i]].any()
    assert differs(mo.mutated_want(c, "lanes32"), c.want).any(1).all()
    mid_c = cases["a mid", k]  # the variant that stands on its own sees the same defects
    assert differs(mo.mutated_want(mid_c, "lanes32"), mid_c.want).any(1).all()
    assert all(differs(mo.mutated_want(mid_c, "swap", s), mid_c.want).any(1).all() for s in SWAPS)
    # the gated kernel's second operand stays finite in f32 under either variant, and silu(g) u leaves f32 here only
    for cc, leaves in ((c, True), (mid_c, False)):
        u = mo.matmul64(cc.xh, cc.up_weight())
        assert (np.abs(cc.xh) @ np.abs(cc.up_weight()).T).max() < 2.0 ** 127
        assert (np.abs(cc.want * cc.want).max() >= mo.F32_TOP) == leaves and (np.abs(cc.want * u).max() >= mo.F32_TOP) == leaves
    for f in range(16):
        hit = (mo.field_of(c.codes) == f) & ((c.codes & 0x7F) != 0)
        assert hit.any(1).sum() >= BM  # in (nearly) every row
        for kind in ("drop", "double"):
            assert np.array_equal(differs(mo.mutated_want(c, kind, f), c.want), hit), (kind, f)


# ---------------------------------------------------------------- b. the B path

@pytest.mark.parametrize("k", KS)
def test_b_covers_nibbles_and_scales_and_discriminates(cases, k):
    c = cases["b", k]
    nib, sb = c.extra["nib"], c.extra["sb"]
    assert (c.m, c.n) == (k, BN + 16) and np.array_equal(c.want, c.wf.T)
    assert np.array_equal(c.wf, mo.w_values(nib, sb)) and np.isfinite(c.wf).all() and le.f32_representable(c.wf)
    for par in (0, 1):  # all 16 nibbles at both nibble positions of a byte
        assert np.array_equal(np.unique(nib[:, par::2]), np.arange(16))
    s4 = mo._steps(sb)[:, : k // 128]
    assert all((s4[:, :, i] != s4[:, :, j]).all() for i, j in SWAPS)
    assert {0, 253, 254} <= set(np.unique(sb).tolist())
    sub = (c.want != 0) & (np.abs(c.want) < 2.0 ** -126)
    assert np.array_equal(differs(mo.mutated_want(c, "flush"), c.want), sub) and sub.any(0).sum() >= 4
    for i, j in SWAPS:  # every column changes: every weight row has non-zero nibbles in block i of the first step
        assert differs(mo.mutated_want(c, "wswap", (i, j)), c.want).any(0).all(), (i, j)


def test_b_scale_bytes_range_over_all_255():
    seen = set()
    for k in KS:
        for layout in LAYOUTS:
            c = mo.readout_b(k, layout)
            assert np.array_equal(c.wf, mo.w_values(c.extra["nib"], c.extra["sb"])), (k, layout)  # the layout holds what was put in
            seen |= set(np.unique(c.extra["sb"]).tolist())
    assert seen == set(range(255))


# ---------------------------------------------------------------- c. scale association

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("live", [1, 2])
def test_c_is_exact_covers_every_block_and_discriminates(cases, k, live):
    c = cases["c" if live == 1 else "c2", k]
    nb = k // 32
    assert (c.m, c.n) == (2 * BM + 5, 48)
    mo.prove_rows(c)
    mo.prove_rows(c, wf=c.up_weight())  # the gated kernel's second operand too
    rows = np.arange(c.m)
    nz = (c.codes.reshape(c.m, nb, 32) != 0).any(-1)
    assert (nz.sum(1) == live).all()
    b1, s1 = c.extra["live_blocks"][0], c.extra["live_scales"][0]
    assert (s1 != 127).all()  # 127 is what an absent block of the tail lends
    for r in range(16):  # every block is the live one in some row of every row position
        assert set(b1[r::16].tolist()) == set(range(nb)), r
    for bv, sv in zip(c.extra["live_blocks"], c.extra["live_scales"]):
        assert nz[rows, bv].all() and np.array_equal(c.scales[rows, bv], sv)
        decoys = np.where(nz, -1, c.scales.astype(int))
        assert not (decoys == sv[:, None]).any()
    if live == 2:
        d = c.extra["live_scales"][1] - s1
        assert d.min() == 0 and d.max() == 8
        f = mo.field_of(c.codes[c.codes != 0])
        assert set(np.unique(f).tolist()) == {5, 6}  # either side of the class boundary
    else:
        assert set(np.unique(mo.class_of(c.codes[c.codes != 0])).tolist()) == {0, 1, 2}
    assert (c.want != 0).any(1).all()
    for i, j in SWAPS:  # the rows whose (first) live block is block i of its step
        d = differs(mo.mutated_want(c, "swap", (i, j)), c.want).any(1)
        lent = mo._steps(c.scales)[rows, b1 // 4, j]  # a decoy, or the second live byte, which may equal the first
        hit = (b1 % 4 == i) & (lent != s1)
        assert d[hit].all() and hit.sum() >= (b1 % 4 == i).sum() - (live == 2) * c.m // 8 > 0, (i, j)
    assert differs(mo.mutated_want(c, "lanes32"), c.want).any(1).all()


# ---------------------------------------------------------------- d. class boundaries

@pytest.mark.parametrize("k", [160, 288])
def test_d_is_exact_and_discriminates(cases, k):
    c = cases["d", k]
    mixed, f64 = c.extra["mixed"], c.extra["float64"]
    plain = np.nonzero(~mixed)[0]
    mo.prove_rows(c, rows=plain)
    assert np.array_equal(c.want[plain], f64[plain])  # the chain rounds nowhere: exact in f32
    # the rows with all three classes in one group: the f32 chain is itself within the bound
    assert mixed.sum() >= 2 * len(mo.group_positions(k))
    err, bound = np.abs(c.want - f64)[mixed], mo.f32_bound(c.xh, c.wf)[mixed]
    print("mixed rows: chain != float64 in", int((err != 0).sum()), "of", err.size, "worst err / bound",
          float((err / bound).max()))
    assert (err <= bound).all() and le.f32_representable(c.want)
    ties = np.array([mixed[r] and c.extra["configs"][r % len(c.extra["configs"])][0] is not None for r in range(c.m)])
    rounded = c.want != f64
    assert rounded[ties][:, [7, 15]].all() and not rounded[:, [i for i in range(16) if i % 8 != 7]].any()  # the ties, and only they
    half = np.abs(c.want - f64)[ties][:, [7, 15]] / np.spacing(np.abs(c.want[ties][:, [7, 15]]).astype(np.float32))
    assert (half == 0.5).all() and ties.sum() >= 2 * len(mo.TIES) * len(mo.group_positions(k)) - len(mo.group_positions(k))
    # every pair at every position, and the small code alone is the answer in columns j and j + 8
    seen = set()
    for r in plain:
        pair, g0, j = c.extra["configs"][r % len(c.extra["configs"])]
        seen.add((pair, g0))
        small = c.xh[r, g0 + j]
        assert small != 0 and np.array_equal(f64[r, [j, j + 8]], small * c.wf[[j, j + 8], g0 + j])
        assert (np.abs(c.wf[[j, j + 8], g0 + j]) == 0.5 * 2.0 ** (c.extra["sb"][[j, j + 8], g0 // 32].astype(int) - 127)).all()
    assert seen == {(p, g0) for p in mo.PAIRS for g0 in mo.group_positions(k)}
    assert mo.group_positions(k)[-1] >= 128 * (k // 128) and mo.group_positions(k)[2] % 128 == 120
    assert (c.want != 0).any(1).all()
    for f in sorted({int(x) for x in mo.field_of(np.array(sum(map(list, mo.PAIRS), []) + mo.MIXED + mo.TIES))}):
        rows = ((mo.field_of(c.codes) == f) & ((c.codes & 0x7F) != 0)).any(1)
        assert rows.any()
        for kind in ("drop", "double"):
            d = differs(mo.mutated_want(c, kind, f), c.extra["float64"]).any(1)
            assert np.array_equal(d, rows), (kind, f)


# ---------------------------------------------------------------- e, f

def test_e_is_wide():
    c = mo.wide()
    assert (c.m, c.n, c.k) == (2 * BM + 5, BN + 16, 1120) and c.k % 128 == 96
    assert c.scales.min() == 90 and c.scales.max() == 160
    assert np.array_equal(np.unique(c.codes), mo.CODES254)
    sb = np.concatenate([c.img[so: so + n // 32] for _, n, _, so in mx.chunk_table(c.total, c.chunk)])
    assert np.isfinite(c.want).all() and np.isfinite(c.wf).all() and sb.max() <= 150
    wsb = c.extra["sb"]
    assert wsb.min() == 100 and wsb.max() == 150
    # a scale byte one block off is far outside the bound
    bound = mo.f32_bound(c.xh, c.wf)
    assert (np.abs(mo.mutated_want(c, "swap", (0, 1)) - c.want) > bound).any(1).all()
    assert (np.abs(mo.mutated_want(c, "lanes32") - c.want) > bound).any(1).all()


def test_f_expectations_come_out_of_the_arithmetic():
    c, variants = mo.nonfinite()
    assert np.isfinite(c.want).all()
    assert len(variants) == 3 * 2 * 2 + 10 * 2
    pieces = set()
    for v in variants:
        want = mo.variant_want(c, v)
        nan = np.zeros_like(want, dtype=bool)
        nan[v["rows"]] = True
        nan[:, v["cols"]] = True
        assert np.array_equal(np.isnan(want), nan), v["name"]
        if "zero_at" in v:
            n0, kk = v["zero_at"]
            wf = mx.ref_weight(v["img"], c.total, c.chunk, c.off, c.n, c.k)
            assert wf[n0, kk] == 0 and np.isnan(wf[mo.NAN_COL, kk]) and np.isfinite(wf[n0]).all()
            pieces.add(kk // 16)
            assert v["codes"][v["rows"][0], kk] & 0x7F == 0x7F
    assert pieces == set(range(10))


# ---------------------------------------------------------------- what the quantizer can make

@pytest.mark.parametrize("name,k", [("a", 160), ("a", 224), ("a", 288), ("d", 160), ("d", 288)])
def test_some_rows_are_what_the_quantizer_makes(cases, name, k):
    """The bf16 form of some rows of builders a and d quantizes, on the host codec, to exactly the
    hand-made codes and scale bytes: the GPU file runs those through ops.mxfp4_linear(act="mxfp8")."""
    c = cases[name, k]
    x, rows = mo.rows_the_quantizer_makes(c, host_quantize)
    print(c.name, "rows the quantizer makes:", len(rows), "of", c.m)
    assert len(rows) >= 1
    q, s = host_quantize(x[rows])
    assert np.array_equal(q, c.codes[rows]) and np.array_equal(s, c.scales[rows])
    assert np.array_equal(dequantize(q, s), c.xh[rows])
