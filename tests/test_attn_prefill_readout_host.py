"""attn_prefill_readout.py without a GPU: what rests on float64 alone, the builders through ops.attn_prefill's
CPU route, and that each mistake of the kernel's decomposition changes an expectation.

1. Exact inputs, from the tensors alone in float64: every (row, head) of every read-out, every-start and tie
   batch reads exactly the positions the builder says, and the next score lies at least GAP below.
   Measured: the smallest gap 181 natural units at d 32, 256 at d 64, 362 at d 128.
2. Coverage, counted: the cases hold every shape, every S, T = start + S, T % BK == 0 and start + S = 0 and 1
   mod BK; over the union of the cases (a case alone need not hold them all), under "near" the diagonal itself is read at every row index mod 32 (both column blocks) in all four
   waves, reads fall into both halves of a tile, even and odd tiles and all 32 slots of a step; under "far"
   every read lies in [0, d), under "mid" reads lie before, in and behind the middle block. The head slots of a
   row read different positions wherever min(d, start + i + 1) >= group has no factor 3 (3 s mod m is then
   one-to-one) or start + i + 1 >= d. Every tie class ties 2 (or 4) positions in the stated relation.
3. `emulate` without a mistake is the float64 reference to rounding, on random normals and on the staircases;
   with each of MISTAKES an exact expectation becomes another row or non-finite, or a staircase leaves its bound.
4. The CPU route reproduces every exact expectation bit for bit, bf16 and MXFP8, and every approximate one
   within its bound. Measured: staircases and flat softmaxes err / bound at most 6.4e-4 in f32 (the route is f32
   throughout) and 0.40 in bf16."""
import numpy as np
import pytest
import torch

import attn_decode_cases as ac
import attn_prefill_readout as pr
import decoder_packed_reference as dp
import test_attn_prefill_host as host

BQ, BK = pr.BQ, pr.BK


def exact_batches(mx=False):
    """[(name, thunk)] of every exact batch (MXFP8: d 64 and 128)."""
    ok = lambda d: not mx or d >= 64  # noqa: E731
    out = [(f"{pr.case_id(c)}-{v}", lambda c=c, v=v: pr.readout(c, v, mx)) for c in pr.READOUT_CASES if ok(c[0]) for v in pr.VARIANTS]
    out += [(f"starts-{pr.case_id(c)}-{v}", lambda c=c, v=v: pr.every_start(c, v, mx)) for c in pr.START_CASES if ok(c[0])
            for v in ("near", "far")]
    out += [(f"ties-{pr.case_id(c)}", lambda c=c: pr.ties(*c, mx)) for c in pr.TIE_SHAPES if ok(c[0])]
    out += [(f"huge-{pr.case_id(c)}", lambda c=c: pr.huge_scores(*c, mx)) for c in pr.EXTREME_SHAPES if ok(c[0])]
    if not mx:
        out += [(f"subnormal-{pr.case_id(c)}", lambda c=c: pr.subnormal_readout(*c)) for c in pr.EXTREME_SHAPES]
    return out


EXACT = exact_batches()
EXACT_MX = exact_batches(True)


def check_exact_inputs(batch):
    """The read positions and the gap from the tensors alone; returns the smallest gap."""
    worst = np.inf
    for b in range(len(batch.start)):
        tie, gap = pr.exact_scores(batch, b)
        n = tie.shape[-1]
        want = np.zeros_like(tie)
        rows = min(batch.s, batch.k.shape[2] - int(batch.start[b]))
        r = batch.read[b, :rows]
        i, h, t = np.nonzero(r >= 0)
        want[i, h, r[i, h, t]] = True
        assert (r >= 0).any(axis=-1).all() and r.max() < n  # every (row, head) reads something
        assert np.array_equal(tie[:rows], want[:rows]), b
        worst = min(worst, float(gap[:rows].min()))
    return worst


@pytest.mark.parametrize("name,thunk", EXACT, ids=[n for n, _ in EXACT])
@dp.one_thread
def test_exact_inputs_have_the_gap_in_float64(name, thunk):
    batch = thunk()
    gap = check_exact_inputs(batch)
    print(name, "smallest gap", gap, "natural units; unit", batch.unit)
    assert gap >= pr.GAP and batch.unit >= pr.GAP
    valid = torch.arange(batch.k.shape[2])[None, :] < torch.tensor(batch.ends())[:, None]
    assert not torch.isfinite(batch.k.float()[~valid[:, None].expand(-1, batch.kvh, -1)]).any()  # NaN and inf behind
    assert not torch.isfinite(batch.v.float()[~valid[:, None].expand(-1, batch.kvh, -1)]).any()


@dp.one_thread
def test_mxfp8_batches_hold_exact_codes_and_a_nan_tail():
    for c in (pr.READOUT_CASES[3], pr.READOUT_CASES[6]):
        b = pr.readout(c, "near", True)
        kc, ks, vc, vs = b.mx
        valid = (torch.arange(b.k.shape[2])[None, :] < torch.tensor(b.ends())[:, None])[:, None, :, None]
        sel, sels = valid.expand_as(kc), valid.expand_as(ks)
        deq = lambda c, s: pr.dequant(c * sel, torch.where(sels, s, torch.tensor(127, dtype=torch.uint8)))  # noqa: E731
        assert torch.equal(deq(kc, ks)[sel], b.k[sel]) and torch.equal(deq(vc, vs)[sel], b.v[sel])
        assert ((kc[~sel] & 0x7F) == 0x7F).all() and ((vc[~sel] & 0x7F) == 0x7F).all()
        assert (ks[~sels] == 0xFF).all() and (vs[~sels] == 0xFF).all()
        one = vs[0, 0, : b.ends()[0]].int()
        assert (one[:, 0] != one[:, 1]).all() and (one[1:] != one[:-1]).all()  # per (position, block)
        assert ((vc[sel] & 0x7F) != 0).all() and ((vc[sel] & 0x7F) != 0x7F).all()


@dp.one_thread
def test_cases_cover_shapes_sizes_and_alignments():
    cases = pr.READOUT_CASES
    assert {c[:3] for c in cases} == set(pr.SHAPES) and {c[3] for c in cases} == set(pr.SIZES)
    ts = [(pr.t_len(c[3], c[4]), c[3]) for c in cases]
    assert any(t == max(pr.STARTS) + s for t, s in ts) and any(t % BK == 0 for t, _ in ts)
    ends = {(st + s) % BK for _, s in ts for st in pr.STARTS}
    assert {0, 1} <= ends
    assert all(t > max(pr.STARTS) + s for (t, s), c in zip(ts, cases) if c[4] == "pad")
    assert pr.STARTS == (0, 1, BK - 1, BK, BK + 5) and pr.EVERY_START == tuple(range(2 * BK + 2))


@dp.one_thread
def test_near_far_and_mid_cover_the_kernel():
    diag, offs, halves, tiles = set(), set(), set(), set()
    for c in pr.READOUT_CASES:
        d = c[0]
        near, far, mid = (pr.readout(c, v) for v in pr.VARIANTS)
        pos = near.start.numpy()[:, None] + np.arange(near.s)[None, :]
        r = near.read[..., 0]
        assert (near.read[..., 1] < 0).all() and ((pos[:, :, None] - r) < d).all() and (r <= pos[:, :, None]).all()
        b, i, h = np.nonzero(r == pos[:, :, None])
        diag |= set(zip((i % BQ // 32).tolist(), (i % 32).tolist()))
        offs |= set((r % 32).ravel().tolist())
        halves |= set((r % BK // 32).ravel().tolist())
        tiles |= set((r // BK % 2).ravel().tolist())
        assert (far.read[..., 0] < d).all()
        nblk = -(-near.k.shape[2] // d)
        if nblk >= 3:  # rows before the middle block read near, rows behind it read inside it
            blk = mid.read[..., 0] // d
            assert {-1, 0} <= set(np.sign(blk - nblk // 2).ravel().tolist()) and (blk <= nblk // 2).all()
            assert (blk[pos >= d * (nblk // 2 + 1)] == nblk // 2).all()
        # head slots of a row read different positions
        m = np.minimum(d, pos + 1)
        ok = ((m >= near.group) & (m % 3 != 0)) | (pos + 1 >= d)
        for kv in range(near.kvh):
            rr = np.sort(r[:, :, kv * near.group: (kv + 1) * near.group], axis=-1)
            assert (rr[ok][:, 1:] != rr[ok][:, :-1]).all()
    assert diag == {(w, x) for w in range(4) for x in range(32)}
    assert offs == set(range(32)) and halves == {0, 1} and tiles == {0, 1}


@dp.one_thread
def test_every_start_batches_read_at_every_start():
    for c in pr.START_CASES:
        near, far = pr.every_start(c, "near"), pr.every_start(c, "far")
        assert near.start.tolist() == list(range(2 * BK + 2)) and near.s == 35
        assert (far.read[..., 0] < c[0]).all() and (near.read[..., 1] < 0).all()
        pos = near.start.numpy()[:, None, None] + np.arange(35)[None, :, None]
        assert ((pos - near.read[..., 0]) < c[0]).all()


@pytest.mark.parametrize("shape", pr.TIE_SHAPES, ids=pr.case_id)
@dp.one_thread
def test_tie_classes_tie_what_they_name(shape):
    d = shape[0]
    b = pr.ties(*shape)
    pos = (pr.EXT_START + np.arange(b.s))[:, None]
    for n, name in enumerate(b.names):
        r = b.read[n]
        count = (r >= 0).sum(axis=-1)
        two, four = r[count == 2], r[count == 4]
        assert len(two) + len(four) > 0 and set(np.unique(count)) <= {1, 2, 4}, name
        x = two[:, 0] ^ two[:, 1]
        if name == "one lane":
            assert (x == 1).all()
        elif name == "two lane groups":
            assert (x == 4).all()
        elif name == "all four lane groups":
            assert len(four) and (np.sort(four % 16 // 4, axis=1) == np.arange(4)).all() and np.isin(x, (4, 8, 12)).all()
        elif name == "two halves of a tile":
            assert (x == 32).all() and (two[:, 0] // BK == two[:, 1] // BK).all()
        elif name == "two tiles in different LDS buffers":
            assert (x == BK).all() and (two[:, 0] // BK % 2 != two[:, 1] // BK % 2).all()
        elif name == "tile 0 and the diagonal step":
            # every tie: a position of tile 0 with one of the block of the sequence's middle row; those of that block's
            # own rows whose class position lies in their diagonal step tie with it there: every head, 16 rows or more
            p2 = np.broadcast_to(pos, count.shape)[count == 2]
            mid = (pr.EXT_START + b.s // 2) // d
            assert (two[:, 0] < min(d, BK)).all() and (two[:, 1] // d == mid).all() and (two[:, 1] <= p2).all()
            own = two[:, 1] // 32 == p2 // 32
            assert (own == ((p2 // d == mid) & (two[:, 1] % d // 32 == p2 % d // 32))).all()
            heads = np.broadcast_to(np.arange(b.heads)[None, :], count.shape)[count == 2]
            assert set(heads[own].tolist()) == set(range(b.heads)) and len(set(p2[own].tolist())) >= 16
        else:  # the diagonal and its predecessor: odd positions tie with the one before, even ones read alone
            p = np.broadcast_to(pos, count.shape)
            assert (r[..., :2].max(axis=-1) == p).all() and ((count == 2) == (p % 2 == 1)).all() and (x == 1).all()


# ---------------------------------------------------------------- the emulation and its mistakes

@dp.one_thread
def test_emulate_is_the_reference_to_rounding():
    for c in ((32, 2, 2 * BQ + 3), (64, 8, BQ + 1), (128, 1, BK + 1), (32, 8, 1)):
        cc = host.case(*c)
        y = pr.emulate(ac.f64(cc["q"]), ac.f64(cc["k"]), ac.f64(cc["v"]), host.STARTS, c[1])
        assert np.isfinite(y).all() and np.allclose(y, cc["y64"], rtol=1e-12, atol=1e-13), c
    for c in pr.STAIR_CASES:
        for variant in pr.STAIR_VARIANTS:
            a = pr.staircase(*c, variant)
            assert np.allclose(pr.emulate_batch(a.batch), a.y64, rtol=1e-11, atol=1e-13), (c, variant)


def probes():
    """The exact batches a mistake is looked for in, the cheapest first."""
    yield "S 1", pr.readout(pr.READOUT_CASES[1], "near")
    yield "near", pr.readout(pr.READOUT_CASES[0], "near")
    yield "mid", pr.readout(pr.READOUT_CASES[0], "mid")
    yield "near kv 3", pr.readout(pr.READOUT_CASES[6], "near")
    yield "end", pr.readout(pr.READOUT_CASES[5], "far")
    yield "ties", pr.ties(*pr.TIE_SHAPES[0])


def stair_away(a, mistake):
    y = pr.emulate_batch(a.batch, mistake)
    return np.inf if not np.isfinite(y).all() else float((np.abs(y - a.y64) / a.bound).max())


@dp.one_thread
def test_the_unmistaken_emulation_reads_every_probe():
    for name, b in probes():
        assert not pr.differs(pr.emulate_batch(b), b.want), name


@pytest.mark.parametrize("mistake", pr.MISTAKES)
@dp.one_thread
def test_each_mistake_changes_an_expectation(mistake):
    for name, b in probes():
        if pr.differs(pr.emulate_batch(b, mistake), b.want):
            print(mistake, "changes", name)
            return
    pytest.fail(f"{mistake} changes no exact expectation")


@pytest.mark.parametrize("mistake", ["no_rescale_o", "no_rescale_l"])
@dp.one_thread
def test_a_lost_rescale_leaves_a_staircase_bound(mistake):
    away = {v: stair_away(pr.staircase(32, 5, v), mistake) for v in ("rising", "rising120")}
    print(mistake, "bounds away", away)
    assert away["rising"] > 1 and away["rising120"] > 1
    assert stair_away(pr.staircase(32, 5, "rising"), None) < 1e-6


# ---------------------------------------------------------------- the CPU routes

def check_exact(batch, device, what):
    """f32 y == want bit for bit, the bf16 y its rounding; of an MXFP8 batch also the bf16 route's bits on the
    dequantized cache; with T cut 2 short the rows at positions >= T zero and the others unchanged."""
    y32, y16 = pr.run(batch, device), pr.run(batch, device, torch.bfloat16)
    got, want = pr.f32_bits(y32), np.ascontiguousarray(batch.want).view(np.uint32)
    bad = np.argwhere(got != want)
    if len(bad):
        b, i, e = bad[0]
        h, dd = divmod(int(e), batch.d)
        name = batch.names[b] if batch.names else ""
        raise AssertionError(f"{what} {name}: {len(bad)} of {got.size} elements differ, rows {sorted(set(bad[:, 1]))[:8]}; "
                             f"first b {b} (start {int(batch.start[b])}) row {i} head {h} d {dd}: got {y32[b, i, e].item()!r} "
                             f"want {batch.want[b, i, e]!r}, reads {batch.read[b, i, h].tolist()}")
    assert np.array_equal(ac.to_bits(y16), ac.to_bits(torch.from_numpy(batch.want).to(torch.bfloat16)))
    if batch.mx is not None:
        assert np.array_equal(got, pr.f32_bits(pr.run(batch, device, mx=False)))
    return y32


def check_cut(batch, device, y32):
    t = batch.k.shape[2]
    last = int(batch.start.max()) + batch.s
    cut = min(t, last) - 2
    if cut < 1:
        return
    yc = pr.run(batch, device, t_cut=cut)
    pos = batch.start.numpy()[:, None] + np.arange(batch.s)[None, :]
    got, ref = pr.f32_bits(yc), pr.f32_bits(y32)
    assert (pos >= cut).any() and not got[pos >= cut].any() and np.array_equal(got[pos < cut], ref[pos < cut])


@pytest.mark.parametrize("name,thunk", EXACT + EXACT_MX, ids=[n for n, _ in EXACT] + ["mx-" + n for n, _ in EXACT_MX])
@dp.one_thread
def test_cpu_route_reads_out_bit_for_bit(name, thunk):
    batch = thunk()
    y32 = check_exact(batch, "cpu", name)
    if name.endswith("near") and not name.startswith("starts"):
        check_cut(batch, "cpu", y32)


def hold(a, device, what):
    """An Approx within its float64 bound in f32 and bf16; returns (err / bound f32, bf16, the f32 result)."""
    y32, y16 = pr.run(a.batch, device), pr.run(a.batch, device, torch.bfloat16)
    got, got16 = y32.cpu().numpy().astype(np.float64), y16.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and (a.bound > 0).all()
    w32 = float((np.abs(got - a.y64) / a.bound).max())
    w16 = float((np.abs(got16 - a.y64) / (a.bound + 2.0 ** -9 * np.abs(a.y64))).max())
    print(what, "err / bound: f32", w32, "bf16", w16)
    assert w32 <= 1 and w16 <= 1
    return w32, w16, y32


@pytest.mark.parametrize("case", pr.STAIR_CASES, ids=lambda c: "d%d-g%d" % c)
@dp.one_thread
def test_cpu_route_holds_the_staircases(case):
    for variant in pr.STAIR_VARIANTS:
        a = pr.staircase(*case, variant)
        hold(a, "cpu", f"d{case[0]}-g{case[1]} {variant}")


@pytest.mark.parametrize("shape", pr.EXTREME_SHAPES, ids=pr.case_id)
@dp.one_thread
def test_cpu_route_holds_the_flat_extremes(shape):
    hold(pr.extreme_v(*shape, 100), "cpu", f"{pr.case_id(shape)} V at 2^100")
    hold(pr.extreme_v(*shape, -100), "cpu", f"{pr.case_id(shape)} V at 2^-100")


@dp.one_thread
def test_visiting_rows_are_fewer_than_63_positions_before():
    for st, s, j in ((BK + 5, BQ + 1, 150), (3, BQ + 1, 100), (0, 2 * BQ, 32), (BK + 5, BQ + 1, BK + 5)):
        rows = pr.visiting_rows(st, s, j)
        assert ((j - (st + rows) > 0) & (j - (st + rows) < 63)).all()
        first_wave = (j - st) // 32 if j >= st else -1  # the wave of j's own row visits j's step
        assert set(range(max(32 * first_wave, 0), max(j - st, 0))) <= set(rows.tolist())
