"""attn_mxfp8_readout.py without a GPU: the MXFP8 decode read-outs on float64 and through ops.attn_decode's CPU
route (the valid prefix dequantized, then the definition in f32).

Per batch: in float64, on the DEQUANTIZED caches, every other score lies at least 128 natural units below a
head's spike score and tied scores are equal (test_attn_readout_host.check_exact_inputs; measured: the gap from
253 at d 64 and 359 at d 128), `want` is the float64 sum of the spike rows over their number, no two V rows of
a sequence are equal, the codes dequantize to the caches the reference holds, a K row's scale bytes differ
across its blocks and V's per (position, block), NaN codes under 0xFF lie behind every length; the CPU route
gives `want` bit for bit in f32 and its rounding in bf16.
The read-out batch (2 C + 3 sequences of 2 C + 3 positions) runs every 16th sequence of 4 of the GPU file's 12
shapes here - every d, group and KV head count - the length batch every 8th length and the empty sequence, the
tie batch all 12 shapes whole. On one BLAS / OpenMP thread, as the neighbouring host files."""
import numpy as np
import pytest
import torch

import attn_decode_cases as ac
import attn_mxfp8_readout as mq
import attn_readout as ar
import decoder_packed_reference as dp
import test_attn_readout_host as rh

HOST_READOUT_CASES = [(64, 7, 3), (64, 16, 1), (128, 1, 1), (128, 7, 1)]
EVERY_16TH = range(0, ar.N, 16)                      # of the read-out batch's sequences
EVERY_8TH_LENGTH = list(range(0, ar.N, 8)) + [ar.N]  # of the length batch's; the last one is the empty sequence


def check_builder(mb, what):
    ref = mb.ref
    gap = rh.check_exact_inputs(ref)
    print(what, "smallest gap on the dequantized keys", gap)
    assert rh.v_rows_differ(ref)
    kc, ks, vc, vs = mb.mx
    cap = kc.shape[2]
    valid = (torch.arange(cap)[None, :] < ref.lens[:, None])[:, None, :, None]
    sel, sels = valid.expand_as(kc), valid.expand_as(ks)
    one = torch.tensor(127, dtype=torch.uint8)
    for codes, scales, want in ((kc, ks, ref.kc), (vc, vs, ref.vc)):
        assert torch.equal(mq.dequant(codes * sel, torch.where(sels, scales, one))[sel], want[sel])
        assert ((codes[~sel] & 0x7F) == 0x7F).all() and (scales[~sels] == 0xFF).all()
        assert not torch.isfinite(want.float()[~sel]).any()
    b = int(ref.lens.argmax())
    n = int(ref.lens[b])
    k_bytes, v_bytes = ks[b, :, :n].int(), vs[b, :, :n].int()
    assert (k_bytes[..., 1:] != k_bytes[..., :-1]).float().mean() > 0.9  # block j under 2^(j - 1): the bytes differ
    assert (v_bytes[..., 1:] != v_bytes[..., :-1]).all() and (n < 2 or (v_bytes[:, 1:] != v_bytes[:, :-1]).all())
    assert ((vc[sel] & 0x7F) != 0).all() and ((vc[sel] & 0x7F) != 0x7F).all()


def check_exact(mb, device, what):
    """f32 y == want bit for bit, the bf16 y its rounding; returns the f32 result."""
    y32, y16 = mq.run(mb, device), mq.run(mb, device, torch.bfloat16)
    ref = mb.ref
    got, want = ar.f32_bits(y32), np.ascontiguousarray(ref.want).view(np.uint32)
    bad = np.argwhere(got != want)
    if len(bad):
        b, i = bad[0]
        h, dd = divmod(int(i), ref.d)
        name = ref.names[b] if ref.names else ""
        raise AssertionError(f"{what} {name}: {len(bad)} of {got.size} elements differ, {len(set(bad[:, 0]))} sequences; first "
                             f"b {b} (len {int(ref.lens[b])}) head {h} d {dd}: got {y32[b, i].item()!r} want "
                             f"{ref.want[b, i]!r}, spikes {ref.spikes[b, h % ref.group].tolist()}")
    assert np.array_equal(ac.to_bits(y16), ac.to_bits(torch.from_numpy(ref.want).to(torch.bfloat16)))
    return y32


def test_cases_hold_every_d_group_and_kv_head_count():
    for cases in (mq.CASES, HOST_READOUT_CASES, mq.LENGTH_CASES):
        assert {c[0] for c in cases} == {64, 128} and {c[1] for c in cases} == {1, 7, 16} and {c[2] for c in cases} == {1, 3}
    assert len(mq.CASES) == 12


@pytest.mark.parametrize("case", HOST_READOUT_CASES, ids=ar.case_id)
@dp.one_thread
def test_readout_builder_and_cpu_route(case):
    mb = mq.to_mx(mq.sub(ar.readout(*case), EVERY_16TH), 3100)
    check_builder(mb, ar.case_id(case))
    check_exact(mb, "cpu", ar.case_id(case))


@pytest.mark.parametrize("case", mq.CASES, ids=ar.case_id)
@dp.one_thread
def test_tie_builder_and_cpu_route(case):
    mb = mq.ties(*case)
    check_builder(mb, ar.case_id(case))
    assert mb.ref.names == ar.TIE_NAMES and set(np.unique((mb.ref.spikes >= 0).sum(axis=2))) == {2, 4}
    check_exact(mb, "cpu", ar.case_id(case))


@pytest.mark.parametrize("front", [False, True], ids=["last", "front"])
@pytest.mark.parametrize("case", mq.LENGTH_CASES, ids=ar.case_id)
@dp.one_thread
def test_length_builder_and_cpu_route(case, front):
    mb = mq.to_mx(mq.sub(ar.lengths(*case, front), EVERY_8TH_LENGTH), 3300)
    assert mb.ref.lens.tolist() == [n + 1 for n in range(0, ar.N, 8)] + [0]
    check_builder(mb, ar.case_id(case))
    y = check_exact(mb, "cpu", ar.case_id(case))
    assert not ar.f32_bits(y[mb.ref.lens.tolist().index(0)]).any()
