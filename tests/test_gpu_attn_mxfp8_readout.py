"""ops.attn_decode(k_scale=, v_scale=) on the GPU (csrc/kernels/attn_decode_mxfp8.hip) on attn_readout.py's exact
read-outs, put into an MXFP8 cache by attn_mxfp8_readout.py. test_gpu_attn_mxfp8.py spikes the chunk edges of random
sequences; here every position between them is read out, so that K's permutation of d, V's 8-byte loads and
the scale-byte address of every (position, 32-block) each decide a result's bits. d 64 and 128, groups 1, 7 and
16, 1 and 3 KV heads; NaN codes under scale bytes 0xFF behind every length.

1. One-hot read-out of every (head slot, position) of 2 C + 3 sequences of 2 C + 3 positions: f32 y[b, h] is the
   dequantized V row at the head's spike position bit for bit, the bf16 result its rounding.
2. attn_readout's ties of 2 and 4 equally scored keys (one lane, lane groups, the steps of a wave, waves, chunks):
   the f32 sum of the dequantized V rows over their number, one launch per class and all as one.
3. Every length 0 .. 2 C + 3 in one batch, the spike at the last valid position and at position 0; the empty row
   is zero."""
import pytest

import attn_mxfp8_readout as mq
import attn_readout as ar
import test_attn_mxfp8_readout_host as host

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", mq.CASES, ids=ar.case_id)
def test_every_position_and_head_slot_reads_its_dequantized_v_row(gpu, case):
    host.check_exact(mq.readout(*case), "cuda", ar.case_id(case))


@pytest.mark.parametrize("case", mq.CASES, ids=ar.case_id)
def test_ties_merge_exactly(gpu, case):
    mb = mq.ties(*case)
    for i, name in enumerate(mb.ref.names):  # per class, so that a failure names the merge
        host.check_exact(mb.only(i), "cuda", f"{ar.case_id(case)} {name}")
    host.check_exact(mb, "cuda", ar.case_id(case))  # and as one launch


@pytest.mark.parametrize("front", [False, True], ids=["last", "front"])
@pytest.mark.parametrize("case", mq.LENGTH_CASES, ids=ar.case_id)
def test_every_length_reads_its_spike(gpu, case, front):
    mb = mq.lengths(*case, front)
    y = host.check_exact(mb, "cuda", ar.case_id(case))
    assert not ar.f32_bits(y[mb.ref.lens.tolist().index(0)]).any()
