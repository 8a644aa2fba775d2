"""attn_readout.py's exact read-outs for ops.attn_decode(k_scale=, v_scale=) (csrc/kernels/attn_decode_mxfp8.hip).
A plain module: test_attn_mxfp8_readout_host.py checks the builders on float64 and through the CPU route,
test_gpu_attn_mxfp8_readout.py runs the gfx950 kernel. test_gpu_attn_mxfp8.py spikes the chunk edges of random
sequences; here every position between them is read out, so that K's permutation of d, V's 8-byte loads and
the scale-byte address of every (position, 32-block) each decide a result's bits.

`to_mx` turns an attn_readout.Batch (`readout`, `lengths`, `ties`) into an MXFP8 one:
  keys   a position that the head slots H of a group read holds 64 times the SUM of their Hadamard rows (not
         attn_readout's sum of rows times 64 / 2^e, which is no e4m3 number for a group of 7 or 16): integers of
         at most 16 times 64, exact in e4m3 under one scale byte. Head slot s, q = 2^(s % 4 - 1) times its row,
         scores 2^(s % 4 - 1) 64 sqrt(d) natural units there (at least 256 at d 64) and exactly 0 on the other
         slots' rows. Every other key is the bf16 normal put through the host codec and back; the gap of 128 is
         asserted again on the dequantized values (test_attn_readout_host.check_exact_inputs);
  scales K's d-block j times 2^(j - 1) and q's times 2^(1 - j), as test_attn_mxfp8_host.sequence does: the scale
         bytes of a K row differ across blocks and every score is what it was;
  V      random e4m3 codes, never zero or NaN, under scale bytes that differ per (position, block)
         (attn_prefill_readout.mx_v; four byte values where rows are summed, so that the sum of 4 is exact in f32);
         no two dequantized V rows of a sequence are equal (asserted on the host);
  tail   NaN codes under scale bytes 0xFF behind every length.
The expectation is the dequantized V row at the spike, or the f32 sum over 2 or 4 of them over their number."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from distributed_llm_dissemination_amd import ops

import attn_readout as ar
from attn_prefill_readout import mx_v
from test_attn_mxfp8_host import dequant, quantize

DS, GROUPS, KVHS = (64, 128), (1, 7, 16), (1, 3)
CASES = [(d, g, kv) for d in DS for g in GROUPS for kv in KVHS]
LENGTH_CASES = [(64, 1, 3), (64, 16, 1), (128, 7, 1), (128, 16, 1)]


def sub(b, idx):
    """The sequences `idx` of an attn_readout.Batch as a batch of their own."""
    idx = list(idx)
    return ar.Batch(b.d, b.group, b.kvh, b.q[idx], b.kc[idx], b.vc[idx], b.lens[idx], b.spikes[idx], max_len=b.max_len,
                    names=tuple(b.names[i] for i in idx) if b.names else ())


@dataclass
class MxBatch:
    """ref: the attn_readout.Batch of the DEQUANTIZED caches (q with its blocks scaled, NaN and inf patterns
    behind the lengths, spikes, want); mx: (k codes, k scales, v codes, v scales) uint8."""
    ref: ar.Batch
    mx: tuple

    def only(self, i):
        r, sl = self.ref, slice(i, i + 1)
        return MxBatch(ar.Batch(r.d, r.group, r.kvh, r.q[sl], r.kc[sl], r.vc[sl], r.lens[sl], r.spikes[sl], r.want[sl]),
                       tuple(t[sl] for t in self.mx))


def run(mb, device="cpu", out_dtype=torch.float32):
    kc, ks, vc, vs = (t.contiguous().to(device) for t in mb.mx)
    return ops.attn_decode(mb.ref.q.to(device), kc, vc, mb.ref.lens.to(device), k_scale=ks, v_scale=vs,
                           max_len=mb.ref.max_len, out_dtype=out_dtype)


def to_mx(b, seed, spread=13):
    d, group, kvh = b.d, b.group, b.kvh
    nb, _, cap, _ = b.kc.shape
    rows = np.sign(ar.head_rows(d, group, kvh)[0])  # [heads, d]: the Hadamard row of every head
    scale = 2.0 ** (torch.arange(d) // 32 - 1)
    valid = (torch.arange(cap)[None, :] < b.lens[:, None])[:, None, :, None]
    k = b.kc.clone()
    flat = k.view(-1, d)
    bi, s, t = np.nonzero(b.spikes >= 0)
    pos = b.spikes[bi, s, t]
    spike_rows = []
    for kv in range(kvh):
        uniq, inv = np.unique((bi * kvh + kv) * cap + pos, return_inverse=True)
        acc = np.zeros((len(uniq), d))
        np.add.at(acc, inv, 64.0 * rows[kv * group + s])
        flat[torch.from_numpy(uniq)] = torch.from_numpy(acc).to(torch.bfloat16)
        spike_rows.append(torch.from_numpy(uniq))
    k = torch.where(valid, (k.float() * scale).to(torch.bfloat16), torch.zeros((), dtype=torch.bfloat16))
    kc, ks = quantize(k)
    kd = dequant(kc, ks)
    at = torch.cat(spike_rows)
    assert torch.equal(kd.view(-1, d)[at], k.view(-1, d)[at])  # the spike keys are e4m3 numbers under their bytes
    q = (b.q.float() * (1.0 / scale)).to(torch.bfloat16)
    assert torch.equal(q.float() * scale, b.q.float())
    gen = torch.Generator().manual_seed(seed)
    vc, vs = mx_v((1, kvh, cap, d), gen, spread)  # one draw for every sequence: rows differ within a sequence
    vc, vs = vc.expand(nb, -1, -1, -1), vs.expand(nb, -1, -1, -1)
    vd = dequant(vc[:1], vs[:1]).expand(nb, -1, -1, -1)
    nan = torch.where(torch.randint(0, 2, (1, kvh, cap, d), generator=gen) == 1, 0x7F, 0xFF).to(torch.uint8)
    ff = torch.tensor(0xFF, dtype=torch.uint8)
    mx = (torch.where(valid, kc, nan), torch.where(valid, ks, ff), torch.where(valid, vc, nan), torch.where(valid, vs, ff))
    shape = tuple(b.kc.shape)
    ref = ar.Batch(d, group, kvh, q, torch.where(valid, kd, ar.garbage_like(shape, seed + 1)),
                   torch.where(valid, vd, ar.garbage_like(shape, seed + 2)), b.lens, b.spikes, max_len=b.max_len,
                   names=b.names)
    r = ref.spike_rows().astype(np.float32)  # exact: bf16 values
    total = r[..., 0]
    for i in range(1, r.shape[3]):
        total = total + r[..., i]  # f32 arithmetic
    count = np.maximum((b.spikes >= 0).sum(axis=2), 1).astype(np.float32)
    ref.want = (total / np.tile(count, (1, kvh))[:, :, None]).reshape(nb, -1)
    return MxBatch(ref, mx)


@functools.lru_cache(maxsize=1)
def readout(d, group, kvh):
    return to_mx(ar.readout(d, group, kvh), 3100 + d + group)


@functools.lru_cache(maxsize=None)
def ties(d, group, kvh):
    return to_mx(ar.ties(d, group, kvh), 3200 + d + group, spread=4)


@functools.lru_cache(maxsize=1)
def lengths(d, group, kvh, front):
    return to_mx(ar.lengths(d, group, kvh, front), 3300 + d + group + int(front))
