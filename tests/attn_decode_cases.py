"""Case builders, the float64 reference, the bound and the mistakes for ops.attn_decode and
ops.rope_append (csrc/kernels/attn_decode.hip). A plain module: test_attn_decode_host.py checks what
rests on the reference alone and runs the ops' CPU routes, test_gpu_attn_decode.py runs the gfx950
kernels.

A case is a head_dim d in {32, 64, 128} and a group (query heads per KV head) in {1, 2, 4, 8, 16}, with
2 KV heads, and one sequence per length in LENGTHS = (1, 2, C - 1, C, C + 1, 2 C + 3, 0), C =
_core.attn_decode_chunk(): every way a length can meet a chunk edge, two full chunks and a tail, and
the empty sequence. The sequences are used alone and as the slots of one mixed batch.

  q, K, V   seeded bf16 standard normals;
  spikes    the keys at positions 0, len - 1 and the first and last position of every chunk are
            replaced by 8 sqrt(d) q_h / |q_h|^2 for a query head h of the group, rotating through the
            heads: q_h . k / sqrt(d) = 8 there, so each boundary position carries a softmax weight of
            at least 0.1 in one head (asserted on the reference). Without them a lost position of 515
            weighs 1/515 and no bound could see it;
  garbage   every cache position at or behind the length holds the bit patterns of NaN and +-inf;
  y64       float64 from the definition: y = sum_j p_j v_j, p = softmax(q . k_j / sqrt(d)) over the
            valid prefix; a length of 0 gives zeros;
  bound     per element, for an f32 result: 2^-7 sum_j p_j |v_j|. A bf16 p_j carries a relative
            rounding error of 2^-9, the normalisation the same again: 2^-8 to first order; the factor
            2 covers second-order terms and the f32 score and exp errors. For a bf16 result
            2^-9 |y64| is added (one more rounding).

The mistakes a kernel of this decomposition can make, each as the float64 reference with that
mistake: drop_first, drop_last (position 0 or len - 1 lost; len > 1), drop_chunk_edge (position C
lost; len > C), head_swap (the query heads of a group rotated by one; group > 1, len > 1) and no_scale (the
1 / sqrt(d) omitted; visible from len >= C - 1). test_attn_decode_host.py asserts how many bounds
away each lies."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from distributed_llm_dissemination_amd import _core

C = _core.attn_decode_chunk()
DS = (32, 64, 128)
GROUPS = (1, 2, 4, 8, 16)
KV_HEADS = 2
LENGTHS = (1, 2, C - 1, C, C + 1, 2 * C + 3, 0)
CAPACITY = 2 * C + 8  # no multiple of the chunk: the last chunk ends behind the cache
CASES = [(d, g) for d in DS for g in GROUPS]
MISTAKES = ("drop_first", "drop_last", "drop_chunk_edge", "head_swap", "no_scale")
GARBAGE = np.array([0x7FC0, 0x7F80, 0xFF80, 0xFFFF, 0x7FA5], dtype=np.uint16)  # NaN, +inf, -inf, NaN, NaN


def case_id(c):
    return f"d{c[0]}-g{c[1]}"


def bits_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def to_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def f64(t):
    return bits_to_f64(to_bits(t)).reshape(tuple(t.shape))


def boundary_positions(n):
    """Positions 0, n - 1 and the first and last position of every chunk, below n, ascending."""
    pos = {0, n - 1}
    for c0 in range(0, n, C):
        pos.add(c0)
        if c0 + C - 1 < n:
            pos.add(c0 + C - 1)
    return sorted(p for p in pos if 0 <= p < n)


@dataclass
class Seq:
    """One sequence: q bf16 [heads, d], k and v bf16 [KV_HEADS, n, d] and what the reference gives."""
    d: int
    group: int
    n: int
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    spike_head: dict      # {(kv head, position): query head that the key there is made for}
    y64: np.ndarray       # [heads * d]
    bound: np.ndarray     # [heads * d], for an f32 result
    p: np.ndarray         # [heads, n] softmax weights

    @property
    def heads(self):
        return KV_HEADS * self.group

    def bound_bf16(self):
        return self.bound + 2.0 ** -9 * np.abs(self.y64)


def reference(q, k, v, group, mistake=None):
    """(y64 [heads * d], bound [heads * d], p [heads, n]) in float64 from float64 q [heads, d] and
    k, v [kv heads, n, d]; `mistake`: one of MISTAKES."""
    heads, d = q.shape
    n = k.shape[1]
    y, bound, p_all = np.zeros((heads, d)), np.zeros((heads, d)), np.zeros((heads, n))
    if n == 0:
        return y.reshape(-1), bound.reshape(-1), p_all
    keep = np.ones(n, dtype=bool)
    if mistake == "drop_first":
        keep[0] = False
    elif mistake == "drop_last":
        keep[n - 1] = False
    elif mistake == "drop_chunk_edge":
        keep[C] = False
    for h in range(heads):
        kv = h // group
        qh = q[kv * group + (h % group + 1) % group] if mistake == "head_swap" else q[h]
        s = k[kv] @ qh
        if mistake != "no_scale":
            s = s / np.sqrt(d)
        s = np.where(keep, s, -np.inf)
        e = np.exp(s - s.max())
        p = e / e.sum()
        y[h] = p @ v[kv]
        bound[h] = 2.0 ** -7 * (p @ np.abs(v[kv]))
        p_all[h] = p
    return y.reshape(-1), bound.reshape(-1), p_all


def applies(mistake, seq):
    if mistake in ("drop_first", "drop_last"):
        return seq.n > 1
    if mistake == "drop_chunk_edge":
        return seq.n > C
    if mistake == "head_swap":
        return seq.group > 1 and seq.n > 1  # over one key the softmax is 1 whatever q holds
    return seq.n >= C - 1  # no_scale


def mistaken(seq, mistake):
    return reference(f64(seq.q), f64(seq.k), f64(seq.v), seq.group, mistake)[0]


@functools.lru_cache(maxsize=None)
def sequence(d, group, n, seed=0):
    g = torch.Generator().manual_seed(1000 * d + 10 * group + 7919 * n + seed)
    heads = KV_HEADS * group
    q = torch.randn(heads, d, generator=g).to(torch.bfloat16)
    k = torch.randn(KV_HEADS, n, d, generator=g).to(torch.bfloat16)
    v = torch.randn(KV_HEADS, n, d, generator=g).to(torch.bfloat16)
    spike_head = {}
    for kv in range(KV_HEADS):
        for i, pos in enumerate(boundary_positions(n)):
            h = kv * group + i % group
            qh = q[h].double()
            k[kv, pos] = (8.0 * d ** 0.5 * qh / (qh * qh).sum()).to(torch.bfloat16)
            spike_head[(kv, pos)] = h
    y64, bound, p = reference(f64(q), f64(k), f64(v), group)
    return Seq(d, group, n, q, k, v, spike_head, y64, bound, p)


def sequences(d, group):
    """The case's sequences, one per length of LENGTHS, in that order."""
    return [sequence(d, group, n) for n in LENGTHS]


def garbage(shape, seed):
    """bf16 tensor of NaN and +-inf bit patterns."""
    rng = np.random.default_rng(seed)
    return from_bits(GARBAGE[rng.integers(0, len(GARBAGE), size=int(np.prod(shape)))]).view(*shape)


def caches(seqs, capacity=CAPACITY, seed=1):
    """(q [B, heads, d], k_cache, v_cache [B, KV_HEADS, capacity, d], lens int32 [B]) on the CPU for
    the sequences as the slots of one batch; everything at or behind a length is garbage."""
    d = seqs[0].d
    shape = (len(seqs), KV_HEADS, capacity, d)
    kc, vc = garbage(shape, seed), garbage(shape, seed + 1)
    for b, s in enumerate(seqs):
        kc[b, :, : s.n] = s.k
        vc[b, :, : s.n] = s.v
    q = torch.stack([s.q for s in seqs])
    return q, kc, vc, torch.tensor([s.n for s in seqs], dtype=torch.int32)


def err_over_bound(y, seqs, bf16):
    """Worst |y - y64| / bound over the batch rows of y [B, heads * d] (f32 or bf16 tensor);
    asserts no NaN and an exactly zero row for a length of 0."""
    got = y.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    worst = 0.0
    for b, s in enumerate(seqs):
        if s.n == 0:
            assert not got[b].any()
            continue
        bound = s.bound_bf16() if bf16 else s.bound
        assert (bound > 0).all()
        worst = max(worst, float((np.abs(got[b] - s.y64) / bound).max()))
    return worst
