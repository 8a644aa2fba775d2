"""Hand-made operands for ops.attn_prefill (csrc/kernels/attn_prefill.hip, attn_prefill_mxfp8.hip): inputs
whose result is known exactly, a float64 model of the kernel's decomposition, and the mistakes that
decomposition can make. A plain module: test_attn_prefill_readout_host.py checks what rests on float64
alone and runs the builders through the op's CPU route, test_gpu_attn_prefill_extremes.py runs the gfx950
kernels. test_attn_prefill_host.py marks one key per position for the row whose diagonal it is and sees
nothing of what any other row does with it; here every row reads one position out of all it may see.

The causal one-hot construction (`build`). Position j of KV head kv holds ONE key: row (cls[j] + 11 kv) mod d
of the +-1 Hadamard matrix of order d times 64 mult[j] 2^k_exp, mult a signed integer of at most 4 bits -
exact in bf16, and in e4m3 under one scale byte. Row i, head slot s of KV head kv asks for the class rho of
one position `pick` that it sees: its q is Hadamard row (rho + 11 kv) mod d times 2^(s % 4 - 1 + q_exp). Keys of
another class score exactly 0 (the rows are orthogonal and every partial sum is an integer times a power of
two), keys of its own class 2^(s % 4 - 1 + q_exp + k_exp) 64 sqrt(d) mult natural units: multiples of a unit of
at least 32 sqrt(32) = 181 > GAP. So the (row, head) reads the visible positions of its class with the
largest mult - asserted positive - with weight exactly 1 in f32 (every other exp2 argument is below -149, every
rescale factor 0 or 1, whatever the MFMA's rounding): y is the V row there bit for bit, or for T positions
of equal key bits their f32 sum over T, exact for T = 2 and 4.

Layouts. `onehot`: cls = j mod d, pick = (7 i + 3 s + 5 kv + 1) mod min(d, start + i + 1), mult a function of
j // d: "near" rises (every row reads within d of its diagonal, at every offset), "far" falls (every row
reads inside [0, d): the maximum in the first step, then alpha = 1 and p = 0), "mid" peaks at the middle block
(alpha = 0 once, then 1). `ties` merges offsets of a block of W positions into one class (TIE_CLASSES).

`emulate` is the kernel's decomposition in float64 - query tiles of BQ, waves of 32 rows, 32-position steps
at absolute positions inside tiles of BK, the diagonal mask, the step skip, the online rescale, the division
by l - and takes one of MISTAKES. Without one it is test_attn_prefill_host.reference to rounding."""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from distributed_llm_dissemination_amd import _core, ops

import attn_decode_cases as ac
from attn_readout import GAP, differs, f32_bits, garbage_like, hadamard, ordinary_v, subnormal_v  # noqa: F401
from test_attn_mxfp8_host import dequant, quantize
from test_attn_prefill_host import reference

BQ, BK = _core.attn_prefill_tiles()
STEP, WAVES = 32, BQ // 32
STARTS = (0, 1, BK - 1, BK, BK + 5)
VARIANTS = ("near", "far", "mid")
SHAPES = [(32, 3, 1), (32, 16, 3), (64, 7, 2), (128, 1, 1), (128, 5, 3), (128, 12, 1)]
SIZES = (1, 31, 33, BQ - 1, BQ, BQ + 1, 2 * BQ, 2 * BQ + 3)
# (d, group, KV heads, S, T): "pad" max(start) + S + 3, "end" max(start) + S, "bk" the next multiple of BK
READOUT_CASES = [(32, 3, 1, 2 * BQ + 3, "pad"), (32, 3, 1, 1, "pad"), (32, 16, 3, BQ + 1, "pad"), (64, 7, 2, 2 * BQ, "bk"),
                 (64, 7, 2, 31, "pad"), (128, 1, 1, BQ, "end"), (128, 5, 3, BQ - 1, "pad"), (128, 12, 1, 33, "pad")]
START_CASES = [(32, 16, 1), (128, 1, 1)]
START_S = 35  # two waves, the second of three rows
TIE_SHAPES = [(32, 3, 1), (64, 7, 2), (128, 12, 1)]
STAIR_CASES = [(32, 5), (64, 7), (128, 16)]  # (d, group), 2 KV heads
STAIR_VARIANTS = ("rising", "falling", "rising120", "diagonal")
EXTREME_SHAPES = [(32, 5, 1), (128, 16, 3)]
EXT_START, EXT_S = BK + 5, BQ + 1
MISTAKES = ("mask_late", "mask_early", "mask_block0", "skip_early", "tile_short", "stale_buffer", "v_row_swap",
            "k_piece", "tile_order", "kv_head_mod", "tail_loaded", "start_dropped", "no_rescale_o", "no_rescale_l")


def case_id(c):
    return "d%d-g%d-kv%d" % tuple(c[:3]) + "".join("-%s" % x for x in c[3:])


def t_len(s, rule, starts=STARTS):
    n = max(starts) + s
    return {"pad": n + 3, "end": n, "bk": -(-n // BK) * BK}[rule]


@dataclass
class Batch:
    """One launch: q bf16 [B, S, heads, d], k and v bf16 [B, kvh, T, d] (of an MXFP8 batch the dequantized
    values, with bf16 NaN and inf patterns as its tail), start int32 [B]; mx (k codes, k scales, v codes, v scales)
    or None; read int [B, S, heads, 4] (the positions a (row, head) reads, -1: none) and want f32 [B, S, heads * d]."""
    d: int
    group: int
    kvh: int
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    start: torch.Tensor
    mx: Optional[tuple] = None
    read: Optional[np.ndarray] = None
    want: Optional[np.ndarray] = None
    unit: float = 0.0
    names: tuple = ()

    @property
    def heads(self):
        return self.kvh * self.group

    @property
    def s(self):
        return self.q.shape[1]

    def ends(self):
        return [min(int(st) + self.s, self.k.shape[2]) for st in self.start.tolist()]

    def only(self, b):
        """Sequence b as a batch of its own."""
        sl = slice(b, b + 1)
        mx = None if self.mx is None else tuple(t[sl] for t in self.mx)
        return Batch(self.d, self.group, self.kvh, self.q[sl], self.k[sl], self.v[sl], self.start[sl], mx,
                     self.read[sl], self.want[sl], self.unit, self.names[sl])


def run(batch, device="cpu", out_dtype=torch.float32, mx=None, t_cut=None):
    """ops.attn_prefill of the batch; mx: through the MXFP8 cache (default: where the batch has one); t_cut: T."""
    mx = batch.mx is not None if mx is None else mx
    cut = lambda t: (t if t_cut is None else t[:, :, :t_cut]).contiguous().to(device)  # noqa: E731
    q, start = batch.q.to(device), batch.start.to(device)
    if mx:
        kc, ks, vc, vs = (cut(t) for t in batch.mx)
        return ops.attn_prefill(q, kc, vc, start, k_scale=ks, v_scale=vs, out_dtype=out_dtype)
    return ops.attn_prefill(q, cut(batch.k), cut(batch.v), start, out_dtype=out_dtype)


def mx_v(shape, gen, spread=13):
    """(codes, scale bytes) of a random MXFP8 V: e4m3 codes of both signs, never zero or NaN (low 7 bits 1 .. 126),
    under scale bytes 120 .. 119 + spread that differ per (position, 32-block): (5 position + 3 block + 7 KV head) mod
    spread. With a spread of 4 every value is a multiple of 2^-16 of at most 448 2^-4 = 28, so a sum of four has 23 bits: exact in f32
    (`build` asserts it)."""
    codes = ((torch.randint(0, 2, shape, generator=gen) << 7) | torch.randint(1, 127, shape, generator=gen)).to(torch.uint8)
    _, kvh, t, d = shape
    byte = 120 + (5 * torch.arange(t)[None, :, None] + 3 * torch.arange(d // 32)[None, None, :]
                  + 7 * torch.arange(kvh)[:, None, None]) % spread
    return codes, byte.to(torch.uint8)[None].expand(shape[0], -1, -1, -1).contiguous()


def build(d, group, kvh, s, starts, t, cls, mult, pick, seed, q_exp=0, k_exp=0, v_draw=ordinary_v, mx=False, names=(),
          mx_spread=13):
    """The construction of the module docstring: cls, mult int [B, T], pick int [B, S, kvh, group]."""
    starts = np.asarray(starts, dtype=np.int64)
    nb, heads = len(starts), kvh * group
    cls, mult = np.broadcast_to(cls, (nb, t)), np.broadcast_to(mult, (nb, t))
    assert (np.abs(mult) <= 15).all() and (mult != 0).all() and cls.min() >= 0 and cls.max() < d
    had = hadamard(d)
    pos = starts[:, None] + np.arange(s)[None, :]                                   # [B, S]
    assert pick.shape == (nb, s, kvh, group) and (pick >= 0).all() and (pick <= pos[:, :, None, None]).all()
    kvs = np.arange(kvh)
    k64 = had[(cls[:, None, :] + 11 * kvs[None, :, None]) % d] * (64.0 * 2.0 ** k_exp * mult[:, None, :, None])
    rho = cls[np.arange(nb)[:, None, None, None], pick]                             # [B, S, kvh, group]
    q64 = had[(rho + 11 * kvs[None, None, :, None]) % d] * 2.0 ** (np.arange(group) % 4 - 1 + q_exp)[None, None, None, :, None]
    q = torch.from_numpy(q64.reshape(nb, s, heads, d)).to(torch.bfloat16)
    k = torch.from_numpy(k64).to(torch.bfloat16)
    assert np.array_equal(ac.f64(q).reshape(q64.shape), q64) and np.array_equal(ac.f64(k), k64)
    gen = torch.Generator().manual_seed(seed)
    shape = (nb, kvh, t, d)
    valid = (torch.arange(t)[None, :] < torch.from_numpy(np.minimum(starts + s, t))[:, None])[:, None, :, None]
    codes = None
    if mx:
        kc, ks = quantize(torch.where(valid, k, torch.zeros((), dtype=torch.bfloat16)))
        assert torch.equal(torch.where(valid, dequant(kc, ks), k), k)  # exact in e4m3 under its scale byte
        vc, vs = mx_v(shape, gen, mx_spread)
        v = dequant(vc, vs)
        nan = torch.where(torch.randint(0, 2, shape, generator=gen) == 1, 0x7F, 0xFF).to(torch.uint8)
        codes = (torch.where(valid, kc, nan), torch.where(valid[..., :1], ks, torch.tensor(0xFF, dtype=torch.uint8)),
                 torch.where(valid, vc, nan), torch.where(valid[..., :1], vs, torch.tensor(0xFF, dtype=torch.uint8)))
    else:
        v = v_draw(shape, gen)
    k = torch.where(valid, k, garbage_like(shape, seed + 1))
    v = torch.where(valid, v, garbage_like(shape, seed + 2))
    # what each (row, head) reads: the visible positions of its class with the largest mult
    j = np.arange(t)
    match = (cls[:, None, None, None, :] == rho[..., None]) & (j <= pos[:, :, None, None, None])  # [B, S, kvh, g, T]
    m = np.where(match, mult.astype(np.int8)[:, None, None, None, :], np.int8(-99))
    top = m.max(axis=-1)
    assert (top >= 1).all()  # positions of other classes score 0: the read score lies a unit above them
    tie = (m == top[..., None]).reshape(nb, s, heads, t)
    count = tie.sum(axis=-1)
    assert np.isin(count, (1, 2, 4)).all()
    read = -np.ones((nb, s, heads, 4), dtype=np.int64)
    v32 = ac.f64(v).astype(np.float32)                                              # [B, kvh, T, d], exact
    bi, hi = np.arange(nb)[:, None, None], (np.arange(heads) // group)[None, None, :]
    total, left = np.zeros((nb, s, heads, d), dtype=np.float32), tie.copy()
    total64 = np.zeros((nb, s, heads, d))
    for n in range(4):
        first = left.argmax(axis=-1)
        has = np.take_along_axis(left, first[..., None], -1)[..., 0]
        read[..., n] = np.where(has, first, -1)
        total = total + np.where(has[..., None], v32[bi, hi, first], np.float32(0))  # f32 arithmetic
        total64 = total64 + np.where(has[..., None], v32[bi, hi, first], np.float32(0))
        np.put_along_axis(left, first[..., None], False, -1)
    assert np.array_equal(total.astype(np.float64), total64)  # the sum is an f32 number, in whatever order it is taken
    want = (total / count[..., None].astype(np.float32)).reshape(nb, s, heads * d)
    beyond = pos >= t  # rows whose position is >= T: zero rows
    want[beyond] = 0
    return Batch(d, group, kvh, q, k, v, torch.from_numpy(starts).to(torch.int32), codes, read, want,
                 2.0 ** (-1 + q_exp + k_exp) * 64 * np.sqrt(d), tuple(names))


def std_pick(s, starts, kvh, group, w):
    """(7 i + 3 s + 5 kv + 1) mod min(w, start + i + 1): a position every (row, head) sees, [B, S, kvh, group]."""
    i = np.arange(s)[None, :, None, None]
    st = np.asarray(starts)[:, None, None, None]
    return (7 * i + 3 * np.arange(group)[None, None, None, :] + 5 * np.arange(kvh)[None, None, :, None] + 1) % np.minimum(w, st + i + 1)


def block_mult(variant, nblk):
    """mult of block 0 .. nblk - 1: distinct, 1 .. nblk."""
    b = np.arange(nblk)
    if variant == "near":
        return b + 1
    if variant == "far":
        return nblk - b
    mid = nblk // 2  # "mid": the nearer to the middle block the larger, a block before it above the one behind
    order = sorted(b, key=lambda x: (abs(x - mid), x > mid))
    out = np.empty(nblk, dtype=np.int64)
    out[order] = nblk - np.arange(nblk)
    return out


# ---------------------------------------------------------------- 1. causal one-hot read-outs, 2. every start

@functools.lru_cache(maxsize=48)
def onehot(d, group, kvh, s, t, variant, starts=STARTS, mx=False, q_exp=0, k_exp=0, subnormal=False, signed=False):
    j = np.arange(t)
    mult = block_mult(variant, -(-t // d))[j // d]
    if signed:  # every other block negative: scores of both signs
        mult = np.where((j // d) % 2 == 0, mult, -mult)
    pick = std_pick(s, starts, kvh, group, d)
    seed = 1000 + 10 * d + group + 7 * s + VARIANTS.index(variant)
    return build(d, group, kvh, s, starts, t, j % d, mult, pick, seed, q_exp, k_exp,
                 subnormal_v if subnormal else ordinary_v, mx)


def readout(case, variant, mx=False):
    d, group, kvh, s, rule = case
    return onehot(d, group, kvh, s, t_len(s, rule), variant, mx=mx)


EVERY_START = tuple(range(2 * BK + 2))


def every_start(shape, variant, mx=False):
    d, group, kvh = shape
    return onehot(d, group, kvh, START_S, t_len(START_S, "pad", EVERY_START), variant, starts=EVERY_START, mx=mx)


# ---------------------------------------------------------------- 3. ties

def _orbits(w, xs):
    """Class of each offset 0 .. w - 1 when offsets that differ by an XOR of `xs` are one class."""
    group = {0}
    for x in xs:
        group |= {e ^ x for e in group}
    rep = np.min([np.arange(w) ^ e for e in group], axis=0)
    return np.unique(rep, return_inverse=True)[1]


def tie_classes(d):
    """{name: (W, xors, pick, tile0)}: offsets of a block of W positions that differ by an XOR of `xors` hold equal
    key bits (mult rises with j // W); pick "std" or "diag" (the class of the row's own position); tile0: the
    positions of tile 0 and of the first block get the mult of the block of the sequence's middle row instead."""
    return {
        "one lane": (d, (1,), "std", False),
        "two lane groups": (d, (4,), "std", False),
        "all four lane groups": (d, (4, 8), "std", False),
        "two halves of a tile": (max(d, BK), (32,), "std", False),
        "two tiles in different LDS buffers": (2 * BK, (BK,), "std", False),
        "tile 0 and the diagonal step": (d, (), "std", True),
        "the diagonal and its predecessor": (d, (1,), "diag", False),
    }


TIE_NAMES = tuple(tie_classes(32))


@functools.lru_cache(maxsize=None)
def ties(d, group, kvh, mx=False):
    """One sequence per tie class, S = BQ + 1 rows behind start = BK + 5."""
    s, st = EXT_S, EXT_START
    t = st + s + 3
    j = np.arange(t)
    cls, mult, pick = [], [], []
    pos = st + np.arange(s)[:, None, None]
    for name, (w, xors, how, tile0) in tie_classes(d).items():
        c = _orbits(w, xors)[j % w]
        m = j // w + 1
        if c.max() >= d:  # more classes than Hadamard rows (d 32, offsets o and o ^ 64 of 128): the odd 32-position
            c, m = (j % w) % 32, np.where((j % w) // 32 % 2 == 1, -m, m)  # steps hold keys nobody reads (mult < 0)
        if tile0:
            m = np.where(j < min(d, BK), (st + s // 2) // w + 1, m)
        cls.append(c), mult.append(m)
        sel = std_pick(s, [st], kvh, group, w)[0]
        if how == "diag":
            sel = np.broadcast_to(pos, sel.shape).copy()
        for _ in range(2 * STEP):  # three of four tied positions seen (the diagonal cuts the four): ask one earlier
            hit = (c[None, None, None, :] == c[sel][..., None]) & (j <= pos[..., None])
            mm = np.where(hit, m, -99)
            bad = (mm == mm.max(axis=-1, keepdims=True)).sum(axis=-1) == 3
            if not bad.any():
                break
            sel = np.where(bad, (sel - 1) % (pos + 1), sel)
        pick.append(sel)
    return build(d, group, kvh, s, [st] * len(TIE_NAMES), t, np.stack(cls), np.stack(mult), np.stack(pick),
                 2000 + d + group, mx=mx, names=TIE_NAMES, mx_spread=4)


# ---------------------------------------------------------------- the kernel's decomposition in float64

def emulate(q, k, v, start, group, mistake=None):
    """y float64 [B, S, heads * d] from float64 q [B, S, heads, d] and the whole caches k, v [B, kvh, T, d], tail
    included, computed as the kernel decomposes it, with one of MISTAKES:
      mask_late      the mask lets prow + 1 through
      mask_early     the diagonal itself is masked
      mask_block0    column block 1 (rows 16 .. 31 of a wave) masked by block 0's row positions
      skip_early     a step skipped when p0 > wpos0 rather than wpos0 + 31
      tile_short     ntiles one short when the last row is the first position of a tile
      stale_buffer   odd tiles read the previous tile's K and V
      v_row_swap     V rows p and p ^ 1 of a tile exchanged
      k_piece        16-byte pieces c and c ^ 1 of a K row exchanged
      tile_order     query tiles not reversed when written
      kv_head_mod    KV head taken as h % kv_heads
      tail_loaded    positions in [start + S, T) loaded
      start_dropped  a row's position taken as i
      no_rescale_o / no_rescale_l   the online softmax's alpha not applied to o / to l"""
    nb, s, heads, d = q.shape
    kvh, t = k.shape[1], k.shape[2]
    tp = -(-t // BK) * BK
    nqt = -(-s // BQ)
    hk = np.arange(heads) % kvh if mistake == "kv_head_mod" else np.arange(heads) // group
    y = np.zeros((nb, s, heads, d))
    with np.errstate(all="ignore"):
        for b in range(nb):
            st = min(max(int(start[b]), 0), t)
            kv_end = min(st + s, t)
            kk, vv = np.zeros((kvh, tp, d)), np.zeros((kvh, tp, d))
            end = t if mistake == "tail_loaded" else kv_end
            kk[:, :end], vv[:, :end] = k[b, :, :end], v[b, :, :end]
            if mistake == "k_piece":
                kk = kk[:, :, np.arange(d) ^ 8]
            elif mistake == "v_row_swap":
                vv = vv[:, np.arange(tp) ^ 1]
            elif mistake == "stale_buffer":
                src = np.arange(tp)
                src = np.where((src // BK) % 2 == 1, src - BK, src)
                kk, vv = kk[:, src], vv[:, src]
            kh, vh = kk[hk], vv[hk]  # [heads, tp, d]
            for qt in range(nqt):
                q0 = qt * BQ
                rows = min(s - q0, BQ)
                pos0 = (0 if mistake == "start_dropped" else st) + q0
                pos_end = min(pos0 + rows, t)
                ntiles = (pos_end - 1) // BK + 1 if pos_end > pos0 else 0
                if mistake == "tile_short" and pos_end > pos0 and (pos_end - 1) % BK == 0:
                    ntiles -= 1
                out0 = (nqt - 1 - qt) * BQ if mistake == "tile_order" else q0
                for w in range(WAVES):
                    iq = 32 * w + np.arange(32)
                    prow = pos0 + iq
                    rvalid = (iq < rows) & (prow < t)
                    wpos0 = pos0 + 32 * w
                    if not rvalid.any():
                        continue
                    qw = np.zeros((heads, 32, d))
                    qw[:, rvalid] = q[b, q0 + iq[rvalid]].transpose(1, 0, 2)
                    mrow = prow + 1 if mistake == "mask_late" else (prow - 1 if mistake == "mask_early" else prow)
                    if mistake == "mask_block0":
                        mrow = np.concatenate([prow[:16], prow[:16]])
                    m, l, o = np.full((heads, 32), -np.inf), np.zeros((heads, 32)), np.zeros((heads, 32, d))
                    for p0 in range(0, ntiles * BK, STEP):
                        if p0 > wpos0 + (0 if mistake == "skip_early" else 31):
                            continue
                        pos = p0 + np.arange(STEP)
                        sc = qw @ kh[:, pos].transpose(0, 2, 1) / np.sqrt(d)
                        sc = np.where((pos[None, :] > mrow[:, None])[None], -np.inf, sc)
                        m_new = np.maximum(m, sc.max(axis=-1))
                        alpha = np.exp(m - m_new)
                        p = np.exp(sc - m_new[..., None])
                        l = l * (1.0 if mistake == "no_rescale_l" else alpha) + p.sum(axis=-1)
                        o = o * (1.0 if mistake == "no_rescale_o" else alpha[..., None]) + p @ vh[:, pos]
                        m = m_new
                    res = np.where(rvalid[None, :, None], o / l[..., None], 0.0)
                    ok = (iq < rows) & (out0 + iq < s)
                    y[b, out0 + iq[ok]] = res[:, ok].transpose(1, 0, 2)
    return y.reshape(nb, s, heads * d)


def emulate_batch(batch, mistake=None):
    return emulate(ac.f64(batch.q), ac.f64(batch.k), ac.f64(batch.v), batch.start.tolist(), batch.group, mistake)


def exact_scores(batch, b):
    """(tie [S, heads, n] bool, gap [S, heads]) of sequence b from the tensors alone, in float64: the visible
    positions whose score is the row's largest, and how far below it the next score lies (inf: none)."""
    n, st = batch.ends()[b], int(batch.start[b])
    q, k = ac.f64(batch.q[b]), ac.f64(batch.k[b, :, :n])
    sc = q.transpose(1, 0, 2) @ k[np.arange(batch.heads) // batch.group].transpose(0, 2, 1) / np.sqrt(batch.d)  # [heads, S, n]
    sc = np.where((np.arange(n)[None, :] <= (st + np.arange(batch.s))[:, None])[None], sc, -np.inf).transpose(1, 0, 2)
    top = sc.max(axis=-1, keepdims=True)
    tie = sc == top
    return tie, (top[..., 0] - np.where(tie, -np.inf, sc).max(axis=-1))


# ---------------------------------------------------------------- 4. the order of the maxima

@dataclass
class Approx:
    """A batch held to float64: y64 and bound [B, S, heads * d] (for an f32 result; bf16: 2^-9 |y64| more)."""
    batch: Batch
    y64: np.ndarray
    bound: np.ndarray


def _with_reference(batch):
    y64, bound, _ = reference(batch.q, batch.k, batch.v, batch.start.tolist())
    return Approx(batch, y64, bound)


def _tail(x, start, s, seed):
    t = x.shape[2]
    valid = (torch.arange(t)[None, :] < (torch.as_tensor(start) + s)[:, None])[:, None, :, None]
    return torch.where(valid, x, garbage_like(x.shape, seed))


@functools.lru_cache(maxsize=None)
def staircase(d, group, variant):
    """Ordinary random q, K, V (2 KV heads), one sequence of S = BQ + 1 rows behind start = BK + 5. Every q row
    carries the same component along one Hadamard row u of its KV head (q = n - (n . u) u / d + u, n normal), and
    the key at offset (5 t + 3) mod 32 of 32-position step t is score_t u / sqrt(d): every row that sees it scores
    score_t there (before the roundings to bf16; the reference takes the rounded values): 6 + 3 t "rising",
    falling by 3, 6 + 120 t "rising120" (every alpha underflows to 0), and 6 throughout for "diagonal", where the
    key of every other position j >= start is 14 sqrt(d) q / |q|^2 for the q of row j - start and head j mod group:
    that row's maximum lies in its own diagonal step."""
    kvh, s, st = 2, EXT_S, EXT_START
    t, heads = st + s + 3, 2 * group
    g = torch.Generator().manual_seed(4000 + 100 * d + group)
    had = torch.from_numpy(hadamard(d)).float()
    u = had[[3, 9]].repeat_interleave(group, 0)  # [heads, d]
    n = torch.randn(1, s, heads, d, generator=g)
    q = (n - (n * u).sum(-1, keepdim=True) * u / d + u).to(torch.bfloat16)
    k = torch.randn(1, kvh, t, d, generator=g).to(torch.bfloat16)
    v = torch.randn(1, kvh, t, d, generator=g).to(torch.bfloat16)
    steps = -(-(st + s) // STEP)
    ts = np.arange(steps, dtype=np.float64)
    score = {"rising": 6 + 3 * ts, "falling": 6 + 3 * (steps - 1 - ts), "rising120": 6 + 120 * ts, "diagonal": 6 + 0 * ts}[variant]
    spikes = [STEP * i + (5 * i + 3) % STEP for i in range(steps)]
    if variant == "diagonal":
        for j in range(st, st + s):
            if j not in spikes:
                for kv in range(kvh):
                    qh = q[0, j - st, kv * group + j % group].double()
                    k[0, kv, j] = (14.0 * d ** 0.5 * qh / (qh * qh).sum()).to(torch.bfloat16)
    for i, j in enumerate(spikes):
        if j < st + s:
            k[0, :, j] = (had[[3, 9]] * float(score[i]) / d ** 0.5).to(torch.bfloat16)
    start = torch.tensor([st], dtype=torch.int32)
    return _with_reference(Batch(d, group, kvh, q, _tail(k, [st], s, 41), _tail(v, [st], s, 42), start))


# ---------------------------------------------------------------- 6. extremes

def huge_scores(d, group, kvh, mx=False):
    """"near" with q rows of 2^53 .. 2^56 and keys of 64 mult 2^k_exp, k_exp 53 at d 32 and 55 at d 128, every other
    block's mult negative: a read score q . k = d 2^(59 + k_exp + s % 4) mult. At d 32 the blocks below position 198
    have mult up to 7: at most 2^5 2^115 7 = 2^122.8; at d 128 mult is 1 and -2: 2^7 2^117 = 2^124 read and -2^125
    beside it. Every sum the MFMA forms is at most 2^125 in magnitude; times log2(e) / sqrt(128) = 2^-2.97 it is a
    score of at most 2^122.03, and less a maximum of 2^121.03 the exp2 argument stays above -2^122.7: inside f32.
    Every partial sum of the MFMA is an integer below 2^10 times one power of two: exact."""
    return onehot(d, group, kvh, EXT_S, EXT_START + EXT_S + 3, "near", starts=(EXT_START,), mx=mx, q_exp=54,
                  k_exp=53 if d == 32 else 55, signed=True)


def subnormal_readout(d, group, kvh):
    """"near" over bf16-subnormal V."""
    return onehot(d, group, kvh, EXT_S, EXT_START + EXT_S + 3, "near", starts=(EXT_START,), subnormal=True)


@functools.lru_cache(maxsize=None)
def extreme_v(d, group, kvh, exponent):
    """A flat softmax (all keys zero) over V = an ordinary V times 2^exponent, +-100. At 2^100 the sum of at
    most BK + 5 + BQ + 1 = 198 rows of magnitude below 2^103 with weight 1 each stays below 2^110.7: inside f32."""
    s, st = EXT_S, EXT_START
    t = st + s + 3
    gen = torch.Generator().manual_seed(530 + d)
    v = (ordinary_v((1, kvh, t, d), gen).float() * 2.0 ** exponent).to(torch.bfloat16)
    q = torch.randn(1, s, kvh * group, d, generator=gen).to(torch.bfloat16)
    k = torch.zeros(1, kvh, t, d, dtype=torch.bfloat16)
    return _with_reference(Batch(d, group, kvh, q, _tail(k, [st], s, 531), _tail(v, [st], s, 532),
                                 torch.tensor([st], dtype=torch.int32)))


@functools.lru_cache(maxsize=None)
def ordinary(d, group, kvh, mx=False):
    """Two sequences of random normal q, K, V, S = BQ + 1 behind start = BK + 5 and behind 3; with `mx` K and V
    are put through the host codec (batch.k, batch.v: the dequantized values)."""
    s, starts = EXT_S, [EXT_START, 3]
    t = EXT_START + s + 3
    gen = torch.Generator().manual_seed(700 + d)
    q = torch.randn(2, s, kvh * group, d, generator=gen).to(torch.bfloat16)
    k = torch.randn(2, kvh, t, d, generator=gen).to(torch.bfloat16)
    v = torch.randn(2, kvh, t, d, generator=gen).to(torch.bfloat16)
    codes = None
    if mx:
        (kc, ks), (vc, vs) = quantize(k), quantize(v)
        k, v = dequant(kc, ks), dequant(vc, vs)
        valid = (torch.arange(t)[None, :] < (torch.tensor(starts) + s)[:, None])[:, None, :, None]
        nan, ff = torch.tensor(0x7F, dtype=torch.uint8), torch.tensor(0xFF, dtype=torch.uint8)
        codes = (torch.where(valid, kc, nan), torch.where(valid, ks, ff), torch.where(valid, vc, ff), torch.where(valid, vs, ff))
    return Batch(d, group, kvh, q, _tail(k, starts, s, 701), _tail(v, starts, s, 702), torch.tensor(starts, dtype=torch.int32), codes)


def visiting_rows(st, s, j):
    """Rows i of a sequence (start st, S rows, T >= st + S) with st + i < j whose wave still visits the 32-position
    step of j. From the kernel: row i lies in query tile i // BQ and in the wave whose first row sits at position
    wpos0 = st + 32 (i // 32); the wave runs step p0 = 32 (j // 32) unless p0 > wpos0 + 31, and the tile loop reaches
    it because j < st + S lies at or before the query tile's last position (a full tile ends at wpos0 + 31 of its last
    wave; the partial last tile at st + S - 1 >= j). So: p0 <= wpos0 + 31, fewer than 63 positions before j."""
    i = np.arange(s)
    return i[(st + i < j) & (STEP * (j // STEP) <= st + STEP * (i // STEP) + STEP - 1)]
