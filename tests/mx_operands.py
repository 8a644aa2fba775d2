"""Hand-made MXFP8 operands for the W4A8 kernels (csrc/kernels/mxfp4_mx.hip): case builders, the
float64 reference and a runner on the raw bindings (_core.mxfp4_linear_mx, _core.mxfp4_swiglu_mx),
which take the codes and scale bytes of x by pointer. A plain module: test_mx_operands_host.py
asserts on the reference alone that every builder covers and discriminates what it says,
test_gpu_mxfp4_mx_extremes.py runs the cases on the GPU.

ops.mxfp4_linear(act="mxfp8") only ever feeds what the quantizer makes: a code of exponent field 14
or 15 in every non-zero block, scale bytes in 1..247 and, on small integers, the same byte in almost
every block. Here x^ is written by hand: any of the 254 non-NaN e4m3 codes under any scale byte.

The reference is numpy float64 and nothing of it goes through ops or a kernel: x^ = dequantize of
test_mxfp4_mx_host.py (a block under scale byte 0xFF, the E8M0 NaN, is NaN), w^ = ref_weight of
test_mxfp4_linear_host.py. Shapes are in terms of BM, BN = _core.mxfp4_mx_tile(). A step is 128
consecutive k (four scale blocks), a piece 16 consecutive bytes of a step; the classes are the
kernel's sort of the e4m3 codes by exponent field f: f <= 5, 6..10, >= 11.

  a. readout_a: an identity weight (N = K, 1.0 at k = n under scale byte 127): y = x^. Every code
     in every byte lane of a dword and in every piece, scale bytes 0..254 that differ inside every
     step; only |code * 2^(byte - 127)| >= 2^128 is left out (restrict_codes). `mid`: scale bytes
     100..140 only. The up parameter of the full-range variant lies under scale bytes 59..61.
  b. readout_b: a one-hot x (M = K, code 0x38 = 1.0 at k = m under byte 127): y[m][n] = w^[n][m].
     All 16 nibbles at both nibble positions under scale bytes 0..254.
  c. association: one (or two) live blocks per row among zero blocks with decoy scale bytes; exact.
  d. boundaries: the smallest and largest code of a class, and the codes on either side of a class
     boundary, in one group of 8 consecutive k; exact. Rows with the extremes of all three classes
     in one group, and rows whose sum is a tie in f32, are held to the f32 chain class 0 -> 1 -> 2
     (class_chain).
  e. wide: random codes, x scale bytes 90..160, weight scale bytes 100..150: the project's bound
     K 2^-23 sum |x^ w^|.
  f. nonfinite: x scale byte 0xFF and the NaN codes 0x7F / 0xFF.

Every case carries a second, ordinary parameter `up` behind the first for the gated kernel.
mutated_want gives the expectation a kernel with a named defect would meet; the host twin asserts
that it differs."""
from dataclasses import dataclass, field

import numpy as np
import torch

from distributed_llm_dissemination_amd import _core

import linear_extremes as le
import test_mxfp4_linear_host as mx
from test_gpu_mxfp4_linear import LAYOUTS
from test_mxfp4_mx_host import dequantize, e4m3_to_f64

BM, BN = _core.mxfp4_mx_tile()
KS = (160, 224, 288)  # a step and a tail of one block, of three blocks, two steps and a tail
CODES254 = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
ONE_E4M3, ONE_E2M1, HALF_E2M1, SIX_E2M1 = 0x38, 2, 1, 7
F32_TOP = 2.0 ** 128


def field_of(codes):
    """The exponent field of e4m3 codes."""
    return (np.asarray(codes).astype(np.int64) >> 3) & 15


def class_of(codes):
    """The kernel's class of e4m3 codes: 0 for f <= 5, 1 for 6..10, 2 for f >= 11 (split_classes)."""
    f = field_of(codes)
    return (f >= 6).astype(np.int64) + (f >= 11)


def x_values(codes, scales):
    """x^ in float64; a block under scale byte 0xFF is NaN (E8M0), zero codes included."""
    with np.errstate(invalid="ignore"):
        v = dequantize(codes, scales)
    return np.where(np.repeat(np.asarray(scales) == 0xFF, 32, axis=-1), np.nan, v)


def w_values(nib, sb):
    """code * 2^(byte - 127) in float64 for nibbles [n, k] under scale bytes [n, k / 32]."""
    v = np.where(nib & 8, -1.0, 1.0) * E2M1[nib & 7]
    return np.ldexp(v, np.repeat(sb.astype(np.int64) - 127, 32, axis=-1))


def restrict_codes(codes, scales):
    """Codes whose value under their scale byte reaches 2^128 get their exponent field lowered by 8
    (such a code has f >= 8); returns (codes, mask of the changed ones)."""
    over = np.abs(dequantize(codes, scales)) >= F32_TOP
    assert (field_of(codes[over]) >= 8).all()
    out = np.where(over, codes - 0x40, codes).astype(np.uint8)
    assert (np.abs(dequantize(out, scales)) < F32_TOP).all()
    return out, over


def restrict_nibbles(nib, sb):
    """Nibbles whose value reaches 2^128 (4 and 6 under byte 253; 2, 3, 4, 6 under 254) get a
    magnitude four places lower; returns (nibbles, mask of the changed ones)."""
    over = np.abs(w_values(nib, sb)) >= F32_TOP
    assert ((nib[over] & 7) >= 4).all()
    out = np.where(over, nib - 4, nib).astype(np.uint8)
    assert (np.abs(w_values(out, sb)) < F32_TOP).all()
    return out, over


def rand_weight(n, k, seed, scales=(126, 127, 128)):
    """Random nibbles and scale bytes from `scales`: (nib [n, k], sb [n, k / 32])."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 16, (n, k), dtype=np.uint8),
            rng.choice(np.array(scales, dtype=np.uint8), (n, k // 32)))


def weight_image(params, chunk, off, behind, seed, gap=64):
    """A packed layer with the parameters `params` = [(nib, sb), ...] one behind the other from
    element `off`, `gap` elements apart, and `behind` elements behind the last; everything else is
    handmade_image's. Returns (image, total elements, [offset of each parameter])."""
    offs, e = [], off
    for nib, _ in params:
        offs.append(e)
        e += nib.size + gap
    total = e - gap + behind
    img = mx.handmade_image(total, chunk, seed)
    for (nib, sb), o in zip(params, offs):
        qi, si = le.mxfp4_index(total, chunk, o + np.arange(nib.size, dtype=np.int64))
        flat = nib.reshape(-1).astype(np.uint8)
        img[qi[0::2]] = flat[0::2] | (flat[1::2] << 4)
        img[si[0::32]] = sb.reshape(-1)
    return img, total, offs


@dataclass
class MxCase:
    name: str
    codes: np.ndarray     # e4m3 codes of x^ [m, k]
    scales: np.ndarray    # E8M0 bytes [m, k / 32]
    img: np.ndarray       # the packed layer
    total: int
    chunk: int
    off: int              # the parameter under test
    up: int               # an ordinary parameter of the same shape behind it (-1: none)
    n: int
    k: int
    xh: np.ndarray        # x^ in float64
    wf: np.ndarray        # w^ of `off` in float64
    want: np.ndarray      # float64 [m, n]
    extra: dict = field(default_factory=dict)

    @property
    def m(self):
        return self.codes.shape[0]

    def up_weight(self):
        return mx.ref_weight(self.img, self.total, self.chunk, self.up, self.n, self.k)


def matmul64(xh, wf):
    with np.errstate(invalid="ignore", over="ignore"):
        return xh @ wf.T


def make_case(name, codes, scales, nib, sb, seed, layout=(1024, 32 * 7, 32 * 5), with_up=True,
              up_scales=(126, 127, 128), **extra):
    """The case of x^ = (codes, scales) against the parameter (nib, sb) at `layout` = (chunk bytes,
    offset, elements behind); with_up: random weights of the same shape under scale bytes from
    `up_scales` 64 elements behind it."""
    n, k = nib.shape
    chunk, off, behind = layout
    params = [(nib, sb)] + ([rand_weight(n, k, seed + 1, up_scales)] if with_up else [])
    img, total, offs = weight_image(params, chunk, off, behind, seed)
    codes, scales = np.ascontiguousarray(codes, dtype=np.uint8), np.ascontiguousarray(scales, dtype=np.uint8)
    assert codes.shape[1] == k and scales.shape == (codes.shape[0], k // 32)
    xh, wf = x_values(codes, scales), mx.ref_weight(img, total, chunk, off, n, k)
    return MxCase(name, codes, scales, img, total, chunk, off, offs[1] if with_up else -1, n, k, xh, wf,
                  matmul64(xh, wf), dict(nib=nib, sb=sb, **extra))


# ---------------------------------------------------------------- a. the A path through an identity weight

def identity_weight(k):
    nib = np.zeros((k, k), dtype=np.uint8)
    nib[np.arange(k), np.arange(k)] = ONE_E2M1
    return nib, np.full((k, k // 32), 127, dtype=np.uint8)


def readout_a(k, mid=False):
    """M = BM + 1 rows. Position (m, k): step s, piece p, dword j of the piece, byte lane l. The code
    is a fixed permutation of the 254 at index 4 m + j + 37 p + 11 l + 101 s: for one (p, l) the
    4 (BM + 1) > 2 * 254 places of a step run through every code. Scale byte of block 4 s + g of
    row m: (13 m + 29 s + 67 g) mod 255, with `mid` 100 + (13 m + 29 s + 11 g) mod 41 - the four
    of a step differ either way. extra["restricted"]: the codes restrict_codes lowered."""
    m = BM + 1
    mm, kk = np.indices((m, k))
    s, o = kk // 128, kk % 128
    lut = np.random.default_rng(254).permutation(CODES254)
    codes = lut[(4 * mm + (o % 16) // 4 + 37 * (o // 16) + 11 * (o % 4) + 101 * s) % 254]
    mr, bb = np.indices((m, k // 32))
    if mid:
        scales = 100 + (13 * mr + 29 * (bb // 4) + 11 * (bb % 4)) % 41
    else:
        scales = (13 * mr + 29 * (bb // 4) + 67 * (bb % 4)) % 255
    scales = scales.astype(np.uint8)
    raw = codes.copy()
    codes, changed = restrict_codes(codes, scales)
    nib, sb = identity_weight(k)
    # under bytes 0..254 |x^| reaches 2^127: weights of at most 6 * 2^-66 keep the f32 sums of `up` finite
    return make_case(f"a K={k}" + (" mid" if mid else ""), codes, scales, nib, sb, 300 + k,
                     up_scales=(126, 127, 128) if mid else (59, 60, 61), restricted=changed, raw=raw)


# ---------------------------------------------------------------- b. the B path through a one-hot x

def one_hot_x(k):
    codes = np.zeros((k, k), dtype=np.uint8)
    codes[np.arange(k), np.arange(k)] = ONE_E4M3
    return codes, np.full((k, k // 32), 127, dtype=np.uint8)


def readout_b(k, layout):
    """N = BN + 16 weight rows, nibble (5 n + 3 k + k / 32) mod 16, scale byte of block 4 s + g of
    row n (13 n + 29 s + 67 g) mod 255; `layout`: a name of test_gpu_mxfp4_linear.LAYOUTS."""
    n = BN + 16
    nn, kk = np.indices((n, k))
    nib = ((5 * nn + 3 * kk + kk // 32) % 16).astype(np.uint8)
    nr, bb = np.indices((n, k // 32))
    sb = ((13 * nr + 29 * (bb // 4) + 67 * (bb % 4)) % 255).astype(np.uint8)
    raw = nib.copy()
    nib, changed = restrict_nibbles(nib, sb)
    codes, scales = one_hot_x(k)
    return make_case(f"b K={k} {layout}", codes, scales, nib, sb, 400 + k, LAYOUTS[layout], with_up=False,
                     restricted=changed, raw=raw)


# ---------------------------------------------------------------- c. scale association, exact

def association(k, live=1):
    """2 BM + 5 rows (17 row tiles: at least 16 per row position m % 16, more than K / 32 blocks) by
    48 weight rows. Row m's live block is (m % 16 + m / 16) mod (K / 32); with live = 2 a second one
    lies 1 .. K / 32 - 1 blocks further. Every other block holds zero codes under a decoy scale byte
    in 90..160 that differs from the live ones. The live codes have an even mantissa and exponent
    fields 4..12 - all three classes - (live = 2: fields 5 and 6, either side of the first class
    boundary, the second block's scale up to 2^8 above the first's): multiples of 2^-5 (2^-4) of
    the row's scale up to 56 (1.75), against multiples of 2^-2 up to 12: a block's products stay
    below 2^22 (2^15) quanta. extra["ux"]: the quantum of x^ per row."""
    m, n, nb = 2 * BM + 5, 48, k // 32
    rng = np.random.default_rng(500 + k + live)
    rows = np.arange(m)
    b1 = (rows % 16 + rows // 16) % nb
    s1 = 100 + rng.integers(0, 41, m)
    s1 = np.where(s1 == 127, 128, s1)  # 127 is what an absent block of the tail carries
    lives = [(b1, s1)]
    if live == 2:
        lives.append(((b1 + 1 + rng.integers(0, nb - 1, m)) % nb, s1 + rng.integers(0, 9, m)))
    scales = rng.integers(90, 161, (m, nb))
    for _ in range(len(lives)):  # a decoy moved off one live byte may land on the other
        for _, sv in lives:
            scales = np.where(scales == sv[:, None], scales + 1, scales)
    assert not any((scales == sv[:, None]).any() for _, sv in lives)
    codes = np.zeros((m, k), dtype=np.uint8)
    lo, hi = (4, 12) if live == 1 else (5, 6)
    for bv, sv in lives:
        blk = (rng.integers(0, 2, (m, 32)) << 7) | (rng.integers(lo, hi + 1, (m, 32)) << 3) | (2 * rng.integers(0, 4, (m, 32)))
        codes[rows[:, None], 32 * bv[:, None] + np.arange(32)] = blk
        scales[rows, bv] = sv
    nib, sb = rand_weight(n, k, 510 + k)
    ux = np.ldexp(1.0, (lo - 9) + s1 - 127)
    return make_case(f"c K={k} live={live}", codes, scales, nib, sb, 520 + k, live_blocks=[b for b, _ in lives],
                     live_scales=[s for _, s in lives], ux=ux, uw=2.0 ** -2)


def prove_rows(c, rows=None, wf=None, want=None):
    """linear_extremes.prove_exact per quantum of x^ (extra["ux"], one per row): every product of
    the rows is a multiple of ux uw and every row's sum of magnitudes is below 2^24 of them."""
    wf = c.wf if wf is None else wf
    want = matmul64(c.xh, wf) if want is None else want
    rows = np.arange(c.m) if rows is None else np.asarray(rows)
    for u in np.unique(c.extra["ux"][rows]):
        r = rows[c.extra["ux"][rows] == u]
        le.prove_exact(c.xh[r], wf, float(u), c.extra["uw"], want[r])


# ---------------------------------------------------------------- d. class boundaries inside a group of 8

# (the small code, the large code): the ends of each class, then the two codes on either side of
# each class boundary (f = 5 | 6 and 10 | 11)
PAIRS = [(0x01, 0x2F), (0x30, 0x57), (0x58, 0x7E), (0x2F, 0x30), (0x57, 0x58)]
MIXED = [0x01, 0x2F, 0x30, 0x57, 0x58, 0x7E, 0xFE, 0x81]  # the ends of all three classes in one group
# seven times the largest code and one subnormal: with the weights 6 and 0.5 the group sums to
# 7 * 2688 + s 2^-10 (s = 1, 3, 5, 7), a tie between two f32 neighbours (2^-9 apart from 2^14 on)
TIES = [0x01, 0x03, 0x05, 0x07]


def group_positions(k):
    """First k of the live group: the first, a middle and the last group of a step, and one of the tail."""
    last = 128 * (k // 128 - 1)
    return [0, last + 56, last + 120, 128 * (k // 128) + 8]


def boundaries(k):
    """BM + 1 rows, each with one live group of 8 consecutive k: small at place j of the group, +large
    and -large one and three places on (the large terms cancel against equal weights). 16 weight
    rows: 6 everywhere but 0.5 where k % 8 == n % 8, negative from row 8 on, scale bytes 126..128 - in
    column j (and j + 8) the answer is the small code times 0.5 alone. Every other block of x is
    zero under scale byte 127, the live one has byte 120 + m % 15. Configurations = PAIRS x
    positions x j in (0, 5), then MIXED and each of TIES (seven 0x7E and the subnormal at place 7)
    at every position, repeated with the sign flipped. want is class_chain: on the PAIRS rows it
    rounds nowhere (asserted by the callers), on the TIES rows columns 7 and 15 sit on a tie, which
    the chain's round to nearest even decides. extra["mixed"]: the rows that hold MIXED or TIES
    (classes 0 and 2, or all three, in one group), extra["ux"] the quantum per row."""
    m, n = BM + 1, 16
    pos = group_positions(k)
    configs = ([(p, g0, j) for p in PAIRS for g0 in pos for j in (0, 5)] + [(None, g0, 0) for g0 in pos]
               + [(("tie", t), g0, 0) for t in TIES for g0 in pos])
    codes = np.zeros((m, k), dtype=np.uint8)
    scales = np.full((m, k // 32), 127, dtype=np.uint8)
    mixed = np.zeros(m, dtype=bool)
    for r in range(m):
        pair, g0, j = configs[r % len(configs)]
        grp = np.zeros(8, dtype=np.uint8)
        if pair is None:
            grp[:], mixed[r] = MIXED, True
        elif pair[0] == "tie":
            grp[:7], grp[7], mixed[r] = 0x7E, pair[1], True
        else:
            grp[j], grp[(j + 1) % 8], grp[(j + 3) % 8] = pair[0], pair[1], pair[1] | 0x80
        if (r // len(configs)) % 2:
            grp = np.where(grp != 0, grp ^ 0x80, grp).astype(np.uint8)
        codes[r, g0: g0 + 8] = grp
        scales[r, g0 // 32] = 120 + r % 15
    nn, kk = np.indices((n, k))
    nib = (np.where(kk % 8 == nn % 8, HALF_E2M1, SIX_E2M1) | np.where(nn >= 8, 8, 0)).astype(np.uint8)
    nr, bb = np.indices((n, k // 32))
    sb = (126 + (nr + bb) % 3).astype(np.uint8)
    live = codes != 0
    lsb = np.where(live, np.maximum(field_of(codes), 1) - 10, 99).min(1)  # a code is a multiple of 2^(max(f, 1) - 10)
    ux = np.ldexp(1.0, lsb + scales[np.arange(m), live.argmax(1) // 32].astype(np.int64) - 127)
    c = make_case(f"d K={k}", codes, scales, nib, sb, 600 + k, mixed=mixed, ux=ux, uw=2.0 ** -2, configs=configs)
    c.extra["float64"] = c.want
    c.want = class_chain(c.codes, c.xh, c.wf)
    return c


def class_chain(codes, xh, wf):
    """The kernel's order of accumulation as f32 steps in numpy: per step of 128 k the classes 0, 1, 2,
    each class's products summed exactly (float64 holds them) and added to the one f32 accumulator
    with one rounding. Returned as float64."""
    cls = class_of(codes)
    acc = np.zeros((xh.shape[0], wf.shape[0]), dtype=np.float32)
    for k0 in range(0, xh.shape[1], 128):
        for c in range(3):
            part = np.where(cls[:, k0: k0 + 128] == c, xh[:, k0: k0 + 128], 0.0) @ wf[:, k0: k0 + 128].T
            acc = (acc.astype(np.float64) + part).astype(np.float32)
    return acc.astype(np.float64)


def f32_bound(xh, wf):
    """K 2^-23 sum_k |x^ w^|: the project's bound on an f32 accumulation of K products."""
    return xh.shape[1] * 2.0 ** -23 * (np.abs(xh) @ np.abs(wf).T)


# ---------------------------------------------------------------- e. wide scales, bounded

WIDE = (2 * BM + 5, BN + 16, 1056 + 64)  # eight steps and a tail of three blocks


def wide():
    m, n, k = WIDE
    rng = np.random.default_rng(700)
    codes = rng.choice(CODES254, (m, k))
    scales = rng.integers(90, 161, (m, k // 32)).astype(np.uint8)
    nib, sb = rand_weight(n, k, 701, scales=tuple(range(100, 151)))
    return make_case("e", codes, scales, nib, sb, 702)


# ---------------------------------------------------------------- f. non-finite

NONFINITE = (BM + 1, 48, 160)
BAD_ROWS = (0, BM - 1, BM)   # the first row, the last of the first tile, the lone row of the second
BAD_BLOCKS = (1, 4)          # a block of the main step, the block of the tail
ZERO_COL, NAN_COL = 3, 20    # the column with a zero weight at the NaN code's k; the one under a 0xFF scale


def nonfinite():
    """(clean case, variants). A variant is a dict: codes, scales, img (the clean image unless the
    weights change), rows (the rows of y that are NaN) and cols (the columns that are). x scale
    byte 0xFF in a block of the main step and of the tail of rows 0, BM - 1 and BM, over the
    block's ordinary codes and over zeros; the codes 0x7F and 0xFF at byte 5 of each of the 8
    pieces of the step and of the 2 of the tail, in a row that walks with the piece, with a zero
    weight at that k in column ZERO_COL and scale byte 0xFF over that k in column NAN_COL."""
    m, n, k = NONFINITE
    rng = np.random.default_rng(800)
    codes = rng.choice(CODES254, (m, k))
    scales = rng.integers(118, 137, (m, k // 32)).astype(np.uint8)
    nib, sb = rand_weight(n, k, 801)
    c = make_case("f", codes, scales, nib, sb, 802)
    out = []
    for r in BAD_ROWS:
        for b in BAD_BLOCKS:
            for zero in (False, True):
                q, s = c.codes.copy(), c.scales.copy()
                s[r, b] = 0xFF
                if zero:
                    q[r, 32 * b: 32 * b + 32] = 0
                out.append(dict(name=f"x scale 0xFF row {r} block {b}" + (" over zeros" if zero else ""), codes=q,
                                scales=s, img=c.img, rows=[r], cols=[]))
    for p in range(10):
        kk = 16 * p + 5
        r = (BM - 1 + 7 * p) % m
        nb2, sb2 = nib.copy(), sb.copy()
        nb2[ZERO_COL, kk] = 0
        sb2[NAN_COL, kk // 32] = 0xFF
        img = weight_image([(nb2, sb2), rand_weight(n, k, 803)], c.chunk, c.off, 32 * 5, 802)[0]
        for code in (0x7F, 0xFF):
            q = c.codes.copy()
            q[r, kk] = code
            out.append(dict(name=f"x code {code:#x} row {r} k {kk}", codes=q, scales=c.scales, img=img, rows=[r],
                            cols=[NAN_COL], zero_at=(ZERO_COL, kk)))
    return c, out


def variant_want(c, v):
    """float64 expectation of a variant of nonfinite(): NaN rows and columns come out of the arithmetic."""
    return matmul64(x_values(v["codes"], v["scales"]), mx.ref_weight(v["img"], c.total, c.chunk, c.off, c.n, c.k))


# ---------------------------------------------------------------- mutated references

def flush_f32(a):
    """`a` with the f32 subnormals flushed to zero."""
    return np.where(np.abs(a) < 2.0 ** -126, 0.0, a)


def _steps(scales):
    """Scale bytes [m, K / 32] as [m, steps, 4], the absent blocks of the tail 127 (what the kernel feeds)."""
    m, nb = scales.shape
    pad = np.full((m, -(-nb // 4) * 4), 127, dtype=np.int64)
    pad[:, :nb] = scales
    return pad.reshape(m, -1, 4)


def mutated_x(c, kind, arg=None):
    """x^ as a kernel with the defect `kind` sees it: "swap" (i, j): block i of every step under
    the scale byte of block j of that step; "lanes32": the byte of lane group g over the 32 codes
    the lane holds (k % 64 in [16 g, 16 g + 16) of either half) in place of block g; "drop" f: the
    codes of exponent field f fall out of every class; "double" f: they are in two classes."""
    codes, nb = c.codes, c.k // 32
    s4 = _steps(c.scales)
    if kind == "swap":
        i, j = arg
        s4 = s4.copy()
        s4[:, :, i] = _steps(c.scales)[:, :, j]
        return x_values(codes, s4.reshape(c.m, -1)[:, :nb])
    if kind == "lanes32":
        kk = np.arange(c.k)
        e = s4[:, kk // 128, (kk % 64) // 16] - 127
        return np.ldexp(e4m3_to_f64(codes), e)
    hit = field_of(codes) == arg
    return np.where(hit, {"drop": 0.0, "double": 2.0}[kind] * c.xh, c.xh)


def mutated_want(c, kind, arg=None):
    """The expectation under the defect: those of mutated_x, "flush" (f32 subnormals of the result
    become 0) and "wswap" (i, j), mutated_x's swap on the weight side."""
    if kind == "flush":
        return flush_f32(c.want)
    if kind == "wswap":
        i, j = arg
        s4 = _steps(c.extra["sb"])
        t = s4.copy()
        t[:, :, i] = s4[:, :, j]
        return matmul64(c.xh, w_values(c.extra["nib"], t.reshape(c.n, -1)[:, : c.k // 32]))
    return matmul64(mutated_x(c, kind, arg), c.wf)


SWAPS = [(i, j) for i in range(4) for j in range(4) if i != j]


# ---------------------------------------------------------------- what the quantizer can make

def as_bf16(c):
    """(x, rows): x^ of the case as a bf16 tensor [m, k] (0 where bf16 cannot hold it) and the rows
    that bf16 holds exactly - candidates for ops.mxfp4_linear(act="mxfp8"), which must then quantize
    them to the case's own codes and scale bytes (rows_the_quantizer_makes)."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = c.xh.astype(np.float32)
    ok = (f.astype(np.float64) == c.xh) & ((f.view(np.uint32) & 0xFFFF) == 0)
    x = torch.from_numpy(np.where(ok, f, np.float32(0))).to(torch.bfloat16)
    return x, np.nonzero(ok.all(1))[0]


def rows_the_quantizer_makes(c, quantize):
    """(x bf16, rows): the rows of the case whose bf16 form `quantize` (x -> (codes, scales) as numpy
    arrays, the host codec) turns into exactly the hand-made operand."""
    x, rows = as_bf16(c)
    q, s = quantize(x)
    same = (q == c.codes).all(1) & (s == c.scales).all(1)
    return x, np.array([r for r in rows if same[r]], dtype=np.int64)


# ---------------------------------------------------------------- the runner

def upload(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def run(c, gated=False, bf16=False, codes=None, scales=None, img=None, rows=None, off=None, up=None):
    """The raw binding on the current stream: _core.mxfp4_linear_mx on the parameter at `off`
    (c.off unless given), or with `gated` _core.mxfp4_swiglu_mx on gate `off` and up `up` (c.up
    unless given). codes / scales / img replace the case's; rows: a slice of the rows of x.
    `img` may be a tensor already on the GPU. Returns y [rows, n] as an f32 or bf16 tensor."""
    codes = c.codes if codes is None else codes
    scales = c.scales if scales is None else scales
    if rows is not None:
        codes, scales = codes[rows], scales[rows]
    q, s = upload(codes), upload(scales)
    p = img if torch.is_tensor(img) else upload(c.img if img is None else img)
    m = q.shape[0]
    y = torch.empty(m, c.n, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    off = c.off if off is None else off
    tail = (q.data_ptr(), s.data_ptr(), m, c.n, c.k, y.data_ptr(), c.n, bf16, stream)
    if gated:
        _core.mxfp4_swiglu_mx(p.data_ptr(), 2 * c.total, c.chunk, off, c.up if up is None else up, *tail)
    else:
        _core.mxfp4_linear_mx(p.data_ptr(), 2 * c.total, c.chunk, off, *tail)
    torch.cuda.synchronize()  # q, s and p are released when this returns
    return y
