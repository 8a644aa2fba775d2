"""Case builders for the packed linears (ops.mxfp4_linear, ops.fp8_linear, ops.mxfp4_swiglu) at
their numeric and addressing extremes. A plain module: test_linear_extremes_host.py runs the cases
through the ops' CPU route, test_gpu_linear_extremes.py through the gfx950 kernels.

The reference is the numpy ref_unpack per chunk of the layer (ref_weight of the host test modules)
followed by a float64 matmul; nothing here goes through the ops. Every builder returns the packed
image, x, the float64 expectation and what the exactness proof needs:

  x holds multiples of `ux`, W multiples of `uw`, so every product is a multiple of u = ux * uw;
  (|x| @ |W|^T).max() < 2^24 u, so every partial sum, in any order, is a multiple of u below
  2^24 u and therefore exact in f32 wherever u itself is (u >= 2^-149);
  every expected value is representable in f32.

prove_exact asserts all three on the reference alone. The f32 output then equals the expectation
bit for bit, and the bf16 output is the expectation rounded to nearest even (f32_to_bf16_bits)."""
from dataclasses import dataclass, field

import numpy as np
import torch

from distributed_llm_dissemination_amd import _core, ops

import test_fp8_linear_host as f8
import test_mxfp4_linear_host as mx

KiB = 1 << 10
SHAPES = [(5, 48, 96), (17, 48, 160), (64, 528, 1056)]  # the K tail alone; main loop + tail; with split K
ROW_TILES_SHAPE = (17, 64, 160)  # N = 64: 4 row tiles, so that row_tiles=2 can be forced


@dataclass
class Case:
    fmt: str              # "mxfp4" or "fp8"
    img: np.ndarray       # the packed image of the whole layer
    total: int            # elements of the layer
    chunk: int
    block: int            # fp8 scale block (32 for MXFP4)
    off: int              # the parameter's first element
    n: int
    k: int
    x: torch.Tensor       # bf16 [m, k]
    xf: np.ndarray        # x in float64
    wf: np.ndarray        # the [n, k] parameter in float64 (may hold inf)
    want: np.ndarray      # float64 [m, n]: what an exact f32 accumulation gives (may hold inf and NaN)
    ux: float = 0.0       # units of the exactness proof (of the finite part where want holds inf or NaN)
    uw: float = 0.0
    extra: dict = field(default_factory=dict)

    @property
    def m(self):
        return self.x.shape[0]


@dataclass
class SwigluCase:
    img: np.ndarray
    total: int
    chunk: int
    gate: int
    up: int
    n: int
    k: int
    x: torch.Tensor
    xf: np.ndarray
    wg: np.ndarray
    wu: np.ndarray
    g: np.ndarray         # float64 x Wg^T and x Wu^T, exact in f32 where finite
    u: np.ndarray
    ux: float = 0.0
    ug: float = 0.0
    uu: float = 0.0
    extra: dict = field(default_factory=dict)


# ---------------------------------------------------------------- checks on the reference alone

def is_multiple(a, unit):
    q = np.asarray(a, dtype=np.float64) / unit  # a power of two: the division is exact
    return bool(np.all(q == np.rint(q)))


def f32_representable(a):
    with np.errstate(over="ignore"):
        return bool(np.array_equal(np.asarray(a).astype(np.float32).astype(np.float64), a))


def prove_exact(xf, wf, ux, uw, want=None):
    """The three assertions of the module docstring; returns u."""
    u = ux * uw
    assert u >= 2.0 ** -149 and np.log2(ux) % 1 == 0 and np.log2(uw) % 1 == 0
    assert is_multiple(xf, ux) and is_multiple(wf, uw)
    assert (np.abs(xf) @ np.abs(wf).T).max() < 2.0 ** 24 * u
    want = xf @ wf.T if want is None else want
    assert f32_representable(want)
    return u


def subnormal_shares(c):
    """Shares that are non-zero and below 2^-126 (f32 subnormals), on the reference alone, of: the
    products of the first row of x, the running sums over the 32-element blocks of K in their
    natural order, and the outputs."""
    def share(a):
        a = np.abs(a[a != 0])
        return float((a < 2.0 ** -126).mean())

    nb = c.k // 32
    blocks = np.einsum("mbj,nbj->mnb", c.xf.reshape(-1, nb, 32), c.wf.reshape(-1, nb, 32))
    return share(c.xf[0][None, :] * c.wf), share(np.cumsum(blocks, -1)), share(c.want)


def f32_to_bf16_bits(a):
    """float32 array -> bf16 bits, to nearest and ties to even on the f32 bits (subnormals and
    overflow to inf included); NaN -> 0x7FC0."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, 0x7FC0, out).astype(np.uint16)


def expected_f32(want):
    """The float64 expectation as f32: exact where finite, +-inf from 2^128 on."""
    with np.errstate(over="ignore"):
        return want.astype(np.float32)


def assert_f32_equal(y, want):
    """y (a float32 tensor or array) against the float64 expectation: equal NaN masks, equal values
    elsewhere (inf == inf)."""
    y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    assert y.dtype == np.float32 and y.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(y), nan)
    bad = np.argwhere((y.astype(np.float64) != want) & ~nan)
    assert len(bad) == 0, (len(bad), [(tuple(i), float(y[tuple(i)]), float(want[tuple(i)])) for i in bad[:6]])


def assert_bf16_is_rounded(y16, want):
    """A bf16 output against the expectation rounded once: bit for bit, any NaN for a NaN."""
    assert y16.dtype == torch.bfloat16 and tuple(y16.shape) == want.shape
    got, exp = mx.bf16_tensor_bits(y16), f32_to_bf16_bits(expected_f32(want)).reshape(-1)
    nan = (exp & 0x7FFF) > 0x7F80
    assert np.array_equal((got & 0x7FFF) > 0x7F80, nan)
    bad = np.nonzero((got != exp) & ~nan)[0]
    assert len(bad) == 0, (len(bad), [(int(i), hex(got[i]), hex(exp[i])) for i in bad[:6]])


def assert_rows_bit_equal(y, clean, rows):
    """Rows `rows` of two tensors of one dtype hold the same bits."""
    a, b = y.detach().cpu().contiguous(), clean.detach().cpu().contiguous()
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    assert torch.equal(a.view(it)[rows], b.view(it)[rows])


# ---------------------------------------------------------------- running a case

def run_linear(c, device, x=None, img=None, **kw):
    """The case's op on `device` ("cpu": the CPU route), optionally with another x or image."""
    x = c.x if x is None else x
    p = img if torch.is_tensor(img) else torch.from_numpy(c.img if img is None else img).to(device)
    if c.fmt == "fp8":
        return ops.fp8_linear(x.to(device), p, c.n, c.k, src_bytes=2 * c.total, chunk_bytes=c.chunk, block=c.block,
                              elem_offset=c.off, **kw)
    return ops.mxfp4_linear(x.to(device), p, c.n, c.k, src_bytes=2 * c.total, chunk_bytes=c.chunk, elem_offset=c.off,
                            **kw)


def run_swiglu(c, device, x=None, img=None, **kw):
    x = c.x if x is None else x
    p = img if torch.is_tensor(img) else torch.from_numpy(c.img if img is None else img).to(device)
    return ops.mxfp4_swiglu(x.to(device), p, c.n, c.k, src_bytes=2 * c.total, chunk_bytes=c.chunk, gate_offset=c.gate,
                            up_offset=c.up, **kw)


# ---------------------------------------------------------------- inputs

def scaled_ints(m, k, seed, s=0, lo=-8, hi=8):
    """Integers in [lo, hi] times 2^s as (bf16 tensor [m, k], float64 array)."""
    v = np.ldexp(np.random.default_rng(seed).integers(lo, hi + 1, (m, k)).astype(np.float32), s)
    t = torch.from_numpy(v).to(torch.bfloat16)
    assert np.array_equal(mx.bits_to_f64(mx.bf16_tensor_bits(t)).reshape(m, k), v.astype(np.float64))
    return t, v.astype(np.float64)


def bits_x(bits):
    """bf16 bit patterns [m, k] as (bf16 tensor, float64 array)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16), mx.bits_to_f64(bits).reshape(bits.shape)


def subnormal_x(m, k, seed):
    """bf16 subnormals of either sign: bit patterns 0x0001..0x007F (multiples of 2^-133)."""
    rng = np.random.default_rng(seed)
    sign = rng.integers(0, 2, (m, k)).astype(np.uint16) << 15
    return bits_x(rng.integers(1, 0x80, (m, k)).astype(np.uint16) | sign)


def fp8_index(total, chunk, block, elem):
    """(index of the code, index of the first scale byte) of elements `elem` in the packed image:
    core/fp8.h's rule, written out (an int or an int64 array)."""
    ce = chunk // 2
    pc = ce + ce // block * 4
    c = elem // ce
    r = elem - c * ce
    nc = np.minimum(ce, total - c * ce)
    return c * pc + r, c * pc + nc + 4 * (r // block)


def mxfp4_index(total, chunk, elem):
    """(index of the code byte, index of the scale byte) of elements `elem`: core/mxfp4.h's rule."""
    ce, pc = chunk // 2, chunk // 4 + chunk // 64
    c = elem // ce
    r = elem - c * ce
    nc = np.minimum(ce, total - c * ce)
    return c * pc + r // 2, c * pc + nc // 2 + r // 32


def _mx_layer(n, k):
    """1024-B chunks (512 elements: chunk edges inside rows), the parameter at element 224 of a
    layer that goes on behind it."""
    off, chunk = 32 * 7, 1024
    return off, chunk, off + n * k + 32 * 5


def _fp8_layer(n, k, block):
    """4096-B chunks (2048 elements), the parameter at element 224 of a layer that goes on behind it."""
    off, chunk = 32 * 7, 4096
    return off, chunk, f8.padded(off + n * k + 32 * 5, block)


def _linear_case(fmt, img, total, chunk, block, off, n, k, x, xf, ux=0.0, uw=0.0, **extra):
    if fmt == "fp8":
        wf = f8.ref_weight(img, total, chunk, block, off, n, k)
    else:
        wf = mx.ref_weight(img, total, chunk, off, n, k)
    with np.errstate(invalid="ignore", over="ignore"):
        want = xf @ wf.T
    return Case(fmt, img, total, chunk, block, off, n, k, x, xf, wf, want, ux, uw, extra)


# ---------------------------------------------------------------- 1. the bottom of the range

# magnitude bytes 0x00..0x1F of either sign: at E <= -124 every one is a bf16 subnormal
FP8_LOW_CODES = np.array([s | c for s in (0, 0x80) for c in range(0x20)], dtype=np.uint8)
FP8_LOW_EXPS = (-126, -125, -124)
# core/fp8.h: the (magnitude byte, E) pairs whose product is rounded, each in both signs
FP8_ROUNDED = ([(c, -126) for c in (1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15, 17, 19, 21, 23)]
               + [(c, -125) for c in (1, 3, 5, 7, 9, 11, 13, 15)])


def fp8_pairs(c):
    """The set of (code byte, E) over the parameter's elements of an fp8 case."""
    e = c.off + np.arange(c.n * c.k, dtype=np.int64)
    ci, si = fp8_index(c.total, c.chunk, c.block, e)
    scales = np.stack([c.img[si + b] for b in range(4)], -1).copy().view(np.float32).reshape(-1)
    return set(zip(c.img[ci].tolist(), np.log2(scales).astype(np.int64).tolist()))


def subnormal_weights(fmt, m, n, k, s, block=32, seed=0):
    """W at the bottom of bf16. MXFP4: scale bytes {0, 1, 2, 3} with random codes, every weight a
    multiple of 2^-128 of magnitude at most 6 * 2^-124. fp8: E in {-126, -125, -124} with magnitude
    bytes up to 0x1F, every weight a multiple of 2^-133 after the reference's rounding (all are
    bf16 subnormals). x: integers in [-8, 8] times 2^s. s = 100: the products are normal f32 (only
    the B operand is subnormal); s = 0: products and sums are f32 subnormals or next to them;
    s = -8: all products are, and so are many of the sums of MXFP4's larger weights."""
    x, xf = scaled_ints(m, k, 31 * seed + m + k, s)
    if fmt == "fp8":
        off, chunk, total = _fp8_layer(n, k, block)
        img = f8.handmade_image(total, chunk, block, 7 + seed + n + k, codes=FP8_LOW_CODES, exps=FP8_LOW_EXPS)
        return _linear_case(fmt, img, total, chunk, block, off, n, k, x, xf, 2.0 ** s, 2.0 ** -133)
    off, chunk, total = _mx_layer(n, k)
    img = mx.handmade_image(total, chunk, 7 + seed + n + k, scales=(0, 1, 2, 3))
    return _linear_case(fmt, img, total, chunk, 32, off, n, k, x, xf, 2.0 ** s, 2.0 ** -128)


def subnormal_activations(fmt, m, n, k, block=32, seed=0):
    """The mirror image: x holds bf16 subnormals (multiples of 2^-133), W is large - MXFP4 scale
    byte 127 + 100 (multiples of 2^99), fp8 E = 100 with codes that are multiples of 1/8
    (multiples of 2^97). Only the A operand is subnormal; products and sums are normal f32."""
    x, xf = subnormal_x(m, k, 17 * seed + m + k)
    if fmt == "fp8":
        off, chunk, total = _fp8_layer(n, k, block)
        img = f8.handmade_image(total, chunk, block, 9 + seed + n + k, exps=(100,))
        return _linear_case(fmt, img, total, chunk, block, off, n, k, x, xf, 2.0 ** -133, 2.0 ** 97)
    off, chunk, total = _mx_layer(n, k)
    img = mx.handmade_image(total, chunk, 9 + seed + n + k, scales=(227,))
    return _linear_case(fmt, img, total, chunk, 32, off, n, k, x, xf, 2.0 ** -133, 2.0 ** 99)


SWIGLU_S = 110  # x = integers times 2^110


def swiglu_subnormal(which, m, n, k, seed=0):
    """mxfp4_swiglu with the `which` ("gate" or "up") weights at the bottom of bf16 (scale bytes
    {0, 1, 2, 3}) and the other ordinary ({126, 127, 128}). One x feeds both products and the two
    weights lie 2^124 apart, so x = integers times 2^110 brings the product with the subnormal
    weights into [2^-20, 2^20] (multiples of 2^-18 up to 1056 * 8 * 96 * 2^-18 < 4) while the other
    one stays finite in f32 (multiples of 2^108 below 2^125); both are exact in f32."""
    chunk, gate = 1024, 32 * 7
    up = gate + n * k + 32 * 3
    total = up + n * k + 32 * 5
    img = mx.handmade_image(total, chunk, 5 + seed + n + k)
    low = mx.handmade_image(total, chunk, 6 + seed + n + k, scales=(0, 1, 2, 3))
    first = gate if which == "gate" else up
    for e in range(first, first + n * k, 32):  # the scale bytes of the chosen parameter
        si = mxfp4_index(total, chunk, e)[1]
        img[si] = low[si]
    x, xf = scaled_ints(m, k, 3 + seed + m, SWIGLU_S)
    wg, wu = mx.ref_weight(img, total, chunk, gate, n, k), mx.ref_weight(img, total, chunk, up, n, k)
    ug, uu = (2.0 ** -128, 2.0 ** -2) if which == "gate" else (2.0 ** -2, 2.0 ** -128)
    return SwigluCase(img, total, chunk, gate, up, n, k, x, xf, wg, wu, xf @ wg.T, xf @ wu.T, 2.0 ** SWIGLU_S, ug, uu,
                      dict(which=which))


# ---------------------------------------------------------------- 2. the top of the range

def _poison_rows(n, k):
    """(weight row, [(block of the row, scale byte, signs)]): blocks of the main loop (K >= 128)
    and of the K tail; "+" and "-" give a row of +-inf, both in one row a NaN."""
    nb = k // 32
    main, tail = (1 if nb > 4 else 0), nb - 1  # nb - 1 lies in the K tail (K % 128 != 0)
    return [(0, [(main, 254, "+")]), (n // 2 + 5, [(tail, 253, "-")]), (n - 1, [(main, 253, "+"), (tail, 254, "-")]),
            (n // 2 - 3, [(tail, 254, "+-")])]


def mxfp4_overflow(m, n, k, zeros=False, seed=0):
    """MXFP4 scale bytes 253 and 254 in a few blocks of chosen weight rows. The codes of those
    blocks are +-0, +-4 and +-6 only, so every non-zero weight there is +-inf in the reference
    (4 * 2^126 = 2^128 is beyond bf16) and no finite product overflows on its own. x: integers in
    [1, 8] (with `zeros`: [0, 8], 0 * inf = NaN). The expectation of the poisoned rows is summed
    element by element in numpy; extra["clean"] is the same case on the unpoisoned image."""
    off, chunk, total = _mx_layer(n, k)
    clean = mx.handmade_image(total, chunk, 11 + seed + n + k)
    x, xf = scaled_ints(m, k, 13 + seed + m, 0, 0 if zeros else 1, 8)
    img = clean.copy()
    rng = np.random.default_rng(seed + 5)
    nib = {"+": [0, 6, 7], "-": [8, 14, 15], "+-": [6, 7, 14, 15]}
    rows = []
    for r, blocks in _poison_rows(n, k):
        rows.append(r)
        for b, sb, signs in blocks:
            qi, si = mxfp4_index(total, chunk, off + r * k + 32 * b)
            codes = rng.choice(nib[signs], 32)
            codes[:4] = (nib[signs] * 4)[:4]  # every listed code at least once
            img[qi: qi + 16] = codes[0::2] | (codes[1::2] << 4)
            img[si] = sb
    c = _linear_case("mxfp4", img, total, chunk, 32, off, n, k, x, xf, 1.0, 2.0 ** -2)
    cl = _linear_case("mxfp4", clean, total, chunk, 32, off, n, k, x, xf, 1.0, 2.0 ** -2)
    keep = np.setdiff1d(np.arange(n), rows)
    assert np.isinf(c.wf[rows]).any(1).all() and np.isfinite(c.wf[keep]).all()
    assert np.array_equal(c.wf[keep], cl.wf[keep])
    assert np.isin(np.abs(c.wf[rows][np.isfinite(c.wf[rows])]), [0, 0.25, 0.5, 0.75, 1, 1.5, 2, 3, 4, 6, 8, 12]).all()
    with np.errstate(invalid="ignore"):
        for r in rows:
            c.want[:, r] = (xf * c.wf[r][None, :]).sum(1)
    assert not np.isfinite(c.want[:, rows]).any() and np.array_equal(c.want[:, keep], cl.want[:, keep])
    c.extra.update(clean=cl, rows=rows, keep=keep)
    return c


FP8_TOP_E, FP8_COOL_E = 120, 96


def fp8_overflow(m, n, k, block, seed=0, layer=None, other=-1):
    """fp8 at E = 120, where the weights reach the bf16 maximum (magnitude byte 0x77 = 240, core/fp8.h
    sat_limit; 0x78..0x7E stay out). A few "hot" weight rows lie in blocks of scale 2^120 with
    magnitudes 16..240; every other block has scale 2^96 and magnitudes 0, 1..15; what a hot block
    holds of other rows is 0. Every code of a weight row has the row's sign and x holds integers in
    [1, 8], so all products of one output have one sign and the partial sums grow monotonically:
    a hot row's sum is at least 96 * 16 * 2^120 > 2^129 and overflows to +-inf, every other sum is
    below 1056 * 8 * 15 * 2^96 < 2^113 and exact (multiples of 2^93 below 2^117).
    Two "warm" rows tell finite weights at E = 120 from inf: they lie in blocks of scale 2^120 too and
    hold 0 except 6.5 and 8 (one in the main loop where K has one, one in the K tail) resp. a single
    112 at a position where every row of x holds 1. Their sums, (14.5 .. 116) * 2^120 and 112 * 2^120,
    lie in [2^123, 2^127) and are exact (multiples of 2^117).
    `layer` = (off, chunk, total) replaces the default layout; `other` >= 0 is a second [n, k]
    parameter of that layer, at least one scale block away, which gets cool codes of one sign per row
    like the cool rows here (extra["wo"], extra["other"]: its weights and x W^T, exact as the kept
    columns are)."""
    off, chunk, total = _fp8_layer(n, k, block) if layer is None else layer
    rng = np.random.default_rng(21 + seed + n + k + block)
    e = np.arange(total, dtype=np.int64)
    ci, si = fp8_index(total, chunk, block, e)
    row = np.where((e >= off) & (e < off + n * k), (e - off) // k, -1)
    hot_rows, warm_rows = [1, n // 2, n - 2], [4, n - 6]
    pa, pb, pc = (37 if k >= 128 else 5), k - 3, k - 20  # pb and pc lie in the K tail
    blk = e // block  # chunks hold whole blocks
    hot_elem = np.isin(blk, np.unique(blk[np.isin(row, hot_rows + warm_rows)]))
    in_hot_row = np.isin(row, hot_rows)
    mag = np.where(in_hot_row, rng.integers(0x58, 0x78, total),
                   np.where(hot_elem, 0, rng.choice(np.r_[0, np.arange(0x38, 0x58)], total)))
    mag[np.isin(e, [off + r * k for r in hot_rows])] = 0x77  # the format's largest value there
    mag[np.isin(row, warm_rows)] = 0
    for r, p, code in [(warm_rows[0], pa, 0x4D), (warm_rows[0], pb, 0x50), (warm_rows[1], pc, 0x6E)]:  # 6.5, 8, 112
        mag[off + r * k + p] = code
    sign = np.where(row >= 0, (row % 2) * 0x80, rng.integers(0, 2, total) * 0x80)
    if other >= 0:
        in_other = (e >= other) & (e < other + n * k)
        assert not (hot_elem & in_other).any()
        sign = np.where(in_other, ((e - other) // k % 2) * 0x80, sign)
    img = np.zeros(int(_core.fp8_packed_size(2 * total, chunk, block)), dtype=np.uint8)
    img[ci] = (mag | sign).astype(np.uint8)
    scales = np.ldexp(1.0, np.where(hot_elem[::block], FP8_TOP_E, FP8_COOL_E)).astype(np.float32)
    img[si[::block, None] + np.arange(4)] = scales.view(np.uint8).reshape(-1, 4)
    xf = scaled_ints(m, k, 23 + seed + m, 0, 1, 8)[1]
    xf[:, pc] = 1.0
    x = torch.from_numpy(xf.astype(np.float32)).to(torch.bfloat16)
    c = _linear_case("fp8", img, total, chunk, block, off, n, k, x, xf, 1.0, 2.0 ** (FP8_COOL_E - 3))
    keep = np.setdiff1d(np.arange(n), hot_rows + warm_rows)
    assert np.isfinite(c.wf).all() and np.abs(c.wf).max() == 240 * 2.0 ** 120
    assert all((np.sign(c.wf[r]) * (-1) ** r >= 0).all() for r in range(n))  # one sign per row
    assert ((np.abs(c.want) < 2.0 ** 127) | (np.abs(c.want) > 2.0 ** 129)).all()
    assert (np.abs(c.want[:, hot_rows]) > 2.0 ** 129).all() and (np.abs(c.want[:, keep]) < 2.0 ** 127).all()
    c.want = np.where(np.abs(c.want) > 2.0 ** 129, np.copysign(np.inf, c.want), c.want)
    warm = np.abs(c.want[:, warm_rows])
    assert (warm >= 2.0 ** 123).all() and (warm < 2.0 ** 127).all()
    assert (np.abs(c.wf[warm_rows]).max(1) >= 2.0 ** 123).all()
    c.extra.update(rows=hot_rows, keep=keep, warm=warm_rows)
    if other >= 0:
        wo = f8.ref_weight(img, total, chunk, block, other, n, k)
        c.extra.update(wo=wo, other=xf @ wo.T)
        cool = img.copy()  # the clean image: every scale 2^96, so the hot and warm rows stay far below 2^127
        cool_scales = np.full(len(scales), 2.0 ** FP8_COOL_E, np.float32)
        cool[si[::block, None] + np.arange(4)] = cool_scales.view(np.uint8).reshape(-1, 4)
        c.extra.update(clean_img=cool)
    return c


BAD_ROW = {5: 3, 17: 16, 65: 64}  # M -> the row of x that holds the non-finite values


def _bad_positions(k):
    """Positions of a NaN, a +inf and a -inf in the bad row: the main loop where K has one, the K tail."""
    nsteps = k // 128
    tail0 = 128 * nsteps
    return (5, tail0 + 1, k - 2) if nsteps == 0 else (37, 128 * (nsteps - 1) + 70, tail0 + 9)


def nonfinite_x(x, xf, with_nan=True, row=None):
    """(x, xf) with a NaN (with_nan), a +inf and a -inf in row `row` (BAD_ROW[m] unless given)."""
    m, k = xf.shape
    r = BAD_ROW[m] if row is None else row
    bits = mx.bf16_tensor_bits(x).reshape(m, k).copy()
    pn, pp, pm = _bad_positions(k)
    if with_nan:
        bits[r, pn] = 0x7FC0
    bits[r, pp], bits[r, pm] = 0x7F80, 0xFF80
    return bits_x(bits)


def bad_row_expectation(xf_bad, wf, want_clean, row=None):
    """The expectation with the bad row summed element by element (inf * 0 and inf - inf are NaN)."""
    r = BAD_ROW[xf_bad.shape[0]] if row is None else row
    want = want_clean.copy()
    with np.errstate(invalid="ignore"):
        want[r] = (xf_bad[r][None, :] * wf).sum(1)
    assert not np.isfinite(want[r]).any()
    return want


def nonfinite_activations(fmt, n, k, m, block=128, seed=0, row=None):
    """A clean exact case (integers in [-8, 8], ordinary weights) of M = 5, 17 or 65 rows (any M with
    `row` given); extra["bad"] = {with_nan: (x, xf, want)} puts the non-finite values into one row of x."""
    row = BAD_ROW[m] if row is None else row
    x, xf = mx.int_x(m, k, 41 + seed + m)
    if fmt == "fp8":
        off, chunk, total = _fp8_layer(n, k, block)
        img = f8.handmade_image(total, chunk, block, 43 + seed + n + k)
        c = _linear_case(fmt, img, total, chunk, block, off, n, k, x, xf, 1.0, 2.0 ** -4)
    else:
        off, chunk, total = _mx_layer(n, k)
        img = mx.handmade_image(total, chunk, 43 + seed + n + k)
        c = _linear_case(fmt, img, total, chunk, 32, off, n, k, x, xf, 1.0, 2.0 ** -2)
    bad = {}
    for with_nan in (True, False):
        xb, xbf = nonfinite_x(x, xf, with_nan, row)
        bad[with_nan] = (xb, xbf, bad_row_expectation(xbf, c.wf, c.want, row))
    assert np.isnan(bad[True][2][row]).all()
    c.extra.update(bad=bad, row=row, keep=[i for i in range(m) if i != row])
    return c


def swiglu_clean(m, n, k, seed=0, chunk=1024):
    """An exact mxfp4_swiglu case: gate at element 224, up behind it after a gap."""
    gate = 32 * 7
    up = gate + n * k + 32 * 3
    total = up + n * k + 32 * 5
    img = mx.handmade_image(total, chunk, 51 + seed + n + k)
    x, xf = mx.int_x(m, k, 53 + seed + m)
    wg, wu = mx.ref_weight(img, total, chunk, gate, n, k), mx.ref_weight(img, total, chunk, up, n, k)
    return SwigluCase(img, total, chunk, gate, up, n, k, x, xf, wg, wu, xf @ wg.T, xf @ wu.T, 1.0, 2.0 ** -2, 2.0 ** -2)


def swiglu_nonfinite(n, k, m, seed=0, row=None):
    """swiglu_clean with extra["bad"] = {with_nan: (x, g, u)}: the non-finite values in one row of x."""
    return add_bad_rows(swiglu_clean(m, n, k, seed), row)


def add_bad_rows(c, row=None):
    """extra["bad"] = {with_nan: (x, g, u)} for a clean gated case (BAD_ROW[m] unless `row` is given)."""
    m = c.x.shape[0]
    row = BAD_ROW[m] if row is None else row
    bad = {}
    for with_nan in (True, False):
        xb, xbf = nonfinite_x(c.x, c.xf, with_nan, row)
        bad[with_nan] = (xb, bad_row_expectation(xbf, c.wg, c.g, row), bad_row_expectation(xbf, c.wu, c.u, row))
    c.extra.update(bad=bad, row=row, keep=[i for i in range(m) if i != row])
    return c


def silu_mul64(g, u):
    """silu(g) * u in float64 as the kernel writes it, g / (1 + exp(-g)) * u: g = -inf gives NaN."""
    with np.errstate(over="ignore", invalid="ignore"):
        return g / (1.0 + np.exp(-g)) * u


# ---------------------------------------------------------------- 3. far into a large layer

FAR_CHUNK = 64 * KiB
FAR_N, FAR_K = 48, 1056  # 50688 elements: longer than one chunk of 32768


@dataclass
class FarCase:
    """A small image S (`img`, `total_s` elements: three chunks and a short tail chunk) that lies
    behind c0 full chunks of a large layer which are never read: the layer has `src_bytes`, S
    starts at byte `base` of its packed image of `need` bytes, the parameter at element
    `elem_offset` (off_s in S)."""
    fmt: str
    block: int
    c0: int
    n: int                # rows of the parameter (FAR_N; 64 where two row tiles per wave are forced)
    img: np.ndarray
    total_s: int
    off_s: int
    x: torch.Tensor
    xf: np.ndarray
    wf: np.ndarray
    want: np.ndarray
    bits: np.ndarray      # reference bf16 bits of the parameter
    src_bytes: int = 0
    elem_offset: int = 0
    base: int = 0
    need: int = 0
    first_byte: int = 0   # packed bytes of the parameter's first and last code
    last_byte: int = 0
    up_s: int = -1        # swiglu: the up parameter in S (the gate is at off_s)
    wu: np.ndarray = None
    up_bits: np.ndarray = None
    chunks: int = 3       # full chunks of S

    def place(self, device):
        """The packed buffer on `device`: uninitialised below S."""
        buf = torch.empty(self.need, dtype=torch.uint8, device=device)
        buf[self.base:].copy_(torch.from_numpy(self.img))
        return buf


def far_pchunk(fmt, block):
    ce = FAR_CHUNK // 2
    return ce + ce // block * 4 if fmt == "fp8" else FAR_CHUNK // 4 + FAR_CHUNK // 64


def far_case(fmt, c0, off_s, m=5, block=128, seed=0, up_s=-1, n=48, chunks=3):
    """`chunks`: the full chunks of S, 3 unless a parameter of more rows (BN + 16 of a tiled kernel)
    or a gate / up pair behind a crossing has to fit."""
    ce = FAR_CHUNK // 2
    total_s = chunks * ce + 32 * 144  # the tail chunk holds 4608 elements (whole blocks of 128 and of 512)
    k = FAR_K
    assert off_s % 32 == 0 and max(off_s, up_s) + n * k <= total_s
    x, xf = mx.int_x(m, k, 61 + seed + m)
    pc = far_pchunk(fmt, block)
    src_bytes = c0 * FAR_CHUNK + 2 * total_s
    elem_offset = c0 * ce + off_s
    last = elem_offset + n * k - 1
    if fmt == "fp8":
        img = f8.handmade_image(total_s, FAR_CHUNK, block, 63 + seed + c0 % 1000)
        layer = f8.ref_layer_bits(img, total_s, FAR_CHUNK, block)
        need = int(_core.fp8_packed_size(src_bytes, FAR_CHUNK, block))
        fb, lb = (int(fp8_index(src_bytes // 2, FAR_CHUNK, block, e)[0]) for e in (elem_offset, last))
    else:
        img = mx.handmade_image(total_s, FAR_CHUNK, 63 + seed + c0 % 1000)
        layer = mx.ref_layer_bits(img, total_s, FAR_CHUNK)
        need = int(_core.mxfp4_packed_size(src_bytes, FAR_CHUNK))
        fb, lb = (int(mxfp4_index(src_bytes // 2, FAR_CHUNK, e)[0]) for e in (elem_offset, last))
    assert need == c0 * pc + img.size
    bits = layer[off_s: off_s + n * k]
    wf = mx.bits_to_f64(bits).reshape(n, k)
    c = FarCase(fmt, block, c0, n, img, total_s, off_s, x, xf, wf, xf @ wf.T, bits, src_bytes, elem_offset, c0 * pc,
                need, fb, lb)
    if up_s >= 0:
        c.up_s, c.up_bits = up_s, layer[up_s: up_s + n * k]
        c.wu = mx.bits_to_f64(c.up_bits).reshape(n, k)
    c.chunks = chunks
    return c


def far_linear(c, buf, **kw):
    if c.fmt == "fp8":
        return ops.fp8_linear(c.x.to(buf.device), buf, c.n, FAR_K, src_bytes=c.src_bytes, chunk_bytes=FAR_CHUNK,
                              block=c.block, elem_offset=c.elem_offset, **kw)
    return ops.mxfp4_linear(c.x.to(buf.device), buf, c.n, FAR_K, src_bytes=c.src_bytes, chunk_bytes=FAR_CHUNK,
                            elem_offset=c.elem_offset, **kw)


def far_swiglu(c, buf, **kw):
    if c.fmt == "fp8":
        return ops.fp8_swiglu(c.x.to(buf.device), buf, c.n, FAR_K, src_bytes=c.src_bytes, chunk_bytes=FAR_CHUNK,
                              block=c.block, gate_offset=c.elem_offset, up_offset=c.elem_offset - c.off_s + c.up_s, **kw)
    return ops.mxfp4_swiglu(c.x.to(buf.device), buf, c.n, FAR_K, src_bytes=c.src_bytes, chunk_bytes=FAR_CHUNK,
                            gate_offset=c.elem_offset, up_offset=c.elem_offset - c.off_s + c.up_s, **kw)


def far_unpack(c, buf, off_s=None):
    off = c.elem_offset - c.off_s + (c.off_s if off_s is None else off_s)
    if c.fmt == "fp8":
        return ops.fp8_unpack_range(buf, c.src_bytes, FAR_CHUNK, off, c.n * FAR_K, c.block)
    return ops.mxfp4_unpack_range(buf, c.src_bytes, FAR_CHUNK, off, c.n * FAR_K)


def crossing_c0(fmt, block, boundary, packed):
    """(c0, off_s) for which `boundary` (a power of two) lies inside the parameter: as an element
    index, or with `packed` as a byte of the packed image among the parameter's codes."""
    ce, pc = FAR_CHUNK // 2, far_pchunk(fmt, block)
    if not packed:
        return boundary // ce - 1, 32 * 700  # S starts one chunk before the boundary, the parameter crosses it
    c0 = boundary // pc
    p = boundary - c0 * pc  # the byte of S's first chunk
    per = 1 if fmt == "fp8" else 2  # elements per code byte
    assert 1024 <= p < ce // per  # among the codes of that chunk
    return c0, (p - 1024) * per // 32 * 32


# ---------------------------------------------------------------- 4. passes, strided output, views of x

def clean_case(fmt, m, n, k, block=128, seed=0):
    """An exact case on ordinary weights: integers in [-8, 8] against multiples of 2^-2 (MXFP4) or
    2^-4 (fp8)."""
    x, xf = mx.int_x(m, k, 71 + seed + m)
    if fmt == "fp8":
        off, chunk, total = _fp8_layer(n, k, block)
        img = f8.handmade_image(total, chunk, block, 73 + seed + n + k)
        return _linear_case(fmt, img, total, chunk, block, off, n, k, x, xf, 1.0, 2.0 ** -4)
    off, chunk, total = _mx_layer(n, k)
    img = mx.handmade_image(total, chunk, 73 + seed + n + k)
    return _linear_case(fmt, img, total, chunk, 32, off, n, k, x, xf, 1.0, 2.0 ** -2)


def strided_out(m, n, ld, dtype, device):
    """(buf, y): y = [m, n] with row stride ld inside a 0xA5-filled byte buffer, rows before and behind it."""
    es = 2 if dtype == torch.bfloat16 else 4
    lead = 3 * ld + 8
    buf = torch.full(((lead + (m + 3) * ld) * es,), 0xA5, dtype=torch.uint8, device=device)
    return buf, buf.view(dtype)[lead: lead + m * ld].view(m, ld)[:, :n]


def assert_untouched_outside(buf, m, n, ld, dtype):
    es = 2 if dtype == torch.bfloat16 else 4
    lead = 3 * ld + 8
    mask = torch.ones(buf.numel() // es, dtype=torch.bool)
    mask[lead: lead + m * ld].view(m, ld)[:, :n] = False
    outside = buf.cpu().view(-1, es)[mask]
    assert outside.numel() and bool((outside == 0xA5).all())


def x_views(x):
    """x [18, k] as the views the ops must take: {name: tensor}, all on x's device, all equal to
    x.view(2, 9, k) or x in value. "offset": contiguous, but 2 bytes off a 16-byte boundary."""
    m, k = x.shape
    wide = torch.zeros(m, k + 32, dtype=x.dtype, device=x.device)
    wide[:, 16: 16 + k] = x
    tr = x.t().contiguous().t()  # column-major
    flat = torch.zeros(m * k + 8, dtype=x.dtype, device=x.device)
    flat[1: 1 + m * k] = x.reshape(-1)
    off = flat[1: 1 + m * k].view(m, k)
    assert not wide[:, 16: 16 + k].is_contiguous() and not tr.is_contiguous() and off.is_contiguous()
    assert x.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 2
    return {"3d": x.view(2, 9, k), "sliced": wide[:, 16: 16 + k], "transposed": tr, "offset": off,
            "3d sliced": wide.view(2, 9, k + 32)[:, :, 16: 16 + k]}
