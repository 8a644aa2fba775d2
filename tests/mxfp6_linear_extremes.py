"""Case builders for ops.mxfp6_linear at its numeric and addressing extremes, in the manner of
linear_extremes.py (whose checks they use). A plain module: test_mxfp6_linear_extremes_host.py
runs the cases through the op's CPU route, test_gpu_mxfp6_linear_extremes.py through the gfx950
kernel.

The reference is the numpy ref_unpack per chunk of the layer (ref_weight of
test_mxfp6_linear_host.py) followed by a float64 matmul; nothing here goes through the ops. Every
case carries the units of linear_extremes.prove_exact: x holds multiples of `ux`, W multiples of
`uw`, and (|x| @ |W|^T).max() < 2^24 ux uw, so an f32 accumulation in any order is exact."""
from dataclasses import dataclass, field

import numpy as np
import torch

from distributed_llm_dissemination_amd import _core, ops

import linear_extremes as le
import test_mxfp6_linear_host as m6
from linear_extremes import (BAD_ROW, FAR_CHUNK, FAR_K, FAR_N, ROW_TILES_SHAPE, SHAPES, assert_bf16_is_rounded,  # noqa: F401
                             assert_f32_equal, assert_rows_bit_equal, assert_untouched_outside, f32_to_bf16_bits,
                             nonfinite_x, prove_exact, scaled_ints, strided_out, subnormal_x, x_views)
from test_mxfp6_host import codes_to_bytes

KiB = 1 << 10


@dataclass
class Case:
    img: np.ndarray       # the packed image of the whole layer
    total: int            # elements of the layer
    chunk: int
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


def run_linear(c, device, x=None, img=None, **kw):
    """ops.mxfp6_linear of the case on `device` ("cpu": the CPU route), optionally with another x or image."""
    x = c.x if x is None else x
    p = img if torch.is_tensor(img) else torch.from_numpy(c.img if img is None else img).to(device)
    return ops.mxfp6_linear(x.to(device), p, c.n, c.k, src_bytes=2 * c.total, chunk_bytes=c.chunk, elem_offset=c.off,
                            **kw)


def mxfp6_index(total, chunk, elem):
    """(index of the first of the block's 24 bytes, index of its scale byte) of element `elem`:
    core/mxfp6.h's rule in plain arithmetic (an int or an int64 array)."""
    ce, pc = chunk // 2, chunk // 64 * 25
    c = elem // ce
    r = (elem - c * ce) // 32
    nb = np.minimum(ce, total - c * ce) // 32
    return c * pc + 24 * r, c * pc + 24 * nb + r


def _layer(n, k):
    """1024-B chunks (512 elements, 16 blocks: chunk edges inside rows), the parameter at element
    224 (an odd block) of a layer that goes on behind it."""
    off, chunk = 32 * 7, 1024
    return off, chunk, off + n * k + 32 * 5


def _case(img, total, chunk, off, n, k, x, xf, ux=0.0, uw=0.0, **extra):
    wf = m6.ref_weight(img, total, chunk, off, n, k)
    with np.errstate(invalid="ignore", over="ignore"):
        want = xf @ wf.T
    return Case(img, total, chunk, off, n, k, x, xf, wf, want, ux, uw, extra)


# ---------------------------------------------------------------- 1. the bottom of the range

def subnormal_weights(m, n, k, s, seed=0):
    """Scale bytes {0, 1, 2, 3} under every code: the weights are multiples of 2^-130 of magnitude
    at most 7.5 * 2^-124, bf16 subnormals or next to them. x: integers in [-8, 8] times 2^s.
    s = 100: the products are normal f32 (only the B operand is subnormal); s = 0: products and
    sums are f32 subnormals or next to them; s = -8: all products are (u = 2^-138 >= 2^-149).
    |sum| <= 1056 * 8 * 7.5 * 2^-124 * 2^s = 4 055 040 u < 2^24 u."""
    x, xf = scaled_ints(m, k, 31 * seed + m + k, s)
    off, chunk, total = _layer(n, k)
    img = m6.handmade_image(total, chunk, 7 + seed + n + k, scales=(0, 1, 2, 3))
    return _case(img, total, chunk, off, n, k, x, xf, 2.0 ** s, 2.0 ** -130)


def subnormal_activations(m, n, k, seed=0):
    """The mirror image: x holds bf16 subnormals (multiples of 2^-133 up to 127 * 2^-133), W lies
    under scale byte 227 (multiples of 2^97 up to 7.5 * 2^100). Only the A operand is subnormal;
    products and sums are normal f32. |sum| <= 1056 * 127 * 60 * 2^-36 = 8 046 720 u < 2^24 u."""
    x, xf = subnormal_x(m, k, 17 * seed + m + k)
    off, chunk, total = _layer(n, k)
    img = m6.handmade_image(total, chunk, 9 + seed + n + k, scales=(227,))
    return _case(img, total, chunk, off, n, k, x, xf, 2.0 ** -133, 2.0 ** 97)


# ---------------------------------------------------------------- 2. the top of the range

def _poison_rows(n, k):
    """(weight row, [(block of the row, scale byte, signs)]): blocks of the main loop (K >= 128)
    and of the K tail; "+" and "-" give a row of +-inf, both in one row a NaN."""
    nb = k // 32
    main, tail = (1 if nb > 4 else 0), nb - 1  # nb - 1 lies in the K tail (K % 128 != 0)
    return [(0, [(main, 254, "+")]), (n // 2 + 5, [(tail, 253, "-")]), (n - 1, [(main, 253, "+"), (tail, 254, "-")]),
            (n // 2 - 3, [(tail, 254, "+-")])]


def overflow(m, n, k, zeros=False, seed=0):
    """Scale bytes 253 and 254 in a few blocks of chosen weight rows. Under byte 253 the non-zero
    codes of those blocks have magnitudes 4 .. 7.5 only (4 * 2^126 = 2^128), under byte 254
    magnitudes 2 .. 7.5 (2 * 2^127): every non-zero weight there is +-inf in the reference and no
    finite product overflows on its own. x: integers in [1, 8] (with `zeros`: [0, 8], 0 * inf =
    NaN). The expectation of the poisoned rows is summed element by element in numpy;
    extra["clean"] is the same case on the unpoisoned image."""
    off, chunk, total = _layer(n, k)
    clean = m6.handmade_image(total, chunk, 11 + seed + n + k)
    x, xf = scaled_ints(m, k, 13 + seed + m, 0, 0 if zeros else 1, 8)
    img = clean.copy()
    rows = poison(img, total, chunk, off, n, k, seed)
    c = _case(img, total, chunk, off, n, k, x, xf, 1.0, 2.0 ** -4)
    cl = _case(clean, total, chunk, off, n, k, x, xf, 1.0, 2.0 ** -4)
    keep = check_poisoned(c.wf, cl.wf, rows)
    with np.errstate(invalid="ignore"):
        for r in rows:
            c.want[:, r] = (xf * c.wf[r][None, :]).sum(1)
    assert not np.isfinite(c.want[:, rows]).any() and np.array_equal(c.want[:, keep], cl.want[:, keep])
    c.extra.update(clean=cl, rows=rows, keep=keep)
    return c


def poison(img, total, chunk, off, n, k, seed=0):
    """Writes the blocks of _poison_rows into the [n, k] parameter at element `off` of `img`;
    returns the poisoned weight rows."""
    rng = np.random.default_rng(seed + 5)
    rows = []
    for r, blocks in _poison_rows(n, k):
        rows.append(r)
        for b, sb, signs in blocks:
            mags = np.arange(24 if sb == 253 else 16, 32)
            pool = np.concatenate([[0] if s == "+" else [32] for s in signs]
                                  + [mags if s == "+" else mags | 32 for s in signs])
            codes = rng.choice(pool, 32)
            take = min(len(pool), 32)
            codes[:take] = rng.permutation(pool)[:take]  # every listed code once, as far as 32 places go
            qi, si = mxfp6_index(total, chunk, off + r * k + 32 * b)
            img[qi: qi + 24] = codes_to_bytes(codes[None, :]).reshape(-1)
            img[si] = sb
    return rows


def check_poisoned(wf, wf_clean, rows):
    """The poisoned rows hold +-inf and otherwise ordinary weights, the others are those of the
    clean image; returns the kept rows."""
    keep = np.setdiff1d(np.arange(len(wf)), rows)
    assert np.isinf(wf[rows]).any(1).all() and np.isfinite(wf[keep]).all()
    assert np.array_equal(wf[keep], wf_clean[keep])
    fin = np.abs(wf[rows][np.isfinite(wf[rows])])
    assert fin.max() <= 15  # what stays finite in those rows is ordinary
    return keep


bad_row_expectation = le.bad_row_expectation


def nonfinite_activations(n, k, m, seed=0, row=None):
    """A clean exact case of M = 5, 17 or 65 rows (any M with `row` given); extra["bad"] =
    {with_nan: (x, xf, want)} puts a NaN (with_nan), a +inf and a -inf into one row of x
    (linear_extremes.nonfinite_x)."""
    c = clean_case(m, n, k, seed)
    row = BAD_ROW[m] if row is None else row
    bad = {}
    for with_nan in (True, False):
        xb, xbf = nonfinite_x(c.x, c.xf, with_nan, row)
        bad[with_nan] = (xb, xbf, bad_row_expectation(xbf, c.wf, c.want, row))
    assert np.isnan(bad[True][2][row]).all()
    c.extra.update(bad=bad, row=row, keep=[i for i in range(m) if i != row])
    return c


# ---------------------------------------------------------------- 3. far into a large layer

FAR_PCHUNK = FAR_CHUNK // 64 * 25


@dataclass
class FarCase:
    """A small image S (`img`, `total_s` elements: three chunks and a short tail chunk) that lies
    behind c0 full chunks of a large layer which are never read: the layer has `src_bytes`, S
    starts at byte `base` of its packed image of `need` bytes, the parameter at element
    `elem_offset` (off_s in S)."""
    c0: int
    n: int
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
    first_byte: int = 0   # packed bytes of the first code byte of the parameter's first and last block
    last_byte: int = 0
    up_s: int = -1        # swiglu: the up parameter in S (the gate is at off_s)
    wu: np.ndarray = None
    up_bits: np.ndarray = None
    chunks: int = 3       # full chunks of S
    fmt: str = "mxfp6"
    block: int = 32

    def place(self, device):
        """The packed buffer on `device`: uninitialised below S."""
        buf = torch.empty(self.need, dtype=torch.uint8, device=device)
        buf[self.base:].copy_(torch.from_numpy(self.img))
        return buf


def far_case(c0, off_s, m=5, seed=0, n=FAR_N, up_s=-1, chunks=3):
    """`chunks`: the full chunks of S, 3 unless a parameter of more rows (BN + 16 of the tiled
    kernel) or a gate / up pair behind a crossing has to fit."""
    ce = FAR_CHUNK // 2
    total_s = chunks * ce + 32 * 143  # the tail chunk holds an odd number of blocks
    k = FAR_K
    assert off_s % 32 == 0 and max(off_s, up_s) + n * k <= total_s
    x, xf = m6.int_x(m, k, 61 + seed + m)
    src_bytes = c0 * FAR_CHUNK + 2 * total_s
    elem_offset = c0 * ce + off_s
    img = m6.handmade_image(total_s, FAR_CHUNK, 63 + seed + c0 % 1000)
    need = int(_core.mxfp6_packed_size(src_bytes, FAR_CHUNK))
    assert need == c0 * FAR_PCHUNK + img.size
    fb, lb = (int(mxfp6_index(src_bytes // 2, FAR_CHUNK, e)[0]) for e in (elem_offset, elem_offset + n * k - 1))
    layer = m6.ref_layer_bits(img, total_s, FAR_CHUNK)
    bits = layer[off_s: off_s + n * k]
    wf = m6.bits_to_f64(bits).reshape(n, k)
    c = FarCase(c0, n, img, total_s, off_s, x, xf, wf, xf @ wf.T, bits, src_bytes, elem_offset, c0 * FAR_PCHUNK, need,
                fb, lb, chunks=chunks)
    if up_s >= 0:
        c.up_s, c.up_bits = up_s, layer[up_s: up_s + n * k]
        c.wu = m6.bits_to_f64(c.up_bits).reshape(n, k)
    return c


def far_linear(c, buf, **kw):
    return ops.mxfp6_linear(c.x.to(buf.device), buf, c.n, FAR_K, src_bytes=c.src_bytes, chunk_bytes=FAR_CHUNK,
                            elem_offset=c.elem_offset, **kw)


def far_swiglu(c, buf, **kw):
    return ops.mxfp6_swiglu(c.x.to(buf.device), buf, c.n, FAR_K, src_bytes=c.src_bytes, chunk_bytes=FAR_CHUNK,
                            gate_offset=c.elem_offset, up_offset=c.elem_offset - c.off_s + c.up_s, **kw)


def far_unpack(c, buf, off_s=None):
    off = c.elem_offset - c.off_s + (c.off_s if off_s is None else off_s)
    return ops.mxfp6_unpack_range(buf, c.src_bytes, FAR_CHUNK, off, c.n * FAR_K)


def crossing_c0(boundary, packed):
    """(c0, off_s) for which `boundary` (a power of two) lies inside the parameter: as an element
    index, or with `packed` as a byte of the packed image among the parameter's codes."""
    ce = FAR_CHUNK // 2
    if not packed:
        return boundary // ce - 1, 32 * 700  # S starts one chunk before the boundary, the parameter crosses it
    c0 = boundary // FAR_PCHUNK
    p = boundary - c0 * FAR_PCHUNK  # the byte of S's first chunk
    assert 24 * 40 <= p < ce // 32 * 24  # among the codes of that chunk
    return c0, (p // 24 - 40) * 32


# ---------------------------------------------------------------- 4. passes, strided output, views of x

def clean_case(m, n, k, seed=0):
    """An exact case on ordinary weights: integers in [-8, 8] against multiples of 2^-4 up to 15."""
    x, xf = m6.int_x(m, k, 71 + seed + m)
    off, chunk, total = _layer(n, k)
    img = m6.handmade_image(total, chunk, 73 + seed + n + k)
    return _case(img, total, chunk, off, n, k, x, xf, 1.0, 2.0 ** -4)
