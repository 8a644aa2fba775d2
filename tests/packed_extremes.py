"""The cases of linear_extremes.py and mxfp6_linear_extremes.py for the entry points that came after
them: the fused gated kernels of the fp8 and MXFP6 formats (ops.fp8_swiglu, ops.mxfp6_swiglu) and
the many-row kernels (tiled=True of the six packed ops). A plain module: test_packed_extremes_host.py
runs the cases through the ops' CPU route, test_gpu_swiglu_extremes.py and
test_gpu_tiled_extremes.py through the gfx950 kernels.

One `PF` per format gives the three formats one signature; the linear builders are those of the two
older modules, the gated builders for fp8 and MXFP6 are new here (MXFP4's are linear_extremes.py's).
The reference is each format's numpy ref_unpack per chunk (ref_weight / ref_layer_bits of the host
test modules) followed by a float64 matmul; nothing of an expectation goes through the ops. Every
case carries the units of linear_extremes.prove_exact, so g and u are exact in f32 in any order."""
from dataclasses import dataclass, field

import numpy as np
import torch

from distributed_llm_dissemination_amd import _core, ops

import linear_extremes as le
import mxfp6_linear_extremes as e6
import test_fp8_linear_host as f8
import test_mxfp4_linear_host as mx
import test_mxfp6_linear_host as m6
from linear_extremes import FAR_CHUNK, FAR_K, FAR_N, prove_exact  # noqa: F401
from test_gpu_mxfp4_swiglu import check_exact_regimes

GB = 10 ** 9
P2_31, P2_32 = 1 << 31, 1 << 32


class PF:
    """One packed format: "mxfp4", "mxfp6" or "fp8" with its scale block."""

    def __init__(self, name, block=32):
        self.name, self.block = name, block
        self.id = name if name != "fp8" else f"fp8b{block}"

    def __repr__(self):
        return self.id

    def tile(self):
        """(BM, BN) of the format's tiled kernel, from the bindings."""
        return tuple(getattr(_core, self.name + "_tiled_tile")())

    def padded(self, elems):
        return -(-elems // self.block) * self.block

    def kw(self):
        return dict(block=self.block) if self.name == "fp8" else {}

    def swiglu_op(self):
        return getattr(ops, self.name + "_swiglu")

    def image(self, total, chunk, seed, low=False):
        """An ordinary handmade image, or with `low` one at the bottom of bf16 (subnormal_weights of
        the two older modules: MXFP4 / MXFP6 scale bytes 0..3, fp8 E in -126..-124 under small codes)."""
        if self.name == "fp8":
            extra = dict(codes=le.FP8_LOW_CODES, exps=le.FP8_LOW_EXPS) if low else {}
            return f8.handmade_image(total, chunk, self.block, seed, **extra)
        mod = mx if self.name == "mxfp4" else m6
        return mod.handmade_image(total, chunk, seed, **(dict(scales=(0, 1, 2, 3)) if low else {}))

    def weight(self, img, total, chunk, off, n, k):
        if self.name == "fp8":
            return f8.ref_weight(img, total, chunk, self.block, off, n, k)
        return (mx if self.name == "mxfp4" else m6).ref_weight(img, total, chunk, off, n, k)

    def copy_param(self, dst, src, total, chunk, off, nelem):
        """Codes and scales of the blocks that hold elements [off, off + nelem), from image `src`."""
        e = off + np.arange(0, nelem, 32, dtype=np.int64)
        if self.name == "fp8":
            ci, si = le.fp8_index(total, chunk, self.block, e)
            idx = np.concatenate([(ci[:, None] + np.arange(32)).reshape(-1), (si[:, None] + np.arange(4)).reshape(-1)])
        elif self.name == "mxfp4":
            qi, si = le.mxfp4_index(total, chunk, e)
            idx = np.concatenate([(qi[:, None] + np.arange(16)).reshape(-1), si])
        else:
            qi, si = e6.mxfp6_index(total, chunk, e)
            idx = np.concatenate([(qi[:, None] + np.arange(24)).reshape(-1), si])
        dst[idx] = src[idx]

    # the units of ordinary and of low weights
    @property
    def uw(self):
        return 2.0 ** -2 if self.name == "mxfp4" else 2.0 ** -4

    @property
    def uw_low(self):
        return {"mxfp4": 2.0 ** -128, "mxfp6": 2.0 ** -130, "fp8": 2.0 ** -133}[self.name]


FORMATS = [PF("mxfp4"), PF("mxfp6"), PF("fp8", 32), PF("fp8", 128)]
GLU_FORMATS = FORMATS[1:]  # the fused kernels that linear_extremes.py does not reach


# ---------------------------------------------------------------- linear cases, by format

def subnormal_weights(f, m, n, k, s):
    return e6.subnormal_weights(m, n, k, s) if f.name == "mxfp6" else le.subnormal_weights(f.name, m, n, k, s, f.block)


def subnormal_activations(f, m, n, k):
    return e6.subnormal_activations(m, n, k) if f.name == "mxfp6" else le.subnormal_activations(f.name, m, n, k, f.block)


def overflow(f, m, n, k, zeros=False):
    """Scale bytes 253 / 254 (MXFP4, MXFP6; extra["clean"]) or E = 120 (fp8; `zeros` has no meaning)."""
    if f.name == "fp8":
        return le.fp8_overflow(m, n, k, f.block)
    return e6.overflow(m, n, k, zeros) if f.name == "mxfp6" else le.mxfp4_overflow(m, n, k, zeros)


def nonfinite_activations(f, n, k, m, row=None):
    if f.name == "mxfp6":
        return e6.nonfinite_activations(n, k, m, row=row)
    return le.nonfinite_activations(f.name, n, k, m, f.block, row=row)


def clean_case(f, m, n, k):
    return e6.clean_case(m, n, k) if f.name == "mxfp6" else le.clean_case(f.name, m, n, k, f.block)


def run_linear(c, device, **kw):
    return (e6 if isinstance(c, e6.Case) else le).run_linear(c, device, **kw)


def subnormal_shares(c):
    """linear_extremes.subnormal_shares for a linear case of any format."""
    return le.subnormal_shares(c)


def flushed(a):
    """`a` with everything below 2^-126 in magnitude (an f32 or bf16 subnormal) made zero."""
    return np.where(np.abs(a) < 2.0 ** -126, 0.0, a)


def flushed_expectation(xf, wf, rows=4):
    """x W^T of the first `rows` rows by a datapath that flushes subnormal operands and subnormal
    products to zero."""
    prod = flushed(flushed(xf[:rows])[:, None, :] * flushed(wf)[None, :, :])
    return prod.sum(-1)


# ---------------------------------------------------------------- gated cases

@dataclass
class GluCase:
    f: PF
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

    @property
    def m(self):
        return self.x.shape[0]


def _from_mxfp4(c):
    return GluCase(FORMATS[0], c.img, c.total, c.chunk, c.gate, c.up, c.n, c.k, c.x, c.xf, c.wg, c.wu, c.g, c.u, c.ux,
                   c.ug, c.uu, c.extra)


def run_swiglu(c, device, x=None, img=None, **kw):
    x = c.x if x is None else x
    p = img if torch.is_tensor(img) else torch.from_numpy(c.img if img is None else img).to(device)
    return c.f.swiglu_op()(x.to(device), p, c.n, c.k, src_bytes=2 * c.total, chunk_bytes=c.chunk, gate_offset=c.gate,
                           up_offset=c.up, **c.f.kw(), **kw)


def prove_swiglu(c, cols=None):
    cols = slice(None) if cols is None else cols
    prove_exact(c.xf, c.wg[cols], c.ux, c.ug, c.g[:, cols])
    prove_exact(c.xf, c.wu[cols], c.ux, c.uu, c.u[:, cols])


def prove_warm(c):
    """fp8 swiglu_overflow: the warm rows of the hot parameter (finite at E = 120, multiples of 2^117)
    and the same rows of the cool one are exact too, so those columns stay in the exact regimes."""
    warm = c.extra.get("warm")
    if warm is None:
        return
    hot_is_gate = c.extra["which"] == "gate"
    wh, sh, wc, sc = (c.wg, c.g, c.wu, c.u) if hot_is_gate else (c.wu, c.u, c.wg, c.g)
    prove_exact(c.xf, wh[warm], 1.0, 2.0 ** 117, sh[:, warm])
    prove_exact(c.xf, wc[warm], c.ux, c.ug, sc[:, warm])


def check_regimes_to_inf(y32, g, u):
    """check_exact_regimes where f32(g) * f32(u) may itself overflow (fp8 under 2^96 and 2^120): the
    expected value of the g >= 18 regime is then +-inf, and numpy's warning about it is not news."""
    with np.errstate(over="ignore"):
        return check_exact_regimes(y32, g, u)


# MXFP6 with and without zeros in x (0 * inf); fp8's overflow comes from finite weights, x stays in [1, 8]
GLU_OVERFLOW = [(FORMATS[1], False), (FORMATS[1], True), (FORMATS[2], False), (FORMATS[3], False)]
GLU_OVERFLOW_IDS = [f.id + (" zeros in x" if z else "") for f, z in GLU_OVERFLOW]


def glu_layout(f, n, k):
    """(chunk, gate, up, total): the gate at element 224, the up behind it after a gap of 96
    elements and one scale block (no scale block holds weights of both), the layer going on behind
    both. 1 KiB chunks (fp8: 4 KiB): chunk edges fall inside rows."""
    chunk, gate = (4096 if f.name == "fp8" else 1024), 32 * 7
    up = gate + n * k + 32 * 3 + (f.block if f.name == "fp8" else 0)
    return chunk, gate, up, f.padded(up + n * k + 32 * 5 + (f.block if f.name == "fp8" else 0))


def _glu_case(f, img, total, chunk, gate, up, n, k, x, xf, ux, ug, uu, **extra):
    wg, wu = f.weight(img, total, chunk, gate, n, k), f.weight(img, total, chunk, up, n, k)
    with np.errstate(invalid="ignore", over="ignore"):
        g, u = xf @ wg.T, xf @ wu.T
    return GluCase(f, img, total, chunk, gate, up, n, k, x, xf, wg, wu, g, u, ux, ug, uu, extra)


def swiglu_clean(f, m, n, k, seed=0):
    """An exact gated case on ordinary weights: integers in [-8, 8] against multiples of 2^-4."""
    if f.name == "mxfp4":
        return _from_mxfp4(le.swiglu_clean(m, n, k, seed))
    chunk, gate, up, total = glu_layout(f, n, k)
    img = f.image(total, chunk, 51 + seed + n + k)
    x, xf = mx.int_x(m, k, 53 + seed + m)
    return _glu_case(f, img, total, chunk, gate, up, n, k, x, xf, 1.0, f.uw, f.uw)


GLU_S = 104  # x = integers times 2^104 in the fp8 and MXFP6 cases (MXFP4: linear_extremes.SWIGLU_S)


def swiglu_subnormal(f, which, m, n, k, seed=0):
    """The `which` ("gate" or "up") weights at the bottom of bf16 - MXFP6 scale bytes {0..3}
    (multiples of 2^-130 up to 7.5 * 2^-124), fp8 E in {-126, -125, -124} under magnitude bytes up to
    0x1F (multiples of 2^-133, all bf16 subnormals) - and the other ordinary (multiples of 2^-4 up to
    15, fp8 30). One x feeds both products, so x = integers in [-8, 8] times 2^104: the products with
    the low weights are multiples of 2^-26 (fp8 2^-29) whose sums stay below 1056 * 8 * 7.5 * 2^-20 <
    2^-3, normal f32 and exact; the other sums are multiples of 2^100 below 1056 * 8 * 30 * 2^104 <
    2^122, finite and exact. MXFP4: linear_extremes.swiglu_subnormal."""
    if f.name == "mxfp4":
        return _from_mxfp4(le.swiglu_subnormal(which, m, n, k, seed))
    chunk, gate, up, total = glu_layout(f, n, k)
    img = f.image(total, chunk, 5 + seed + n + k)
    f.copy_param(img, f.image(total, chunk, 6 + seed + n + k, low=True), total, chunk, gate if which == "gate" else up,
                 n * k)
    x, xf = le.scaled_ints(m, k, 3 + seed + m, GLU_S)
    ug, uu = (f.uw_low, f.uw) if which == "gate" else (f.uw, f.uw_low)
    return _glu_case(f, img, total, chunk, gate, up, n, k, x, xf, 2.0 ** GLU_S, ug, uu, which=which)


def swiglu_nonfinite(f, n, k, m, row=None):
    """swiglu_clean with extra["bad"] = {with_nan: (x, g, u)}: NaN, +inf and -inf in one row of x."""
    return le.add_bad_rows(swiglu_clean(f, m, n, k), row)


def silu_mul_f32(g, u):
    """silu(g) * u as linear_extremes.silu_mul64 writes it, with the one step of the f32 epilogue
    that changes the class of a result: expf(-g) is +inf from -g = 88.75 on (e^88.75 = 1.027 FLT_MAX;
    e^88.6875 = 0.965 FLT_MAX is still finite, and g is a multiple of 2^-4), so g / (1 + inf) is -0
    there and -0 * (+-inf) is NaN, where float64 keeps a tiny negative quotient down to g = -709. Used
    only for elements whose u is not finite; for a non-finite g the two agree."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.where(-g >= 88.75, np.inf, np.exp(-g))
        return g / (1.0 + e) * u


def swiglu_overflow(f, which, m, n, k, zeros=False):
    """The top of the range in the `which` parameter of a gated pair, the other parameter ordinary.
    MXFP6: scale bytes 253 / 254 in the rows of mxfp6_linear_extremes._poison_rows (x integers in
    [1, 8], with `zeros` [0, 8]). fp8: the hot and warm rows of linear_extremes.fp8_overflow at
    E = 120, every other weight under 2^96. extra: rows (columns of y that are not finite), keep
    (columns whose weights are those of extra["clean_img"]), want (float64 [m, len(rows)], from
    silu_mul_f32 of the reference g and u per element)."""
    chunk, gate, up, total = glu_layout(f, n, k)
    hot, cool = (gate, up) if which == "gate" else (up, gate)
    if f.name == "fp8":
        lc = le.fp8_overflow(m, n, k, f.block, layer=(hot, chunk, total), other=cool)
        c = _glu_case(f, lc.img, total, chunk, gate, up, n, k, lc.x, lc.xf, 1.0, lc.uw, lc.uw,
                      clean_img=lc.extra["clean_img"], rows=lc.extra["rows"], keep=lc.extra["keep"],
                      warm=lc.extra["warm"], which=which)
        poisoned = lc.want  # the hot parameter's x W^T with the sums beyond 2^129 as +-inf
        assert np.array_equal(lc.extra["wo"], c.wu if which == "gate" else c.wg)
    else:
        assert f.name == "mxfp6"
        clean = f.image(total, chunk, 11 + n + k)
        x, xf = le.scaled_ints(m, k, 13 + m, 0, 0 if zeros else 1, 8)
        img = clean.copy()
        rows = e6.poison(img, total, chunk, hot, n, k)
        c = _glu_case(f, img, total, chunk, gate, up, n, k, x, xf, 1.0, f.uw, f.uw, clean_img=clean, rows=rows,
                      which=which)
        wh = c.wg if which == "gate" else c.wu
        c.extra["keep"] = e6.check_poisoned(wh, f.weight(clean, total, chunk, hot, n, k), rows)
        poisoned = (c.g if which == "gate" else c.u).copy()
        with np.errstate(invalid="ignore"):
            for r in rows:
                poisoned[:, r] = (xf * wh[r][None, :]).sum(1)
    if which == "gate":
        c.g = poisoned
    else:
        c.u = poisoned
    rows = c.extra["rows"]
    assert not np.isfinite(poisoned[:, rows]).any()
    c.extra["want"] = silu_mul_f32(c.g[:, rows], c.u[:, rows])
    assert not np.isfinite(c.extra["want"]).any()
    return c


# ---------------------------------------------------------------- far into a large layer

def far_case(f, c0, off_s, **kw):
    """linear_extremes.far_case / mxfp6_linear_extremes.far_case by format (`up_s`: a gated pair)."""
    if f.name == "mxfp6":
        return e6.far_case(c0, off_s, **kw)
    return le.far_case(f.name, c0, off_s, block=f.block, **kw)


def crossing_c0(f, boundary, packed):
    return e6.crossing_c0(boundary, packed) if f.name == "mxfp6" else le.crossing_c0(f.name, f.block, boundary, packed)


def _far_mod(c):
    return e6 if isinstance(c, e6.FarCase) else le


def far_linear(c, buf, **kw):
    return _far_mod(c).far_linear(c, buf, **kw)


def far_swiglu(c, buf, **kw):
    return _far_mod(c).far_swiglu(c, buf, **kw)


def far_unpack(c, buf, off_s=None):
    return _far_mod(c).far_unpack(c, buf, off_s)


def far_up_first_byte(c):
    """Packed byte of the up parameter's first code."""
    e = c.elem_offset - c.off_s + c.up_s
    if c.fmt == "fp8":
        return int(le.fp8_index(c.src_bytes // 2, FAR_CHUNK, c.block, e)[0])
    return int((le.mxfp4_index if c.fmt == "mxfp4" else e6.mxfp6_index)(c.src_bytes // 2, FAR_CHUNK, e)[0])


def wrapped_inside(c):
    """The condition under which a wrong kernel shows as a wrong value, not as a fault: whatever a
    truncation to 31 or 32 bits makes of the first element or first packed byte of the parameter
    (of the up too) is either unchanged or, with the whole parameter behind it, inside the
    never-read low part of the packed buffer (2 bytes per element bound every format's codes and
    scales)."""
    ce, pc, span = FAR_CHUNK // 2, c.base // c.c0, c.n * FAR_K
    elems, byts = [c.elem_offset], [c.first_byte]
    if c.up_s >= 0:
        elems.append(c.elem_offset - c.off_s + c.up_s)
        byts.append(far_up_first_byte(c))
    for mod in (P2_31, P2_32):
        for e in elems:
            if e % mod != e and ((e % mod + span) // ce + 1) * pc > c.base:
                return False
        for b in byts:
            if b % mod != b and b % mod + 2 * span + pc > c.base:
                return False
    return 2 * span + pc < c.base  # what wraps from inside the parameter lands in [0, span)


def late32(c, up=False):
    """x W^T with the parameter taken 32 elements late in S: what a kernel one block off computes."""
    layer = _layer_bits(c)
    o = (c.up_s if up else c.off_s) + 32
    return c.xf @ mx.bits_to_f64(layer[o: o + c.n * FAR_K]).reshape(c.n, FAR_K).T


def _layer_bits(c):
    if c.fmt == "fp8":
        return f8.ref_layer_bits(c.img, c.total_s, FAR_CHUNK, c.block)
    return (mx if c.fmt == "mxfp4" else m6).ref_layer_bits(c.img, c.total_s, FAR_CHUNK)


# (format, c0, boundary, packed, rows, gated): the far cases of the gated decode kernels and of all
# tiled kernels. c0 given: everything behind 2^32 elements and bytes. boundary given: it lies
# inside the parameter (the gate), as an element index or as a byte of the packed image.
F4, F6, F8 = FORMATS[0], FORMATS[1], FORMATS[3]
FAR_GLU = {
    "mxfp6 behind 2^32 elements and bytes": (F6, 180_000, None, None, FAR_N),
    "mxfp6 element 2^31 inside the gate": (F6, None, P2_31, False, FAR_N),
    "mxfp6 packed byte 2^32 inside the gate": (F6, None, P2_32, True, FAR_N),
    "mxfp6 element 2^31 inside the gate, 64 rows, 2 row tiles per wave": (F6, None, P2_31, False, 64),
    "fp8 behind 2^32 elements and bytes": (F8, 140_000, None, None, FAR_N),
    "fp8 element 2^31 inside the gate": (F8, None, P2_31, False, FAR_N),
    "fp8 packed byte 2^31 inside the gate": (F8, None, P2_31, True, FAR_N),
    "fp8 packed byte 2^31 inside the gate, 64 rows, 2 row tiles per wave": (F8, None, P2_31, True, 64),
}
FAR_GLU_MXFP4 = {  # test_gpu_linear_extremes.test_far_swiglu's two, for the tiled kernel
    "mxfp4 behind 2^32 elements and bytes": (F4, 250_000, None, None, FAR_N),
    "mxfp4 element 2^32 inside the gate": (F4, None, P2_32, False, FAR_N),
}


def far_glu_case(name, m=17, n=None, table=None):
    """The named gated far case: S of 6 full chunks, the gate where the name says and the up 64
    elements behind it (behind the boundary whenever the gate crosses one)."""
    f, c0, boundary, packed, rows = (table or {**FAR_GLU, **FAR_GLU_MXFP4})[name]
    n = rows if n is None else n
    gate = 32 * 3
    if c0 is None:
        c0, gate = crossing_c0(f, boundary, packed)
    chunks = -(-(gate + 2 * n * FAR_K + 64) // (FAR_CHUNK // 2))
    c = far_case(f, c0, gate, m=m, n=n, up_s=gate + n * FAR_K + 64, chunks=max(chunks, 6))
    assert_far_position(c, boundary, packed)
    return c


def assert_far_position(c, boundary, packed):
    """The boundary lies where the case's name says, on the case's own arithmetic."""
    last_elem = c.elem_offset + c.n * FAR_K
    if boundary is None:
        assert c.elem_offset > P2_32 and c.first_byte > P2_32
    elif packed:
        assert c.first_byte < boundary < c.last_byte
    else:
        assert c.elem_offset < boundary < last_elem
    if c.up_s >= 0 and boundary is not None:
        up_elem = c.elem_offset - c.off_s + c.up_s
        assert up_elem >= last_elem and (far_up_first_byte(c) > boundary if packed else up_elem > boundary)


# ---------------------------------------------------------------- rows of x and of y beyond 32 bits

BIG_K, BIG_N = 1056, 16


def big_x_rows(bm):
    """M with M * BIG_K just beyond 2^32 elements, and the checked rows: the first tile, the tiles
    that hold element 2^31, byte 2^32 (the same row: 2 bytes per element) and element 2^32 of x with
    one tile before and behind each, and the last, partial tile."""
    m = P2_32 // BIG_K + 2 * bm + 5
    assert m * BIG_K > P2_32 and m % bm
    return m, _windows(m, bm, [P2_31 // BIG_K, P2_32 // 2 // BIG_K, (P2_32 - 1) // BIG_K, P2_32 // BIG_K])


def big_y_rows(bm, ld):
    """M = 2^22 + 5 rows of `ld` f32: M * ld beyond 2^31 elements and 4 M ld beyond 2^32 bytes; the
    checked rows lie around element 2^30 (byte 2^32), element 2^31 and in the first and last tile."""
    m = (1 << 22) + 5
    assert m * ld > P2_31 and 4 * m * ld > P2_32 and m % bm
    return m, _windows(m, bm, [(1 << 30) // ld, P2_31 // ld])


def _windows(m, bm, rows):
    """Sorted, merged [r0, r1) windows of whole tiles: tile 0, the last tile, and the tile of each
    of `rows` with its two neighbours."""
    tiles = {0, (m - 1) // bm}
    for r in rows:
        tiles |= {t for t in (r // bm - 1, r // bm, r // bm + 1) if 0 <= t <= (m - 1) // bm}
    out = []
    for t in sorted(tiles):
        r0, r1 = t * bm, min((t + 1) * bm, m)
        if out and out[-1][1] == r0:
            out[-1] = (out[-1][0], r1)
        else:
            out.append((r0, r1))
    return out
