"""The four many-row kernels at the K depths and grids they are served at: mxfp4_tiled.hip,
fp8_tiled.hip and mxfp6_tiled.hip (tiled=True of the packed ops) and mxfp4_mx.hip (act="mxfp8", the
W4A8 route). Each has one launch shape - 128 x 128 tiles of y, one step per 128 k through a two-image
LDS pipeline, a tail step for K % 128, workgroups dealt to the XCDs by lid = xcd q8 + min(xcd, r8) +
(b >> 3) - and the older files run it at K <= 1056 and at most 66 workgroups. A plain module:
test_tiled_depth_grid_host.py holds the table to what it claims and proves every exact case on the
reference alone, test_gpu_tiled_depth_grid.py runs it on gfx950.

VARIANTS: the four tiled formats of packed_extremes.FORMATS and "w4a8" (MXFP4 weights, act="mxfp8").
BM, BN come from the bindings; a gated kernel covers BN / 2 columns of y per workgroup, so its N is
written with BN / 2 and gives the same workgroup counts. CUS = 256.

cases(variant, gated), as (M, N, K):

  depth   M = BM + 1, N = BN + 16 (four workgroups); K = 256 (two steps, no tail), 448 (three steps
          and two blocks), 640 (five steps), 4096 (32 steps), 4192 (32 steps and three blocks), 8160
          (63 steps and three blocks: the tail reads image 1), 28672 (224 steps), 53248 (416 steps,
          llama3.1-405b's down_proj). Linear: all eight; gated: 448, 8160, 28672; W4A8 linear: 448,
          4192, 28672; W4A8 gated: 448, 8160.
  grid    K = 416 (three steps and one block). G1 = (2 BM, 256 BN): 512 workgroups, two per CU, r8 = 0,
          no partial tile. G2 = (2 BM + 5, 682 BN + 16): 3 x 683 = 2049 = 8 * 256 + 1 workgroups, r8 = 1,
          q8 = 256, more than four per CU (the most the LDS of any of the kernels allows), so a second
          round starts while the first is mid-K. G3 = (4 BM + 7, 50 BN + 16): 5 x 51 = 255, r8 = 7.
          Linear: all three; gated and W4A8 linear: G1, G2; W4A8 gated: G2.
  both    linear (2 BM + 5, 8192 + 16, 8192), gated (BM + 1, 2048 + 16, 4096), W4A8 linear
          (2 BM + 5, 4096 + 16, 8192).

Inputs are the existing builders: each format's handmade_image, its ref_layer_bits (numpy ref_unpack
per chunk, through decode_launch_matrix.layer_f64) and linear_extremes.scaled_ints; the expectation is
a float64 library matmul of the dequantized values. 1 MiB chunks; the parameter at element 224, a
gated pair's up 96 elements (and a scale block) behind the gate, the layer going on 64 elements behind
them. level(f, k) picks the widest inputs whose closed form hi wmax K < 2^24 uw holds: x integers in
[-8, 8], then [-2, 2], then [-2, 2] against an image narrowed through the builder's own arguments
(MXFP6: scale bytes 126, 127; fp8: codes of magnitude up to 3.75) so that |w| <= 7.5 - at K = 53248
that is 15 K = 798 720 < 2^20. Built.prove asserts that closed form and linear_extremes.prove_exact
on the inputs themselves, and for W4A8 that the host quantizer returns the integers unchanged: the
f32 result equals the float64 one in any summation order.

RANDOM: (BM + 1, BN + 16, 8160) and (BM + 1, 144, 28672) with x ~ N(0, 1) and weights ~ N(0, 1 / K)
packed by the codec (random_case); W4A8 also with the outlier x of
test_gpu_mxfp4_mx.test_outliers_within_f32_accumulation_error at the second shape."""
import hashlib
from dataclasses import dataclass

import numpy as np
import torch

from distributed_llm_dissemination_amd import _core, ops

import decode_launch_matrix as dm
import linear_extremes as le
import test_fp8_linear_host as f8
import test_mxfp4_linear_host as mx
import test_mxfp6_linear_host as m6
from packed_extremes import FORMATS
from test_mxfp4_mx_host import dequantize, host_quantize

MiB = 1 << 20
CHUNK = MiB
CUS = 256
VARIANTS = [f.id for f in FORMATS] + ["w4a8"]
DEPTH_K = [256, 448, 640, 4096, 4192, 8160, 28672, 53248]
# +-{0, 1 .. 3.75 in steps of 1/8}: under scales 2^-1 .. 2^1 multiples of 2^-4 of magnitude at most 7.5
FP8_NARROW = np.array([s | c for s in (0, 0x80) for c in [0] + list(range(0x38, 0x48))], dtype=np.uint8)
# (largest |x|, largest |w|, arguments of the format's handmade_image), widest first
LEVELS = {
    "mxfp4": [(8, 12.0, {}), (2, 12.0, {})],
    "mxfp6": [(8, 15.0, {}), (2, 15.0, {}), (2, 7.5, dict(scales=(126, 127)))],
    "fp8": [(8, 30.0, {}), (2, 30.0, {}), (2, 7.5, dict(codes=FP8_NARROW))],
}


def fmt(variant):
    """The PF of a variant; W4A8 reads MXFP4 weights."""
    return FORMATS[0] if variant == "w4a8" else next(f for f in FORMATS if f.id == variant)


def tile(variant):
    return tuple(_core.mxfp4_mx_tile()) if variant == "w4a8" else fmt(variant).tile()


@dataclass(frozen=True)
class Case:
    name: str
    tag: str      # "depth", "grid" or "both"
    gated: bool
    m: int
    n: int
    k: int

    @property
    def id(self):
        return ("glu " if self.gated else "lin ") + self.name


def cases(variant, gated):
    bm, bn = tile(variant)
    cols = bn // 2 if gated else bn
    w4a8 = variant == "w4a8"
    if w4a8:
        depth = [448, 8160] if gated else [448, 4192, 28672]
        grids = ["G2"] if gated else ["G1", "G2"]
    else:
        depth = [448, 8160, 28672] if gated else DEPTH_K
        grids = ["G1", "G2"] if gated else ["G1", "G2", "G3"]
    grid = {"G1": (2 * bm, 256 * cols), "G2": (2 * bm + 5, 682 * cols + 16), "G3": (4 * bm + 7, 50 * cols + 16)}
    out = [Case(f"K={k}", "depth", gated, bm + 1, cols + 16, k) for k in depth]
    out += [Case(g, "grid", gated, *grid[g], 416) for g in grids]
    if gated and not w4a8:
        out.append(Case("both", "both", True, bm + 1, 2048 + 16, 4096))
    elif not gated:
        out.append(Case("both", "both", False, 2 * bm + 5, (4096 if w4a8 else 8192) + 16, 8192))
    return out


EXACT = [(v, c) for v in VARIANTS for gated in (False, True) for c in cases(v, gated)]


def exact_id(p):
    return f"{p[0]} {p[1].id}"


def geometry(variant, c):
    """What the launcher and the kernel make of a case: mblocks, nblocks, nwg, q8, r8, nsteps, tail."""
    bm, bn = tile(variant)
    cols = bn // 2 if c.gated else bn
    mblocks, nblocks = -(-c.m // bm), -(-c.n // cols)
    nwg = mblocks * nblocks
    return dict(bm=bm, cols=cols, mblocks=mblocks, nblocks=nblocks, nwg=nwg, q8=nwg >> 3, r8=nwg & 7, nsteps=c.k >> 7,
                tail=(c.k >> 5) & 3, total_steps=(c.k >> 7) + ((c.k >> 5) & 3 > 0))


def remap(b, nwg):
    """tiled_x.h's xcd_remap (and mxfp4_tiled.hip's own copy) in Python."""
    q8, r8, xcd = nwg >> 3, nwg & 7, b & 7
    return xcd * q8 + min(xcd, r8) + (b >> 3)


# ---------------------------------------------------------------- inputs and expectations

def level(f, k):
    """The first of LEVELS whose closed form holds at this K."""
    for hi, wmax, extra in LEVELS[f.name]:
        if hi * wmax * k < 2.0 ** 24 * f.uw:
            return hi, wmax, extra
    raise AssertionError((f.id, k))


def image(f, total, seed, extra):
    if f.name == "fp8":
        return f8.handmade_image(total, CHUNK, f.block, seed, **extra)
    return (mx if f.name == "mxfp4" else m6).handmade_image(total, CHUNK, seed, **extra)


def layout(f, n, k, gated):
    """([offsets], total): the parameter at element 224; a gated pair's up behind the gate after a gap
    of 96 elements and one scale block; the layer goes on 64 elements behind them."""
    pad = f.block if f.name == "fp8" else 0
    offs = [32 * 7]
    if gated:
        offs.append(offs[0] + n * k + 32 * 3 + pad)
    return offs, f.padded(offs[-1] + n * k + 64)


def matmul64(xf, w, device="cpu"):
    """x W^T in float64 by a library GEMM: numpy's, or torch's on `device`. Returns a float64 tensor
    on `device` (cuda) or a numpy array (cpu)."""
    if device == "cpu":
        return xf @ w.T
    return torch.from_numpy(xf).to(device) @ torch.from_numpy(w).to(device).T


def steps_of(k):
    """[k0, k1) of every step of the K loop, the tail step included."""
    return [(k0, min(k0 + 128, k)) for k0 in range(0, k, 128)]


def tiles_any(a, bm, cols):
    """bool [mblocks, nblocks]: whether a workgroup's tile of the boolean array holds a True."""
    r = np.add.reduceat(a.astype(np.int64), np.arange(0, a.shape[0], bm), axis=0)
    return np.add.reduceat(r, np.arange(0, a.shape[1], cols), axis=1) > 0


def tile_digests(a, bm, cols):
    """One digest per workgroup tile, partial tiles padded with zeros to bm x cols."""
    out = []
    for r0 in range(0, a.shape[0], bm):
        for c0 in range(0, a.shape[1], cols):
            t = np.zeros((bm, cols))
            part = a[r0: r0 + bm, c0: c0 + cols]
            t[: part.shape[0], : part.shape[1]] = part
            out.append(hashlib.blake2b(t.tobytes(), digest_size=16).digest())
    return out


class Built:
    """One exact case with its inputs: f, img, total, offs, ws (float64 [n, k] per parameter), x, xf,
    hi, wmax; wants(device) is the float64 x W^T per parameter. Built once per (variant, case) and
    left unchanged."""

    def __init__(self, variant, c):
        self.variant, self.case, self.f = variant, c, fmt(variant)
        self.m, self.n, self.k, self.gated, self.w4a8 = c.m, c.n, c.k, c.gated, variant == "w4a8"
        f = self.f
        self.hi, self.wmax, extra = level(f, c.k)
        self.offs, self.total = layout(f, c.n, c.k, c.gated)
        seed = 1009 * VARIANTS.index(variant) + c.m + 3 * c.n + 7 * c.k + c.gated
        self.img = image(f, self.total, seed, extra)
        flat = dm.layer_f64(f, self.img, self.total, CHUNK)
        self.ws = [flat[o: o + c.n * c.k].reshape(c.n, c.k) for o in self.offs]
        self.x, self.xf = le.scaled_ints(c.m, c.k, seed + 11, 0, -self.hi, self.hi)
        self.geo = geometry(variant, c)
        self._wants = {}

    def wants(self, device="cpu"):
        if device not in self._wants:
            self._wants[device] = [matmul64(self.xf, w, device) for w in self.ws]
        return self._wants[device]

    def prove(self):
        """The closed form, linear_extremes.prove_exact on the inputs themselves and, for W4A8, that
        MXFP8 holds this x exactly."""
        f = self.f
        assert np.abs(self.xf).max() <= self.hi <= 8 and self.hi * self.wmax * self.k < 2.0 ** 24 * f.uw
        for w, want in zip(self.ws, self.wants()):
            assert np.abs(w).max() <= self.wmax
            le.prove_exact(self.xf, w, 1.0, f.uw, want)
        if self.w4a8:
            assert np.array_equal(dequantize(*host_quantize(self.x)), self.xf)

    def run(self, device, x=None, img=None, offs=None, n=None, linear_of=None, untiled=False, **kw):
        """The case's op on `device` ("cpu": the CPU route). x: other rows; offs, n: another window
        of weight rows; linear_of = 0 or 1: the variant's linear on the gate or the up parameter;
        untiled: the decode kernel with split_k=1."""
        x = self.x if x is None else x
        p = torch.from_numpy(self.img).to(device) if img is None else img
        offs, n = self.offs if offs is None else offs, self.n if n is None else n
        a = dict(src_bytes=2 * self.total, chunk_bytes=CHUNK, **self.f.kw(), **kw)
        a.update(dict(split_k=1) if untiled else dict(act="mxfp8") if self.w4a8 else dict(tiled=True))
        if self.gated and linear_of is None:
            return getattr(ops, self.f.name + "_swiglu")(x.to(device), p, n, self.k, gate_offset=offs[0],
                                                         up_offset=offs[1], **a)
        return getattr(ops, self.f.name + "_linear")(x.to(device), p, n, self.k, elem_offset=offs[linear_of or 0], **a)


# ---------------------------------------------------------------- random and outlier inputs at depth

def random_shapes(variant):
    bm, bn = tile(variant)
    return [(bm + 1, bn + 16, 8160), (bm + 1, 144, 28672)]


def outlier_x(m, k):
    """x = N(0, 1) * 2^j, j uniform in -14 .. 3 per element: the generator of
    test_gpu_mxfp4_mx.test_outliers_within_f32_accumulation_error, seed and all."""
    g = torch.Generator().manual_seed(7 * m + k)
    return (torch.randn(m, k, generator=g) * torch.exp2(torch.randint(-14, 4, (m, k), generator=g).float())).to(torch.bfloat16)


def pack_layer(f, flat, device):
    """The layer packed by ops.*_pack_layer on a GPU, by the host codec of the same layout on the CPU."""
    if device != "cpu":
        args = (CHUNK, f.block) if f.name == "fp8" else (CHUNK,)
        return getattr(ops, f.name + "_pack_layer")(flat.to(device), *args)
    raw = flat.view(torch.int16).numpy().tobytes()
    args = (CHUNK, f.block) if f.name == "fp8" else (CHUNK,)
    return torch.from_numpy(np.frombuffer(getattr(_core, f.name + "_pack_layer_host")(raw, *args), dtype=np.uint8).copy())


class Random:
    """x ~ N(0, 1) in bf16 (or outlier_x) and two [n, k] weights ~ N(0, 1 / k), one behind the other in
    a layer packed by the codec in 1 MiB chunks; want and bound for the first weight:
    |y - y_ref| <= K 2^-23 sum_k |x w|, for W4A8 over x^ (the host quantizer's bytes, dequantized in
    numpy) and w^."""

    def __init__(self, variant, m, n, k, device, outliers=False):
        self.variant, self.f, self.m, self.n, self.k, self.w4a8 = variant, fmt(variant), m, n, k, variant == "w4a8"
        g = torch.Generator().manual_seed(12 + k + VARIANTS.index(variant))
        self.x = outlier_x(m, k) if outliers else torch.randn(m, k, generator=g).to(torch.bfloat16)
        w = (torch.randn(2 * n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
        self.total = 2 * n * k
        assert self.total % self.f.block == 0
        self.packed = pack_layer(self.f, w.view(-1), device)
        wf = dm.layer_f64(self.f, self.packed.cpu().numpy(), self.total, CHUNK)[: n * k].reshape(n, k)
        if self.w4a8:
            xf = dequantize(*host_quantize(self.x))
        else:
            xf = mx.bits_to_f64(mx.bf16_tensor_bits(self.x)).reshape(m, k)
        self.want, self.bound = xf @ wf.T, k * 2.0 ** -23 * (np.abs(xf) @ np.abs(wf).T)

    def run(self, device, gated=False, untiled=False, **kw):
        a = dict(src_bytes=2 * self.total, chunk_bytes=CHUNK, **self.f.kw(), **kw)
        a.update(dict(split_k=1) if untiled else dict(act="mxfp8") if self.w4a8 else dict(tiled=True))
        x, p = self.x.to(device), self.packed.to(device)
        if gated:
            return getattr(ops, self.f.name + "_swiglu")(x, p, self.n, self.k, gate_offset=0, up_offset=self.n * self.k, **a)
        return getattr(ops, self.f.name + "_linear")(x, p, self.n, self.k, elem_offset=0, **a)
