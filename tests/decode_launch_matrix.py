"""Every launch shape the six decode launchers can choose: mxfp4_linear, fp8_linear, mxfp6_linear
and the three *_swiglu kernels are families of template instantiations (MT = 1..4 tiles of x; NT =
1, 2, 4 row tiles or P = 1, 2 pairs per wave; 1..16 K slices reduced through LDS), and the launcher
picks one member per pass of up to 64 rows. `_core.<kernel>_plan(m, n, k, split_k, row_tiles)` is
the launcher's own choice, bound to Python (host code; it needs no GPU). A plain module:
test_decode_launch_matrix_host.py holds the matrix to the plans the served models reach and runs
every case through the ops' CPU route, test_gpu_decode_launch_matrix.py runs it on gfx950.

served_plans(kernel): the (mt, nt, slices) the launcher picks, nothing forced, for every projection
of every served preset at every m in 1..64 (a launcher works in passes of 64 rows).

MATRIX[kernel]: cases (mt, nt, slices, m, n, k, split_k, row_tiles) with split_k and row_tiles such
that the plan function returns exactly (mt, nt, slices):

  every instantiation of the launcher's switch, at 1, 2, 3 slices, at its most, and at every other
  count served_plans holds for it; m = 16 mt - 3 (a partial last tile) and 16 mt; N = 16 nt 3
  (three workgroups); per slice count S three K:
    128 S + 32          one step for every wave, the tail (1 block) on the last working wave;
    128 (2 S + 1) + 96  3 steps per wave, an uneven last working wave, idle waves behind it, the
                        tail (3 blocks) on an idle wave;
    512 S               4 steps on every wave (the prefetch loop at length 4), no tail;
  and at 16 slices also K = 128 * 64 + 96 = 8288: 4 steps on all 16 waves and a tail behind them;
  two unforced cases (split_k = row_tiles = 0) at N = 4096 and 16384, K = 288, m = 13, where N alone
  moves the launcher's rule: the linears take 2 and 4 row tiles, the gated kernels 1 and 2 pairs
  (their rule counts 2 N / 16 tiles against 1024, which N = 4096 does not reach).

Inputs are the existing ones: PF.image of packed_extremes.py (handmade images), each format's
ref_layer_bits (numpy ref_unpack per chunk) and linear_extremes.scaled_ints; the expectation is a float64 matmul. The
parameters sit at element 224 of a layer in 1 KiB chunks (fp8: 8 * block bytes, the smallest the
format allows), so chunk edges fall inside rows and inside steps of 128; the two N-alone cases use
64 KiB chunks. x holds integers in [-8, 8], or in [-2, 2] where the closed-form bound 8 wmax K <
2^24 uw would not hold (fp8 from K = 4370 on); prove() asserts the conditions of
linear_extremes.prove_exact on the inputs themselves, so the f32 result equals the float64 one in
any summation order and any K slicing."""
from functools import lru_cache

import numpy as np
import torch

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.weights import PRESETS

import linear_extremes as le
import test_fp8_linear_host as f8
import test_mxfp4_linear_host as mx
import test_mxfp6_linear_host as m6
from packed_extremes import PF

KiB = 1 << 10
KERNELS = ["mxfp4_linear", "fp8_linear", "mxfp6_linear", "mxfp4_swiglu", "fp8_swiglu", "mxfp6_swiglu"]
# the cases of each launcher's switch: (MT, NT) of a linear, (MT, P) of a gated kernel
INSTANTIATIONS = {
    "linear": [(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4), (3, 1), (3, 2), (4, 1), (4, 2)],
    "swiglu": [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (4, 1)],
}
SERVED_MODELS = [name for name in PRESETS if name != "tiny"]
UNFORCED = [(13, 4096, 288), (13, 16384, 288)]  # (m, n, k) of the two cases where N alone decides
K_LONGEST = 128 * 64 + 96
WMAX = {"mxfp4": 12.0, "mxfp6": 15.0, "fp8": 30.0}  # largest magnitude of a handmade image's weights


def kind(kernel):
    return kernel.split("_")[1]


def fmt_name(kernel):
    return kernel.split("_")[0]


def formats(kernel):
    """The PFs a kernel's cases run with; fp8 block 512 takes the most-slices cases only."""
    name = fmt_name(kernel)
    return [PF("fp8", 32), PF("fp8", 128), PF("fp8", 512)] if name == "fp8" else [PF(name)]


def plan(kernel, m, n, k, split_k=0, row_tiles=0):
    return tuple(getattr(_core, kernel + "_plan")(m, n, k, split_k, row_tiles))


def served_shapes(kernel):
    """(model, projection, N, K) of every launch decoder_forward / decoder_step can make of `kernel`."""
    out = []
    for name in SERVED_MODELS:
        s = PRESETS[name]
        h, i, kv = s.hidden, s.intermediate, s.kv_heads * s.head_dim
        if kind(kernel) == "swiglu":
            out.append((name, "gate/up fused", i, h))
        else:
            out += [(name, "q_proj", h, h), (name, "k/v_proj", kv, h), (name, "q/k/v merged", h + 2 * kv, h),
                    (name, "o_proj", h, h), (name, "gate/up alone", i, h), (name, "down_proj", h, i)]
    return out


@lru_cache(maxsize=None)
def served_plans(kernel):
    return frozenset(plan(kernel, m, n, k) for _, _, n, k in served_shapes(kernel) for m in range(1, 65))


# The most slices of an instantiation (512 threads and 64 KiB of LDS; 1024 threads for the thinnest
# waves), and the slice counts beyond 1, 2, 3 and the most that the served models reach. Written out, not
# computed: a retune of a launcher's rules that moves a served plan out of the matrix, or changes what an
# instantiation is clipped to, fails test_decode_launch_matrix_host.py until this table - and with it the
# GPU file's cases - follows.
MOST = {"linear": {(1, 1): 16, (1, 2): 16, (2, 1): 16}, "swiglu": {(1, 1): 16}}  # every other instantiation: 8
SERVED_SLICES = {
    "mxfp4_linear": {(1, 2): [8], (1, 4): [4], (2, 4): [4], (3, 2): [4], (4, 2): [4]},
    "fp8_linear": {(1, 2): [4, 8], (1, 4): [4], (2, 2): [4], (2, 4): [4], (3, 2): [4], (4, 2): [4]},
    "mxfp6_linear": {(1, 2): [4, 8], (1, 4): [4], (2, 2): [4], (2, 4): [4], (3, 2): [4], (4, 2): [4]},
    "mxfp4_swiglu": {(1, 1): [4, 8], (1, 2): [4], (2, 2): [4]},
    "fp8_swiglu": {(1, 1): [4, 8], (1, 2): [4]},
    "mxfp6_swiglu": {(1, 1): [4, 8], (1, 2): [4], (2, 2): [4]},
}


def max_slices(kernel, mt, nt):
    return MOST[kind(kernel)].get((mt, nt), 8)


def slice_counts(kernel, mt, nt):
    return sorted({1, 2, 3, max_slices(kernel, mt, nt)} | set(SERVED_SLICES[kernel].get((mt, nt), [])))


def k_cases(s):
    return [128 * s + 32, 128 * (2 * s + 1) + 96, 512 * s] + ([K_LONGEST] if s == 16 else [])


def _matrix(kernel):
    cases = []
    for mt, nt in INSTANTIATIONS[kind(kernel)]:
        for s in slice_counts(kernel, mt, nt):
            for k in k_cases(s):
                for m in (16 * mt - 3, 16 * mt):
                    cases.append((mt, nt, s, m, 16 * nt * 3, k, s, nt))
    for m, n, k in UNFORCED:
        cases.append(plan(kernel, m, n, k) + (m, n, k, 0, 0))
    return cases


MATRIX = {kernel: _matrix(kernel) for kernel in KERNELS}


def is_unforced(case):
    return case[6] == 0 and case[7] == 0


def at_most_slices(kernel, case):
    mt, nt, s = case[:3]
    return not is_unforced(case) and s == max_slices(kernel, mt, nt)


def cases_of(kernel, f, mt, nt):
    """The forced cases of one instantiation that format `f` runs."""
    out = [c for c in MATRIX[kernel] if c[:2] == (mt, nt) and not is_unforced(c)]
    return [c for c in out if at_most_slices(kernel, c)] if f.block == 512 else out


# ---------------------------------------------------------------- inputs and expectations

def x_bound(f, k):
    """8, or 2 where integers up to 8 would leave the closed-form condition 8 wmax K < 2^24 uw."""
    return 8 if 8 * WMAX[f.name] * k < 2.0 ** 24 * f.uw else 2


def layout(f, n, k, gated, unforced=False):
    """(chunk, [offsets], total): the parameter at element 224; a gated pair's up behind the gate
    after a gap of 96 elements and one scale block; the layer goes on behind them."""
    chunk = 64 * KiB if unforced else 8 * f.block if f.name == "fp8" else 1024
    pad = f.block if f.name == "fp8" else 0
    offs = [32 * 7]
    if gated:
        offs.append(offs[0] + n * k + 32 * 3 + pad)
    return chunk, offs, f.padded(offs[-1] + n * k + 32 * 5 + pad)


def layer_f64(f, img, total, chunk):
    """All `total` elements of the image in float64: each format's ref_layer_bits (ref_unpack per chunk)."""
    if f.name == "fp8":
        return f8.bits_to_f64(f8.ref_layer_bits(img, total, chunk, f.block))
    mod = mx if f.name == "mxfp4" else m6
    return mod.bits_to_f64(mod.ref_layer_bits(img, total, chunk))


@lru_cache(maxsize=32)
def inputs(f_id, gated, n, k, unforced=False):
    """(f, image, total, chunk, offsets, [float64 [n, k] per offset], x, xf, [float64 x W^T per offset]) with 64 rows
    of x; built once per shape and left unchanged. A case of m rows takes the first m: row r of x W^T depends on
    row r of x alone."""
    f = PF(*(("fp8", int(f_id[4:])) if f_id.startswith("fp8") else (f_id,)))
    chunk, offs, total = layout(f, n, k, gated, unforced)
    img = f.image(total, chunk, 7 + n + k)
    flat = layer_f64(f, img, total, chunk)  # what PF.weight slices, decoded once for both parameters
    ws = [flat[o: o + n * k].reshape(n, k) for o in offs]
    hi = x_bound(f, k)
    x, xf = le.scaled_ints(64, k, 11 + k, 0, -hi, hi)
    return f, img, total, chunk, offs, ws, x, xf, [xf @ w.T for w in ws]


class Built:
    """One matrix case with its inputs: img, total, chunk, offs, ws (float64 weights), x, xf and
    wants (float64 x W^T per parameter)."""

    def __init__(self, kernel, f, case):
        self.kernel, self.case = kernel, case
        self.m, self.n, self.k, self.split_k, self.row_tiles = case[3:]
        self.gated = kind(kernel) == "swiglu"
        self.f, self.img, self.total, self.chunk, self.offs, self.ws, x, xf, wants = inputs(
            f.id, self.gated, self.n, self.k, is_unforced(case))
        self.hi = x_bound(f, self.k)
        self.x, self.xf, self.wants = x[: self.m], xf[: self.m], [w[: self.m] for w in wants]

    def prove(self):
        """The closed form and linear_extremes.prove_exact on the inputs themselves."""
        f = self.f
        assert np.abs(self.xf).max() <= self.hi and self.hi * WMAX[f.name] * self.k < 2.0 ** 24 * f.uw
        for w, want in zip(self.ws, self.wants):
            assert np.abs(w).max() <= WMAX[f.name]
            le.prove_exact(self.xf, w, 1.0, f.uw, want)

    def run(self, device, img=None, linear_of=None, **kw):
        """The case's op with its forced split_k and row_tiles. `linear_of` = 0 or 1: the format's
        linear op on the gate or the up parameter instead, with the same split_k."""
        p = torch.from_numpy(self.img).to(device) if img is None else img
        a = dict(src_bytes=2 * self.total, chunk_bytes=self.chunk, split_k=self.split_k, **self.f.kw(), **kw)
        x = self.x.to(device)
        if linear_of is not None:
            return getattr(ops, self.f.name + "_linear")(x, p, self.n, self.k, elem_offset=self.offs[linear_of], **a)
        if self.gated:
            return getattr(ops, self.kernel)(x, p, self.n, self.k, gate_offset=self.offs[0], up_offset=self.offs[1],
                                             row_tiles=self.row_tiles, **a)
        return getattr(ops, self.kernel)(x, p, self.n, self.k, elem_offset=self.offs[0], row_tiles=self.row_tiles, **a)
