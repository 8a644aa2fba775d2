"""Case builders and checks for models/weights.py decoder_forward over PackedParams, against the
float64 reference of test_decoder_reference.py. A plain module: test_decoder_packed_reference_host.py
checks everything that rests on the reference alone and runs the ops' CPU routes through this
harness, test_gpu_decoder_packed_reference.py runs the gfx950 kernels through it.

A case is a spec (`tiny`, `uneven`), a row count (batch, seq) and a packed format with its chunk size:

  weights   random_layer(spec, 2) with every 32-element block of every 2-D parameter multiplied by
            2^j, j seeded and uniform in {-2 .. 2} (exact in bf16), so that neighbouring scale blocks
            have different scales and a kernel that read the neighbour's could not pass;
  image     the host codec's (_core.*_pack_layer_host) packed image of the flattened layer;
  W         the host codec's dequantization of that image (_core.*_unpack_layer_host, itself tested
            exhaustively against numpy), in float64. Nothing of the reference goes through the ops
            or through PackedParam.dequantize();
  x         bf16, per-position scales logspace(-2.5, 0), seeded, as in test_decoder_reference.py;
  y64       ref_decoder(x, W) in float64; e16 = rel(ref_decoder(..., rnd=bf16_round), y64) is the
            bf16 rounding floor of one layer, globally and per token row;
  d_cpu     the distance from y64 of decoder_forward on the CPU over plain bf16 tensors of W.

Check A (end to end): a route's output y lies within tol = 2 max(e16, d_cpu, d_ctl) of y64, globally,
and every token row within 2 max over rows of (row e16, row d_cpu, row d_ctl). d_ctl is the distance
of plain torch on the GPU over bf16 tensors of W; on the CPU there is no d_ctl. Nothing in the
tolerance comes from a packed route. The factor 2: a packed route rounds in other places than the
twin (the fused SwiGLU once instead of four times, the merged q/k/v in another summation order),
each an independent perturbation of the floor's own size, about sqrt(2) e16 together.
Check A sees a wrong convention, a wrong split of the merged q/k/v, a shifted parameter, a lost K
tail and a lost row tile (`mistakes`: each at least 5 tol away). It cannot see one wrong output row
(0.3 to 16 e16 away) or one wrong scale block (0.1 to 10 e16 away): no norm over the output can. With
seq = 1 it cannot see q, k or the rotary embedding at all (blind_at_one_position). Those are check B's.
Measured on an MI355X: every route, the control included, lies at most 1.03 e16 from float64.

Check B (every weight launch in situ): the ops are wrapped during the pass and every call's input,
arguments and result are recorded. The launch list is compared with one computed from
layer_params(spec) alone. Each call is made again on its recorded input with out_dtype=float32 and
must lie, per element, within K 2^-23 (|x| |W|^T) of float64 x W^T with W sliced from the host
codec's dequantization at the expected offset (the f32 accumulation bound of
test_gpu_mxfp4_swiglu.py); for the SwiGLU, with g = x Wg^T, u = x Wu^T and their bounds bg, bu,
within 4 2^-23 |silu(g) u| + 1.1 |u| bg + |silu(g)| bu + 1.1 bg bu + 2^-100 (the epilogue's bound,
then the two sums propagated through |silu'| <= 1.1). One scale block off by 2 is 64 to 560 bounds
away in its column, one code a step off 38 or more. On the GPU the recorded bf16 result must be
the f32 result rounded to nearest even, bit for bit (any NaN matching any NaN). Measured: err / bound
at most 6e-3 on an MI355X and 1e-2 on the CPU routes; one doubled scale 130 bounds or more. Check B cannot see
a mistake outside the weight launches (norms, rotary embedding, attention): that is check A's."""
import functools
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.weights import (decoder_forward, flatten, layer_nbytes, layer_params,
                                                             random_layer, unflatten_packed)

from test_decoder_reference import SPECS, bf16_round, ref_decoder, rel

KiB = 1 << 10
ROWS = [(1, 1), (3, 7), (5, 13)]  # M = 1; 21, a partial second 16-row tile; 65, a second pass of 64 rows
# (fmt, fp8 scale block, chunk bytes). 5 KiB = 2560 elements: in `uneven` chunk edges fall inside
# rows of 192 and 320 elements and q_proj starts 1.5 fp8 blocks of 128 into the image (the rows of
# `tiny` start at multiples of their own length: no chunk size cuts them)
FORMATS = {
    "mxfp4-5k": ("mxfp4", 32, 5 * KiB),
    "mxfp4-64k": ("mxfp4", 32, 64 * KiB),
    "mxfp6-5k": ("mxfp6", 32, 5 * KiB),
    "fp8b32-5k": ("fp8", 32, 5 * KiB),
    "fp8b128-5k": ("fp8", 128, 5 * KiB),
    "fp8b512-4k": ("fp8", 512, 4 * KiB),
}
CASES = [(s, r, f) for s in SPECS for r in ROWS for f in FORMATS]
PROJECTIONS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
OPS = ("mxfp4_linear", "mxfp6_linear", "fp8_linear", "mxfp4_swiglu")
CONTROL_FACTOR = 20  # what test_decoder_reference.py grants plain torch over the noise floor
# At one token row the distance of a lost row tile is a single sample and varies from 3.6 to 15
# tol with the seeds; these are chosen, on the reference alone, so that it clears 5 tol there too
WEIGHT_SEED, BLOCK_SEED, X_SEED = 2, 1, 11

try:  # these small matmuls only lose to BLAS and OpenMP threads, most of all under xdist
    from threadpoolctl import threadpool_limits as _threads
except ImportError:
    import contextlib

    def _threads(limits):
        return contextlib.nullcontext()


def one_thread(fn):
    @functools.wraps(fn)
    def wrapper(*a, **kw):
        with _threads(1):
            return fn(*a, **kw)
    return wrapper


def case_id(c):
    spec, (b, s), f = c
    return f"{spec}-{b}x{s}-{f}"


def bits_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bits_to_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def tensor_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def row_rel(a, b):
    """rel per token row: [batch, seq]."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def offsets(spec):
    """{name: (first element, shape)} from layer_params(spec) alone."""
    out, off = {}, 0
    for name, shape in layer_params(spec):
        out[name] = (off, tuple(shape))
        off += int(np.prod(shape))
    return out


def block_scaled_layer(spec):
    """random_layer with each 32-block of each 2-D parameter times 2^j, j in {-2 .. 2}."""
    wt = random_layer(spec, WEIGHT_SEED)
    g = torch.Generator().manual_seed(BLOCK_SEED)
    for name, w in wt.items():
        if w.dim() == 2:
            j = torch.randint(-2, 3, (w.numel() // 32,), generator=g)
            scaled = (w.float().view(-1, 32) * torch.exp2(j.float())[:, None]).to(torch.bfloat16)
            assert torch.equal(scaled.float(), w.float().view(-1, 32) * torch.exp2(j.float())[:, None])  # exact
            wt[name] = scaled.view(w.shape)
    return wt


def host_pack(blob, fmt, block, chunk):
    if fmt == "fp8":
        return _core.fp8_pack_layer_host(blob, chunk, block)
    return (_core.mxfp6_pack_layer_host if fmt == "mxfp6" else _core.mxfp4_pack_layer_host)(blob, chunk)


def host_unpack(img, src, fmt, block, chunk):
    if fmt == "fp8":
        return _core.fp8_unpack_layer_host(img, src, chunk, block)
    return (_core.mxfp6_unpack_layer_host if fmt == "mxfp6" else _core.mxfp4_unpack_layer_host)(img, src, chunk)


@dataclass
class Layer:
    """A spec's block-scaled layer in one packed format."""
    spec: object
    fmt: str
    block: int
    chunk: int
    src: int              # bytes of the bf16 layer
    img: np.ndarray       # the host codec's packed image (uint8)
    bits: np.ndarray      # bf16 bits of the host codec's dequantization, all src / 2 elements
    flat: np.ndarray      # the same in float64
    off: dict             # offsets(spec)
    w: dict = field(default_factory=dict)      # {name: float64 view of flat}
    dense: dict = field(default_factory=dict)  # {name: bf16 CPU tensor}

    def weight(self, first, n, k):
        return self.flat[first: first + n * k].reshape(n, k)

    def packed_params(self, device="cpu"):
        return unflatten_packed(torch.from_numpy(self.img).to(device), self.spec, self.chunk, self.fmt, self.block)


@functools.lru_cache(maxsize=None)
def layer(spec_name, fmt_name):
    spec = SPECS[spec_name]
    fmt, block, chunk = FORMATS[fmt_name]
    src = layer_nbytes(spec)
    img = host_pack(flatten(block_scaled_layer(spec), spec).numpy().tobytes(), fmt, block, chunk)
    bits = np.frombuffer(host_unpack(img, src, fmt, block, chunk), dtype=np.uint16)
    L = Layer(spec, fmt, block, chunk, src, np.frombuffer(img, dtype=np.uint8).copy(), bits, bits_to_f64(bits),
              offsets(spec))
    for name, (first, shape) in L.off.items():
        n = int(np.prod(shape))
        L.w[name] = L.flat[first: first + n].reshape(shape)
        L.dense[name] = bits_to_tensor(bits[first: first + n]).view(shape)
    return L


def packed_chunks(L):
    """[(first element, elements, offset of the scales in the image)] per source chunk: the codes
    (n / 2 bytes of e2m1, 24 n / 32 of e2m3, n of e4m3), then the scales (one E8M0 byte per 32
    elements, or one f32 per block)."""
    out, pos, ce, total = [], 0, L.chunk // 2, L.src // 2
    for e0 in range(0, total, ce):
        n = min(ce, total - e0)
        pos += {"mxfp4": n // 2, "mxfp6": n // 32 * 24, "fp8": n}[L.fmt]
        out.append((e0, n, pos))
        pos += 4 * (n // L.block) if L.fmt == "fp8" else n // 32
    assert pos == L.img.size
    return out


def scale_exponents(L):
    """log2 of every scale of the packed image, in layer order, read from the image itself."""
    if L.fmt == "fp8":
        return np.concatenate([np.log2(L.img[so: so + 4 * (n // L.block)].view(np.float32).astype(np.float64))
                               for _, n, so in packed_chunks(L)])
    return np.concatenate([L.img[so: so + n // 32].astype(np.float64) - 127 for _, n, so in packed_chunks(L)])


def image_with_a_doubled_scale(L, elem):
    """A copy of the image in which the scale of element `elem`'s block is twice what it was."""
    img = L.img.copy()
    for e0, n, so in packed_chunks(L):
        if e0 <= elem < e0 + n:
            i = (elem - e0) // L.block
            if L.fmt == "fp8":
                img[so + 4 * i: so + 4 * i + 4].view(np.float32)[0] *= 2
            else:
                assert img[so + i] < 0xFE
                img[so + i] += 1
            return img
    raise IndexError(elem)


def amax_binades(L, name):
    """floor(log2(amax)) of every 32-block of a parameter as the kernels see it (dequantized)."""
    a = np.abs(L.w[name]).reshape(-1, 32).max(axis=1)
    return np.floor(np.log2(a))


@dataclass
class Case:
    id: str
    layer: Layer
    batch: int
    seq: int
    xt: torch.Tensor      # bf16 [batch, seq, hidden]
    x: np.ndarray         # float64
    y64: np.ndarray
    e16: float
    row_e16: np.ndarray   # [batch, seq]
    d_cpu: float
    row_d_cpu: np.ndarray

    @property
    def spec(self):
        return self.layer.spec

    def tol(self, d_ctl=0.0):
        return 2 * max(self.e16, self.d_cpu, d_ctl)

    def row_tol(self, row_d_ctl=0.0):
        return 2 * max(self.row_e16.max(), self.row_d_cpu.max(), np.max(row_d_ctl))


@functools.lru_cache(maxsize=None)
@one_thread
def case(spec_name, rows, fmt_name):
    L = layer(spec_name, fmt_name)
    b, s = rows
    g = torch.Generator().manual_seed(X_SEED)
    scale = torch.logspace(-2.5, 0, s)[torch.randperm(s, generator=g)]
    xt = (torch.randn(b, s, L.spec.hidden, generator=g) * scale[None, :, None]).to(torch.bfloat16)
    x = xt.float().numpy().astype(np.float64)
    y64 = ref_decoder(x, L.w, L.spec)
    y16 = ref_decoder(x, L.w, L.spec, rnd=bf16_round)
    ycpu = decoder_forward(xt, L.dense, L.spec).float().numpy()
    return Case(case_id((spec_name, rows, fmt_name)), L, b, s, xt, x, y64, rel(y16, y64), row_rel(y16, y64),
                rel(ycpu, y64), row_rel(ycpu, y64))


# ---------------------------------------------------------------- check A

def check_a(c, y, what, d_ctl=0.0, row_d_ctl=0.0):
    """Asserts check A for the output tensor y of one route; returns (dist / e16, worst row dist /
    row tolerance's floor)."""
    yf = y.float().cpu().numpy()
    assert y.dtype == torch.bfloat16 and yf.shape == c.y64.shape
    dist, rows = rel(yf, c.y64), row_rel(yf, c.y64)
    tol, row_tol = c.tol(d_ctl), c.row_tol(row_d_ctl)
    print(f"{c.id} {what}: dist / e16 {dist / c.e16:.3f} (tol {tol / c.e16:.3f}), worst row dist / worst row floor "
          f"{rows.max() / (row_tol / 2):.3f}, worst row dist / its own e16 {(rows / c.row_e16).max():.3f}")
    assert dist <= tol
    assert (rows <= row_tol).all()
    return dist / c.e16, float(rows.max() / (row_tol / 2))


def mistakes(spec_name):
    """Names of the mistakes check A must see: the conventions of test_decoder_reference.py that
    the packed routes could get wrong, k and v exchanged (a wrong split of the merged result), and
    per projection: read 32 elements late, its K tail (K mod 128 columns) lost, its last 16 output
    rows zero."""
    L = layer(spec_name, "mxfp4-5k")
    out = ["kv_modulo", "silu_on_up", "interleaved_rope", "kv_exchanged"]
    out += [f"late32:{p}" for p in PROJECTIONS]
    out += [f"k_tail_lost:{p}" for p in PROJECTIONS if L.off[p][1][1] % 128]
    out += [f"last_tile_zero:{p}" for p in PROJECTIONS]
    return out


def blind_at_one_position(name):
    """With seq = 1 the softmax runs over one key: the attention output is v whatever q and k hold,
    and position 0 is not rotated. A mistake confined to q, k or the rotary embedding then changes
    nothing, by the definition of the layer; only check B sees q and k at M = 1."""
    return name == "interleaved_rope" or name.split(":")[-1] in ("q_proj", "k_proj")


@one_thread
def mistaken(c, name):
    """The float64 reference with one mistake."""
    L = c.layer
    if ":" not in name and name != "kv_exchanged":
        return ref_decoder(c.x, L.w, c.spec, mistake=name)
    w = dict(L.w)
    if name == "kv_exchanged":
        w["k_proj"], w["v_proj"] = w["v_proj"], w["k_proj"]
        return ref_decoder(c.x, w, c.spec)
    kind, p = name.split(":")
    first, (n, k) = L.off[p]
    if kind == "late32":
        assert first + 32 + n * k <= L.flat.size
        w[p] = L.weight(first + 32, n, k)
    elif kind == "k_tail_lost":
        assert k % 128
        w[p] = w[p].copy()
        w[p][:, k - k % 128:] = 0
    else:
        assert kind == "last_tile_zero"
        w[p] = w[p].copy()
        w[p][-16:] = 0
    return ref_decoder(c.x, w, c.spec)


# ---------------------------------------------------------------- check B

@dataclass
class Launch:
    op: str
    x: torch.Tensor       # the input, cloned at the call
    packed: torch.Tensor
    n: int
    k: int
    kw: dict
    y: torch.Tensor       # the very tensor decoder_forward went on with


@one_thread
def run_captured(x, params, spec, fuse):
    """decoder_forward with the four packed ops wrapped: (y, [Launch])."""
    rec = []
    with pytest.MonkeyPatch.context() as mp:
        for name in OPS:
            def wrapped(xx, packed, n, k, _fn=getattr(ops, name), _name=name, **kw):
                y = _fn(xx, packed, n, k, **kw)
                rec.append(Launch(_name, xx.detach().clone(), packed, n, k, dict(kw), y))
                return y
            mp.setattr(ops, name, wrapped)
        y = decoder_forward(x, params, spec, fuse=fuse)
    return y, rec


def expected_launches(c, fuse, merged_qkv):
    """[(op, offsets, N, K)] from layer_params(spec) and the format alone. `merged_qkv`: the
    device merges q, k and v (the GPU does, the CPU does not)."""
    L, spec = c.layer, c.spec
    o = {name: first for name, (first, _) in L.off.items()}
    h, i, kv = spec.hidden, spec.intermediate, spec.kv_heads * spec.head_dim
    lin = L.fmt + "_linear"
    assert o["q_proj"] == h and o["k_proj"] == h + h * h and o["v_proj"] == o["k_proj"] + kv * h
    if fuse and merged_qkv:
        out = [(lin, (o["q_proj"],), h + 2 * kv, h)]
    else:
        out = [(lin, (o["q_proj"],), h, h), (lin, (o["k_proj"],), kv, h), (lin, (o["v_proj"],), kv, h)]
    out.append((lin, (o["o_proj"],), h, h))
    if fuse and L.fmt == "mxfp4":
        out.append(("mxfp4_swiglu", (o["gate_proj"], o["up_proj"]), i, h))
    else:
        out += [(lin, (o["gate_proj"],), i, h), (lin, (o["up_proj"],), i, h)]
    out.append((lin, (o["down_proj"],), h, i))
    return out


def check_launch_list(c, rec, expected, packed):
    assert [r.op for r in rec] == [e[0] for e in expected]
    L = c.layer
    for r, (op, offs, n, k) in zip(rec, expected):
        assert (r.n, r.k) == (n, k), (op, r.n, r.k)
        want = dict(src_bytes=layer_nbytes(c.spec), chunk_bytes=L.chunk, out_dtype=torch.bfloat16)
        if op == "mxfp4_swiglu":
            want.update(gate_offset=offs[0], up_offset=offs[1])
        else:
            want.update(elem_offset=offs[0])
        if L.fmt == "fp8":
            want.update(block=L.block)
        assert r.kw == want, (op, r.kw, want)
        assert r.packed.data_ptr() == packed.data_ptr() and r.packed.numel() == packed.numel() == L.img.size
        assert r.x.dtype == torch.bfloat16 and tuple(r.x.shape) == (c.batch, c.seq, k)
        assert r.y.dtype == torch.bfloat16 and tuple(r.y.shape) == (c.batch, c.seq, n)


def silu(g):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


def linear_bound(xf, w):
    return xf @ w.T, xf.shape[1] * 2.0 ** -23 * (np.abs(xf) @ np.abs(w).T)


def worst_ratio(err, bound):
    assert (err <= bound).all(), float((err[bound > 0] / bound[bound > 0]).max())
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@one_thread
def check_launch(c, r, expected, rounded_f32):
    """Steps 2 to 4 for one recorded launch: the call again with out_dtype=float32 against float64
    on the expected slice of the host codec's dequantization; with `rounded_f32` (the GPU) the
    recorded bf16 result is that f32 result rounded. Returns the worst err / bound."""
    L = c.layer
    op, offs, n, k = expected
    xf = bits_to_f64(tensor_bits(r.x)).reshape(-1, k)
    y32 = getattr(ops, op)(r.x, r.packed, r.n, r.k, **{**r.kw, "out_dtype": torch.float32})
    assert y32.dtype == torch.float32 and y32.shape == r.y.shape
    got = y32.cpu().numpy().astype(np.float64).reshape(-1, n)
    if op == "mxfp4_swiglu":
        (g, bg), (u, bu) = linear_bound(xf, L.weight(offs[0], n, k)), linear_bound(xf, L.weight(offs[1], n, k))
        want = silu(g) * u
        bound = (4 * 2.0 ** -23 * np.abs(want) + 1.1 * np.abs(u) * bg + np.abs(silu(g)) * bu + 1.1 * bg * bu
                 + 2.0 ** -100)
    else:
        want, bound = linear_bound(xf, L.weight(offs[0], n, k))
    worst = worst_ratio(np.abs(got - want), bound)
    if rounded_f32:
        assert_same_bf16(r.y, y32.to(torch.bfloat16))
    return worst


def assert_same_bf16(a, b):
    """Equal bf16 bits; any NaN matches any NaN."""
    assert a.dtype == b.dtype == torch.bfloat16 and a.shape == b.shape
    na, nb = torch.isnan(a).cpu().numpy().reshape(-1), torch.isnan(b).cpu().numpy().reshape(-1)
    assert np.array_equal(na, nb)
    assert np.array_equal(tensor_bits(a)[~na], tensor_bits(b)[~nb])
