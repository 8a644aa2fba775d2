"""The gfx950 many-row kernels (mxfp4_tiled.hip, fp8_tiled.hip, mxfp6_tiled.hip, tiled_x.h;
tiled=True of ops.mxfp4_linear, mxfp4_swiglu, fp8_linear, fp8_swiglu, mxfp6_linear, mxfp6_swiglu; fp8
with blocks 32 and 128, and 512 on one far case) at their numeric and addressing extremes: the
cases of linear_extremes.py, mxfp6_linear_extremes.py and packed_extremes.py, which the host twins
run through the CPU route. The expectation is the numpy ref_unpack per chunk and a float64 matmul;
every case carries the proof, asserted here on the reference alone, that an f32 accumulation in
any order is exact: linear f32 outputs are compared for equality, bf16 outputs with the rounding of
the expectation, gated f32 outputs through check_exact_regimes of test_gpu_mxfp4_swiglu.py.

Row counts follow the tile (BM, BN from the bindings): 5 rows (a partial tile, K tail alone), BM + 1
(a second tile of one row) and 2 BM + 5 rows by BN + 16 weight rows (a second workgroup along M
and along N, eight K steps and a tail).

1. bf16-subnormal weights (B operand), bf16-subnormal activations (A operand, through the staging
   registers and the swizzled LDS image of tiled_x.h) and f32-subnormal products and sums; the
   subnormal gate against an ordinary up and the reverse. A flush anywhere on the way shows as a
   wrong value (the host twin asserts that the flushed expectation differs).
2. weights that convert to +-inf (scale bytes 253 / 254), f32 sums that overflow (fp8, E = 120), NaN
   and +-inf in one row of x - row BM, the only row of the second tile, in two of three variants.
   The non-finite row again as a one-row call gives the same bits: batch invariance there. Cannot
   tell NaN payloads apart.
3. parameters behind and across 2^31 / 2^32 elements and packed bytes of a layer that is never
   read, with BM + 1 rows: the FAR tables of the two decode suites, the gated pairs of
   packed_extremes.FAR_GLU, and per format a parameter of BN + 16 rows whose second workgroup
   starts behind the boundary. Peak 4.73 GB. A truncated index shows as a wrong value only: the
   wrapped address lies in the allocated low part of the buffer (asserted before the launch).
4. x and y themselves beyond 2^31 elements and 2^32 bytes in one launch: M K just beyond 2^32
   elements of x (8.6 GB, written only where checked; peak 8.9 GB), and 2^22 + 5 rows of y with a
   row stride of 528 f32 in a 0xA5-filled buffer (8.9 GB; peak 9.2 GB). Checked are the first
   tile, the tiles around each crossing and the last, partial tile: bit for bit against a small call
   on those rows alone, which is itself held to the float64 expectation. Rows that read
   uninitialised x are not looked at; a store that lands outside the checked windows and the guard
   rows of y is not seen.
5. views of x."""
import numpy as np
import pytest
import torch

import packed_extremes as pe
import test_gpu_linear_extremes as gl4
import test_gpu_mxfp6_linear_extremes as gl6
from packed_extremes import FAR_K, FORMATS, GB, P2_31, P2_32, PF, le
from test_gpu_mxfp4_swiglu import check_exact_regimes

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = [f.id for f in FORMATS]
SHAPE_NAMES = ["K tail alone", "second tile", "two workgroups each way"]


def _shape(f, name):
    bm, bn = f.tile()
    return {"K tail alone": (5, 48, 96), "second tile": (bm + 1, 48, 160),
            "two workgroups each way": (2 * bm + 5, bn + 16, 1056)}[name]


def _bits16(y32):
    return le.f32_to_bf16_bits(y32.cpu().numpy()).reshape(-1)


def _check_linear(c, want=None, **kw):
    """f32 output == expectation, bf16 output == its rounding; returns both."""
    want = c.want if want is None else want
    y32 = pe.run_linear(c, DEV, tiled=True, out_dtype=torch.float32, **kw)
    y16 = pe.run_linear(c, DEV, tiled=True, **kw)
    le.assert_f32_equal(y32, want)
    le.assert_bf16_is_rounded(y16, want)
    return y32, y16


def _run_glu(c, **kw):
    y32 = pe.run_swiglu(c, DEV, tiled=True, out_dtype=torch.float32, **kw)
    y16 = pe.run_swiglu(c, DEV, tiled=True, **kw)
    assert np.array_equal(le.mx.bf16_tensor_bits(y16), _bits16(y32))
    return y32, y16


def _check_glu(c, cols=None, check=check_exact_regimes, **kw):
    y32, y16 = _run_glu(c, **kw)
    cols = slice(None) if cols is None else cols
    print(c.f.id, "worst err / bound", check(y32[:, cols], c.g[:, cols], c.u[:, cols]))
    return y32, y16


# ---------------------------------------------------------------- 1. the bottom of the range

LOW = [(f, s) for f in FORMATS for s in (100, 0)] + [(FORMATS[0], -8)]


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("f,s", LOW, ids=[f"{f.id} s={s}" for f, s in LOW])
def test_subnormal_weights(gpu, f, s, shape):
    c = pe.subnormal_weights(f, *_shape(f, shape), s)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    _check_linear(c)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_subnormal_activations(gpu, f, shape):
    """bf16 subnormals through XStage's registers and the LDS image."""
    c = pe.subnormal_activations(f, *_shape(f, shape))
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    _check_linear(c)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("which", ["gate", "up"])
@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_swiglu_subnormal_weights(gpu, f, which, shape):
    c = pe.swiglu_subnormal(f, which, *_shape(f, shape))
    pe.prove_swiglu(c)
    _check_glu(c)


# ---------------------------------------------------------------- 2. the top of the range

OVERFLOW = [(FORMATS[0], False), (FORMATS[0], True), (FORMATS[1], False), (FORMATS[1], True), (FORMATS[2], False),
            (FORMATS[3], False)]


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("f,zeros", OVERFLOW, ids=[f.id + (" zeros in x" if z else "") for f, z in OVERFLOW])
def test_overflow_to_inf(gpu, f, zeros, shape):
    """MXFP4 / MXFP6 scale bytes 253 and 254 (kept columns carry the bits of the run on the clean
    image); fp8 at E = 120, where one-signed sums pass 2^129 and warm rows stay finite."""
    c = pe.overflow(f, *_shape(f, shape), zeros)
    keep = c.extra["keep"]
    if f.name == "fp8":
        le.prove_exact(c.xf, c.wf[keep], c.ux, c.uw, c.want[:, keep])
        le.prove_exact(c.xf, c.wf[c.extra["warm"]], 1.0, 2.0 ** 117, c.want[:, c.extra["warm"]])
        _check_linear(c)
        return
    cl = c.extra["clean"]
    le.prove_exact(cl.xf, cl.wf, cl.ux, cl.uw, cl.want)
    (y32, y16), (c32, c16) = _check_linear(c), _check_linear(cl)
    le.assert_rows_bit_equal(y32.t(), c32.t(), keep)
    le.assert_rows_bit_equal(y16.t(), c16.t(), keep)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("which", ["gate", "up"])
@pytest.mark.parametrize("f,zeros", pe.GLU_OVERFLOW, ids=pe.GLU_OVERFLOW_IDS)
def test_swiglu_overflow_to_inf(gpu, f, zeros, which, shape):
    """The gated pair of the fp8 and MXFP6 kernels with the top of the range in the gate, then in
    the up (MXFP4's gated kernel meets the top in test_swiglu_nonfinite_activations)."""
    c = pe.swiglu_overflow(f, which, *_shape(f, shape), zeros=zeros)
    rows, keep = c.extra["rows"], c.extra["keep"]
    pe.prove_swiglu(c, keep)
    pe.prove_warm(c)
    c32, c16 = _run_glu(c, img=c.extra["clean_img"])
    y32, y16 = _check_glu(c, np.setdiff1d(np.arange(c.n), rows), check=pe.check_regimes_to_inf)
    le.assert_f32_equal(y32[:, rows], le.expected_f32(c.extra["want"]).astype(np.float64))
    le.assert_rows_bit_equal(y32.t(), c32.t(), keep)
    le.assert_rows_bit_equal(y16.t(), c16.t(), keep)


def _bad_shape(f, name):
    """(m, n, k, bad row): row 3 of 5, and row BM - the second tile's only row, and a row of the
    second of three tiles."""
    m, n, k = _shape(f, name)
    return m, n, k, 3 if m == 5 else f.tile()[0]


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_nonfinite_activations(gpu, f, shape):
    m, n, k, r = _bad_shape(f, shape)
    c = pe.nonfinite_activations(f, n, k, m, row=r)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    c32, c16 = _check_linear(c)
    for xb, _, want in c.extra["bad"].values():
        y32, y16 = _check_linear(c, want=want, x=xb)
        le.assert_rows_bit_equal(y32, c32, c.extra["keep"])
        le.assert_rows_bit_equal(y16, c16, c.extra["keep"])
        a32, a16 = _check_linear(c, want=want[r: r + 1], x=xb[r: r + 1])  # the bad row alone
        assert torch.equal(a32.view(torch.int32), y32[r: r + 1].view(torch.int32))
        assert torch.equal(a16.view(torch.int16), y16[r: r + 1].view(torch.int16))


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_swiglu_nonfinite_activations(gpu, f, shape):
    m, n, k, r = _bad_shape(f, shape)
    c = pe.swiglu_nonfinite(f, n, k, m, row=r)
    pe.prove_swiglu(c)
    c32, c16 = _check_glu(c)
    for xb, g, u in c.extra["bad"].values():
        want = le.expected_f32(le.silu_mul64(g[r], u[r])).astype(np.float64)
        assert not np.isfinite(want).any()
        y32, y16 = _run_glu(c, x=xb)
        le.assert_f32_equal(y32[r], want)
        le.assert_rows_bit_equal(y32, c32, c.extra["keep"])
        le.assert_rows_bit_equal(y16, c16, c.extra["keep"])
        a32, a16 = _run_glu(c, x=xb[r: r + 1])  # the bad row alone
        assert torch.equal(a32.view(torch.int32), y32[r: r + 1].view(torch.int32))
        assert torch.equal(a16.view(torch.int16), y16[r: r + 1].view(torch.int16))


# ---------------------------------------------------------------- 3. far into a large layer

def _far_run(c, uw, gated):
    """The tiled linear on the case's (gate) parameter and, for a pair, the tiled gated kernel,
    behind one allocation."""
    le.prove_exact(c.xf, c.wf, 1.0, uw, c.want)
    assert c.need < 5 * GB and pe.wrapped_inside(c)
    torch.cuda.empty_cache()
    buf = c.place(DEV)
    try:
        le.assert_f32_equal(pe.far_linear(c, buf, tiled=True, out_dtype=torch.float32), c.want)
        le.assert_bf16_is_rounded(pe.far_linear(c, buf, tiled=True), c.want)
        assert np.array_equal(le.mx.bf16_tensor_bits(pe.far_unpack(c, buf)), c.bits)
        if gated:
            u = c.xf @ c.wu.T
            le.prove_exact(c.xf, c.wu, 1.0, uw, u)
            y32 = pe.far_swiglu(c, buf, tiled=True, out_dtype=torch.float32)
            check_exact_regimes(y32, c.want, u)
            assert np.array_equal(le.mx.bf16_tensor_bits(pe.far_swiglu(c, buf, tiled=True)), _bits16(y32))
            assert np.array_equal(le.mx.bf16_tensor_bits(pe.far_unpack(c, buf, c.up_s)), c.up_bits)
    finally:
        del buf
        torch.cuda.empty_cache()


FAR_LINEAR = [("mxfp4/fp8: " + k, v) for k, v in gl4.FAR.items()] + \
             [("mxfp6: " + k, ("mxfp6",) + v[:3]) for k, v in gl6.FAR.items()]


@pytest.mark.parametrize("name,spec", FAR_LINEAR, ids=[n for n, _ in FAR_LINEAR])
def test_far_linear_tables_of_the_decode_suites(gpu, name, spec):
    fmt, c0, boundary, packed = spec
    f = PF(fmt, 128 if fmt == "fp8" else 32)
    off_s = 32 * 700
    if c0 is None:
        c0, off_s = pe.crossing_c0(f, boundary, packed)
    c = pe.far_case(f, c0, off_s, m=f.tile()[0] + 1, n=64 if "64 rows" in name else pe.FAR_N)
    pe.assert_far_position(c, boundary, packed)
    _far_run(c, f.uw, False)


FAR_PAIRS = {**pe.FAR_GLU_MXFP4, **pe.FAR_GLU}


@pytest.mark.parametrize("name", list(FAR_PAIRS))
def test_far_gate_up_pairs(gpu, name):
    f = FAR_PAIRS[name][0]
    _far_run(pe.far_glu_case(name, m=f.tile()[0] + 1), f.uw, True)


FAR_WIDE = {
    "mxfp4 element 2^32 inside": (FORMATS[0], None, P2_32),
    "mxfp6 element 2^31 inside": (FORMATS[1], None, P2_31),
    "fp8 element 2^31 inside": (FORMATS[3], None, P2_31),
    "fp8 block 512 behind 2^32 elements and bytes": (PF("fp8", 512), 131_100, None),
}


@pytest.mark.parametrize("name", list(FAR_WIDE))
def test_far_parameter_of_two_workgroups(gpu, name):
    """A gate / up pair of BN + 16 rows each: the second and third workgroup along N (gated: 64
    columns each) start from row_elem values behind the boundary that the first one crosses."""
    f, c0, boundary = FAR_WIDE[name]
    bm, bn = f.tile()
    n, gate = bn + 16, 32 * 3
    if c0 is None:
        c0, gate = pe.crossing_c0(f, boundary, False)
    up = gate + n * FAR_K + 64
    c = pe.far_case(f, c0, gate, m=bm + 1, n=n, up_s=up, chunks=-(-(up + n * FAR_K) // (pe.FAR_CHUNK // 2)))
    pe.assert_far_position(c, boundary, False)
    if boundary is not None:
        assert c.elem_offset + (bn // 2) * FAR_K > boundary  # the second workgroup's first row, linear and gated
    _far_run(c, f.uw, True)


# ---------------------------------------------------------------- 4. rows of x and of y beyond 32 bits

BIG = [(FORMATS[0], False), (FORMATS[1], False), (FORMATS[3], False), (FORMATS[3], True)]
BIG_IDS = [f.id + (" swiglu" if g else " linear") for f, g in BIG]


def _big_case(f, gated, rows, k):
    """A clean exact case of `rows` rows (the checked windows, one behind the other) and its runner."""
    if gated:
        c = pe.swiglu_clean(f, rows, pe.BIG_N, k)
        pe.prove_swiglu(c)
        return c, lambda x, img, **kw: pe.run_swiglu(c, DEV, x=x, img=img, tiled=True, **kw)
    c = pe.clean_case(f, rows, pe.BIG_N, k)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    return c, lambda x, img, **kw: pe.run_linear(c, DEV, x=x, img=img, tiled=True, **kw)


def _check_small(c, gated, y, a, b):
    """Rows [a, b) of the case, as computed by a small call, against the float64 expectation."""
    if gated:
        check_exact_regimes(y, c.g[a:b], c.u[a:b])
    else:
        le.assert_f32_equal(y, c.want[a:b])


@pytest.mark.parametrize("f,gated", BIG, ids=BIG_IDS)
def test_rows_of_x_beyond_32_bits(gpu, f, gated):
    """x of M K > 2^32 elements: (m0 + sr) * K of the staging loads crosses 2^31 and 2^32 elements
    and 2^32 and 2^33 bytes. Peak 8.9 GB."""
    bm = f.tile()[0]
    m, wins = pe.big_x_rows(bm)
    k, n = pe.BIG_K, pe.BIG_N
    assert wins[0][0] == 0 and wins[-1][1] == m and (m - wins[-1][0]) % bm
    assert any(r0 * k < P2_31 < r1 * k for r0, r1 in wins) and any(r0 * k < P2_32 < r1 * k for r0, r1 in wins)
    assert 2 * m * k + 4 * m * n + (64 << 20) < 10 * GB  # x, y and the small calls
    assert (m * k) % P2_32 < m * k and ((m - 1) * k) % P2_31 + k <= m * k  # a wrapped row lies inside x
    c, run = _big_case(f, gated, sum(r1 - r0 for r0, r1 in wins), k)
    p = torch.from_numpy(c.img).to(DEV)
    torch.cuda.empty_cache()
    x = torch.empty(m, k, dtype=torch.bfloat16, device=DEV)
    try:
        xs, a = c.x.to(DEV), 0
        for r0, r1 in wins:
            x[r0:r1] = xs[a: a + r1 - r0]
            a += r1 - r0
        y = run(x, img=p, out_dtype=torch.float32)
        assert y.shape == (m, n)
        a = 0
        for r0, r1 in wins:
            b = a + r1 - r0
            small = run(xs[a:b], img=p, out_dtype=torch.float32)
            _check_small(c, gated, small, a, b)
            assert torch.equal(y[r0:r1].view(torch.int32), small.view(torch.int32)), (r0, r1)
            a = b
    finally:
        del x
        torch.cuda.empty_cache()


@pytest.mark.parametrize("f,gated", BIG, ids=BIG_IDS)
def test_rows_of_y_beyond_32_bits(gpu, f, gated):
    """y of 2^22 + 5 rows with a row stride of 528 f32: m * ldy crosses 2^30 (byte 2^32) and 2^31
    elements. Peak 9.2 GB."""
    bm = f.tile()[0]
    k, n, ld = 32, pe.BIG_N, 528
    m, wins = pe.big_y_rows(bm, ld)
    lead = 3 * ld + 8  # le.strided_out
    total = lead + (m + 3) * ld
    assert 4 * total + 2 * m * k + (64 << 20) < 10 * GB  # the 0xA5 buffer, x and the small calls
    assert any(r0 * ld < 1 << 30 < r1 * ld for r0, r1 in wins) and any(r0 * ld < P2_31 < r1 * ld for r0, r1 in wins)
    assert ((m - 1) * ld) % P2_31 + lead + ld <= total and (4 * (m - 1) * ld) % P2_32 + 4 * (lead + ld) <= 4 * total
    c, run = _big_case(f, gated, sum(r1 - r0 for r0, r1 in wins), k)
    p = torch.from_numpy(c.img).to(DEV)
    torch.cuda.empty_cache()
    x = torch.zeros(m, k, dtype=torch.bfloat16, device=DEV)
    buf = None
    try:
        xs, a = c.x.to(DEV), 0
        for r0, r1 in wins:
            x[r0:r1] = xs[a: a + r1 - r0]
            a += r1 - r0
        buf, y = le.strided_out(m, n, ld, torch.float32, DEV)
        assert buf.numel() == 4 * total and y.stride(0) == ld
        got = run(x, img=p, out=y)
        assert got.data_ptr() == y.data_ptr()
        words = buf.view(torch.int32)
        a5 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
        assert bool((words[:lead] == a5).all()) and bool((words[lead + m * ld:] == a5).all())
        full = words[lead: lead + m * ld].view(m, ld)
        a = 0
        for r0, r1 in wins:
            b = a + r1 - r0
            small = run(xs[a:b], img=p, out_dtype=torch.float32)
            _check_small(c, gated, small, a, b)
            assert torch.equal(full[r0:r1, :n], small.view(torch.int32)), (r0, r1)
            assert bool((full[r0:r1, n:] == a5).all()), (r0, r1)
            a = b
    finally:
        del x, buf
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 5. views of x

@pytest.mark.parametrize("gated", [False, True], ids=["linear", "swiglu"])
@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_views_of_x(gpu, f, gated):
    """x as [2, 9, k], as sliced and transposed non-contiguous views and as a contiguous view 2
    bytes off a 16-byte boundary: the bits of the contiguous, aligned x; leading dimensions kept."""
    k, n = 160, 48
    if gated:
        c = pe.swiglu_clean(f, 18, n, k)
        run = lambda x, **kw: pe.run_swiglu(c, DEV, x=x, img=p, tiled=True, **kw)
    else:
        c = pe.clean_case(f, 18, n, k)
        run = lambda x, **kw: pe.run_linear(c, DEV, x=x, img=p, tiled=True, **kw)
    p = torch.from_numpy(c.img).to(DEV)
    xd = c.x.to(DEV)
    base, base16 = run(xd, out_dtype=torch.float32), run(xd)
    if gated:
        pe.prove_swiglu(c)
        check_exact_regimes(base, c.g, c.u)
    else:
        le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
        le.assert_f32_equal(base, c.want)
    for name, v in le.x_views(xd).items():
        y = run(v, out_dtype=torch.float32)
        assert tuple(y.shape) == tuple(v.shape[:-1]) + (n,), name
        assert torch.equal(y.reshape(18, n).view(torch.int32), base.view(torch.int32)), name
        assert torch.equal(run(v).reshape(18, n).view(torch.int16), base16.view(torch.int16)), name
