"""The W4A8 kernels (csrc/kernels/mxfp4_mx.hip, csrc/kernels/mxfp8_act.hip) on hand-made MXFP8
operands and at their numeric and addressing extremes. test_gpu_mxfp4_mx.py reaches the matmul
only through ops.*(act="mxfp8"), so its A operand is always what the quantizer makes; here the
codes and scale bytes of x go to the raw bindings (_core.mxfp4_linear_mx, _core.mxfp4_swiglu_mx)
by pointer. The cases, the float64 reference and the runner are mx_operands.py's; the host twin
test_mx_operands_host.py asserts on the reference alone that each case covers what it names and
that each defect (flushed subnormals, another block's scale byte, the A operand read as 32
consecutive k per lane, a code that falls out of the classes or into two) changes its expectation.

1. Builders a to e through the linear binding: f32 equal to the float64 expectation (a, b, c, d;
   f32 subnormals, both ends of both scale ranges and all 254 codes included) or within
   K 2^-23 sum |x^ w^| (e); the bf16 output is the f32 one rounded once.
2. The gated binding on a (both variants), c, d and e, gate and up in both orders and equal: against
   silu(g) u in float64 of the two raw f32 linears with test_gpu_mxfp4_swiglu.py's mixed_bound;
   where g u leaves f32 (a under bytes 0..254, e) the output is +-inf, and only within two bounds
   of f32's overflow threshold either (_hold_gated); check_exact_regimes where g and u are proven
   exact.
3. Non-finite: x scale byte 0xFF and the codes 0x7F / 0xFF make exactly their row NaN, a 0xFF weight
   scale its column; every other row carries the bits of the clean run, the bad row alone gives the
   same bits, the gated kernel has the linear's NaN rows and columns.
4. The quantizer joined in: rows of a and d whose bf16 form the host codec quantizes to exactly the
   hand-made operand give, through ops.mxfp4_linear(act="mxfp8"), the bits of the raw call.
5. Parameters behind and across 2^31 / 2^32 elements and packed bytes (the MXFP4 rows of the FAR
   tables of test_gpu_linear_extremes.py and packed_extremes.py, BM + 1 rows) and a parameter of
   BN + 16 rows whose second workgroup starts behind packed byte 2^32. Peak 4.7 GB.
6. M K just beyond 2^32 bytes of codes in one launch (K = 32, N = 16, bf16 y; peak 13.1 GB: 8.6 GB
   of x, written only where checked and freed once quantized, 4.3 GB of codes, then 4.3 GB of y),
   and 2^22 + 5 rows of y with a row stride of 528 f32 (peak 9.3 GB). Checked are the first tile,
   the tiles around each crossing and the last, partial tile: the quantizer's bytes against the
   host codec, y bit for bit against a small call on those rows that is itself held to float64.
7. What the raw launchers refuse before they launch."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import _core, ops

import mx_operands as mo
import packed_extremes as pe
import test_gpu_linear_extremes as gl4
import test_gpu_mxfp4_swiglu as glu
from mx_operands import BM, BN, KS
from packed_extremes import FAR_K, GB, P2_31, P2_32, le
from test_gpu_mxfp4_linear import LAYOUTS
from test_mxfp4_linear_host import bf16_tensor_bits, handmade_image
from test_mxfp4_mx_host import dequantize, host_quantize

pytestmark = pytest.mark.gpu

DEV = "cuda"
F4 = pe.FORMATS[0]


def _bits16(y32):
    return le.f32_to_bf16_bits(y32.cpu().numpy()).reshape(-1)


def _check_exact(c, **kw):
    """f32 output == the expectation, bf16 output == its rounding; returns the f32 output."""
    y32 = mo.run(c, **kw)
    le.assert_f32_equal(y32, c.want)
    le.assert_bf16_is_rounded(mo.run(c, bf16=True, **kw), c.want)
    return y32


F32_OVERFLOW = 2.0 ** 128 * (1 - 2.0 ** -25)  # from here on a real number rounds to +-inf in f32


def _hold_gated(y32, g, u):
    """A gated f32 output against silu(g) u in float64 of its two f32 sums, by mixed_bound. Where
    g u leaves f32: every v with |v - ref| <= bound is finite in f32 if |ref| + bound is below the
    overflow threshold - then y is held to the bound - and rounds to +-inf if |ref| - bound is at or
    above it - then y is that inf. Only in between, a band of 2 bounds (2^-20 of 2^128) around the
    threshold, may y be either. Returns (worst err / bound of the first group, elements of the second)."""
    y = y32.cpu().numpy().astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        ref = glu.silu_mul(g, u)
        bound = glu.mixed_bound(ref, u)
        err = np.abs(y - ref)
    assert np.isfinite(ref).all() and np.isfinite(bound).all()
    low, top = np.abs(ref) + bound < F32_OVERFLOW, np.abs(ref) - bound >= F32_OVERFLOW
    assert (err[low] <= bound[low]).all(), float((err[low] / bound[low]).max())
    assert np.array_equal(y[top], np.copysign(np.inf, ref[top]))
    band = ~(low | top)
    assert ((np.abs(ref[band]) > 2.0 ** 128 * (1 - 2.0 ** -19)) & (np.abs(ref[band]) < 2.0 ** 128 * (1 + 2.0 ** -19))).all()
    assert ((y[band] == np.copysign(np.inf, ref[band])) | (err[band] <= bound[band])).all()
    return float((err[low] / bound[low]).max()), int(top.sum())


def _check_gated(c, exact=None):
    """The gated binding with gate and up in both orders and equal, against silu(g) u in float64 of
    the two raw f32 linears (_hold_gated). `exact`: {order: (g, u, rows)} float64 expectations proven
    exact in f32."""
    exact = exact or {}
    p = mo.upload(c.img)
    lin = {o: mo.run(c, img=p, off=o).cpu().numpy().astype(np.float64) for o in (c.off, c.up)}
    for name, (gate, up) in {"gate first": (c.off, c.up), "up first": (c.up, c.off), "equal": (c.off, c.off)}.items():
        g, u = lin[gate], lin[up]
        y32 = mo.run(c, gated=True, img=p, off=gate, up=up)
        assert np.isfinite(g).all() and np.isfinite(u).all()
        worst, beyond = _hold_gated(y32, g, u)
        print(c.name, name, "worst err / bound", worst, "beyond f32", beyond)
        assert np.array_equal(bf16_tensor_bits(mo.run(c, gated=True, bf16=True, img=p, off=gate, up=up)), _bits16(y32))
        if name in exact:
            ge, ue, rows = exact[name]
            le.assert_f32_equal(torch.from_numpy(lin[gate][rows].astype(np.float32)), ge[rows])
            glu.check_exact_regimes(y32[rows], ge[rows], ue[rows])


# ---------------------------------------------------------------- 1, 2. the builders

@pytest.mark.parametrize("mid", [False, True], ids=["bytes 0..254", "bytes 100..140"])
@pytest.mark.parametrize("k", KS)
def test_a_reads_out_x_through_an_identity_weight(gpu, k, mid):
    """y = x^ bit for bit: all 254 codes in every byte lane and piece under scale bytes that differ
    inside every step, f32 subnormals included (the instruction neither flushes nor rounds them:
    profiles/mxfp4_mx/mxprobe.jsonl). The variant with bytes 100..140 stands on its own. Both go
    through the gated binding too; under bytes 0..254, where |x^| reaches 2^127, the up parameter
    has scale bytes 59..61 so that its f32 sums stay finite, and silu(g) u leaves f32 in part."""
    c = mo.readout_a(k, mid)
    _check_exact(c)
    _check_gated(c)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k", KS)
def test_b_reads_out_w_through_a_one_hot_x(gpu, k, layout):
    """y[m][n] = nibble * 2^(byte - 127) bit for bit, for all 16 nibbles under scale bytes 0..254."""
    c = mo.readout_b(k, layout)
    assert np.array_equal(c.want, mo.w_values(c.extra["nib"], c.extra["sb"]).T)
    _check_exact(c)


@pytest.mark.parametrize("live", [1, 2])
@pytest.mark.parametrize("k", KS)
def test_c_every_block_meets_its_own_scale(gpu, k, live):
    c = mo.association(k, live)
    up = c.up_weight()
    mo.prove_rows(c)
    mo.prove_rows(c, wf=up)
    _check_exact(c)
    rows = np.arange(c.m)
    u = mo.matmul64(c.xh, up)
    _check_gated(c, exact={"gate first": (c.want, u, rows), "up first": (u, c.want, rows), "equal": (c.want, c.want, rows)})


@pytest.mark.parametrize("k", [160, 288])
def test_d_class_boundaries_inside_a_group_of_8(gpu, k):
    """The ends of every class and the codes on either side of every class boundary in one group
    of 8, the large terms cancelling: exact, so the three per-class MFMAs sum the group exactly. The
    rows with the ends of all three classes in one group are held to the f32 chain class 0 -> 1 -> 2,
    which rounds nowhere on them; the rows of seven 0x7E and one subnormal sum to a tie between two
    f32 neighbours in columns 7 and 15, which the chain's round to nearest even decides."""
    c = mo.boundaries(k)
    plain = np.nonzero(~c.extra["mixed"])[0]
    mo.prove_rows(c, rows=plain)
    assert np.array_equal(c.want[plain], c.extra["float64"][plain])
    _check_exact(c)
    _check_gated(c, exact={"equal": (c.want, c.want, plain)})


def test_e_wide_scales_within_the_f32_bound(gpu):
    c = mo.wide()
    y32 = mo.run(c)
    err, bound = np.abs(y32.cpu().numpy().astype(np.float64) - c.want), mo.f32_bound(c.xh, c.wf)
    print("max err / bound", float((err / bound).max()))
    assert (err <= bound).all()
    assert np.array_equal(bf16_tensor_bits(mo.run(c, bf16=True)), _bits16(y32))
    _check_gated(c)


# ---------------------------------------------------------------- 3. non-finite

@pytest.fixture(scope="module")
def nonfinite(gpu):
    """(clean case, variants, {id of an image: its upload and its clean runs}): the clean runs are
    made once and shared by the two parametrisations."""
    c, variants = mo.nonfinite()
    return c, variants, {}


def _baseline(c, img):
    """(image on the GPU, linear on gate, linear on up, gated) of the clean x on `img`, each held to
    the reference outside the image's NaN columns."""
    p = mo.upload(img)
    b32, bup, bglu = mo.run(c, img=p), mo.run(c, img=p, off=c.up), mo.run(c, img=p, gated=True)
    for y, off in ((b32, c.off), (bup, c.up)):
        wf = le.mx.ref_weight(img, c.total, c.chunk, off, c.n, c.k)
        cols = np.isfinite(wf).all(1)
        assert cols.sum() >= c.n - 1
        got = y.cpu().numpy().astype(np.float64)
        assert np.isnan(got[:, ~cols]).all()
        assert (np.abs(got - mo.matmul64(c.xh, wf))[:, cols] <= mo.f32_bound(c.xh, wf[cols])).all()
    g, u = (t.cpu().numpy().astype(np.float64) for t in (b32, bup))
    cols = ~np.isnan(g).any(0)
    assert np.isnan(bglu.cpu().numpy()[:, ~cols]).all()
    _hold_gated(bglu.cpu()[:, torch.from_numpy(np.nonzero(cols)[0])], g[:, cols], u[:, cols])
    return p, b32, bup, bglu


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("kind", ["x scale", "x code"])
def test_f_nan_rows_and_columns(nonfinite, kind):
    c, variants, base = nonfinite
    seen = 0
    for v in variants:
        if not v["name"].startswith(kind):
            continue
        seen += 1
        if id(v["img"]) not in base:
            base[id(v["img"])] = _baseline(c, v["img"])
        p, b32, bup, bglu = base[id(v["img"])]
        want_nan = np.isnan(mo.variant_want(c, v))
        r = v["rows"][0]
        keep = [i for i in range(c.m) if i != r]
        assert want_nan[r].all() and np.array_equal(want_nan[keep], np.isnan(b32.cpu().numpy())[keep]), v["name"]
        kw = dict(codes=v["codes"], scales=v["scales"], img=p)
        y = mo.run(c, **kw)
        assert np.array_equal(np.isnan(y.cpu().numpy()), want_nan), v["name"]
        assert _same_bits(y[keep], b32[keep]), v["name"]
        assert _same_bits(mo.run(c, rows=slice(r, r + 1), **kw), y[r: r + 1]), v["name"]
        y16 = mo.run(c, bf16=True, **kw)
        assert np.array_equal(np.isnan(y16.float().cpu().numpy()), want_nan), v["name"]
        yg = mo.run(c, gated=True, **kw)
        nan_up = np.isnan(mo.run(c, off=c.up, **kw).cpu().numpy())
        assert nan_up[r].all() and not nan_up[keep].any()
        assert np.array_equal(np.isnan(yg.cpu().numpy()), want_nan | nan_up), v["name"]
        assert _same_bits(yg[keep], bglu[keep]), v["name"]
        assert _same_bits(mo.run(c, gated=True, rows=slice(r, r + 1), **kw), yg[r: r + 1]), v["name"]
    assert seen == {"x scale": 12, "x code": 20}[kind]


# ---------------------------------------------------------------- 4. the quantizer joined in

@pytest.mark.parametrize("name,k", [("a", 160), ("a", 224), ("a", 288), ("d", 160), ("d", 288)])
def test_the_quantizer_and_the_raw_call_agree(gpu, name, k):
    c = mo.readout_a(k) if name == "a" else mo.boundaries(k)
    x, rows = mo.rows_the_quantizer_makes(c, host_quantize)
    print(c.name, "rows the quantizer makes:", len(rows), "of", c.m)
    assert len(rows) >= 1
    xr = x[rows].cuda()
    q, s = ops.mxfp8_quantize_rows(xr)
    assert np.array_equal(q.cpu().numpy(), c.codes[rows]) and np.array_equal(s.cpu().numpy(), c.scales[rows])
    p = mo.upload(c.img)
    raw = mo.run(c, img=p, rows=rows)
    le.assert_f32_equal(raw, c.want[rows])
    kw = dict(src_bytes=2 * c.total, chunk_bytes=c.chunk, elem_offset=c.off, act="mxfp8")
    assert _same_bits(ops.mxfp4_linear(xr, p, c.n, c.k, out_dtype=torch.float32, **kw), raw)
    y16 = ops.mxfp4_linear(xr, p, c.n, c.k, **kw)
    assert torch.equal(y16.view(torch.int16), mo.run(c, img=p, rows=rows, bf16=True).view(torch.int16))


# ---------------------------------------------------------------- 5. far into a large layer

def _far_run(c, gated):
    """act="mxfp8" on the case's (gate) parameter and, for a pair, the gated kernel, behind one
    allocation. x holds integers in [-8, 8], which the quantizer keeps: x^ = x."""
    assert np.array_equal(dequantize(*host_quantize(c.x)), c.xf)
    le.prove_exact(c.xf, c.wf, 1.0, F4.uw, c.want)
    assert c.need < 5 * GB and pe.wrapped_inside(c)
    torch.cuda.empty_cache()
    buf = c.place(DEV)
    try:
        le.assert_f32_equal(pe.far_linear(c, buf, act="mxfp8", out_dtype=torch.float32), c.want)
        le.assert_bf16_is_rounded(pe.far_linear(c, buf, act="mxfp8"), c.want)
        if gated:
            u = c.xf @ c.wu.T
            le.prove_exact(c.xf, c.wu, 1.0, F4.uw, u)
            y32 = pe.far_swiglu(c, buf, act="mxfp8", out_dtype=torch.float32)
            glu.check_exact_regimes(y32, c.want, u)
            assert np.array_equal(bf16_tensor_bits(pe.far_swiglu(c, buf, act="mxfp8")), _bits16(y32))
    finally:
        del buf
        torch.cuda.empty_cache()


FAR_LINEAR = {k: v for k, v in gl4.FAR.items() if v[0] == "mxfp4"}
FAR_PAIRS = {k: v for k, v in {**pe.FAR_GLU_MXFP4, **pe.FAR_GLU}.items() if v[0].name == "mxfp4"}


@pytest.mark.parametrize("name", list(FAR_LINEAR))
def test_far_linear_table(gpu, name):
    assert len(FAR_LINEAR) == 4
    _, c0, boundary, packed = FAR_LINEAR[name]
    off_s = 32 * 700
    if c0 is None:
        c0, off_s = pe.crossing_c0(F4, boundary, packed)
    c = pe.far_case(F4, c0, off_s, m=BM + 1, n=64 if "64 rows" in name else pe.FAR_N)
    pe.assert_far_position(c, boundary, packed)
    _far_run(c, False)


@pytest.mark.parametrize("name", list(FAR_PAIRS))
def test_far_gate_up_pairs(gpu, name):
    assert len(FAR_PAIRS) == 2
    _far_run(pe.far_glu_case(name, m=BM + 1), True)


def test_far_parameter_whose_second_workgroup_starts_behind_packed_byte_2_32(gpu):
    """A gate / up pair of BN + 16 rows each; the gate's codes cross packed byte 2^32 in its first
    rows, so the linear's second workgroup (row BN) and the gated kernel's second and third (rows
    BN / 2 and BN) start from positions behind it."""
    n = BN + 16
    c0, gate = pe.crossing_c0(F4, P2_32, True)
    up = gate + n * FAR_K + 64
    c = pe.far_case(F4, c0, gate, m=BM + 1, n=n, up_s=up, chunks=-(-(up + n * FAR_K) // (pe.FAR_CHUNK // 2)))
    pe.assert_far_position(c, P2_32, True)
    for row in (BN // 2, BN):
        assert int(le.mxfp4_index(c.src_bytes // 2, pe.FAR_CHUNK, c.elem_offset + row * FAR_K)[0]) > P2_32
    _far_run(c, True)


# ---------------------------------------------------------------- 6. rows of x and of y beyond 32 bits

BIG_K, BIG_N = 32, 16


def _big_case(rows):
    c = le.clean_case("mxfp4", rows, BIG_N, BIG_K)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    assert np.array_equal(dequantize(*host_quantize(c.x)), c.xf)
    return c


def test_rows_of_codes_beyond_32_bits(gpu):
    """M = 2^27 + 2 BM + 5 rows of K = 32: the quantizer's thread index passes 2^29 (x byte 2^33), the
    launcher's (m0 + sr) * K passes 2^31 and 2^32 bytes of codes and m * ldy 2^31 elements and 2^32
    bytes of the bf16 y. Peak 13.1 GB (x 8.6 GB and codes 4.3 GB with their scale bytes; x is freed
    before y, 4.3 GB, is allocated). Rows that read uninitialised x are not looked at."""
    k, n = BIG_K, BIG_N
    m = P2_32 // k + 2 * BM + 5
    wins = pe._windows(m, BM, [P2_31 // k - 1, P2_31 // k, P2_32 // k - 1, P2_32 // k])
    assert wins[0][0] == 0 and wins[-1][1] == m and (m - wins[-1][0]) % BM and m * k > P2_32
    assert any(r0 * k < P2_31 < r1 * k for r0, r1 in wins) and any(r0 * k < P2_32 < r1 * k for r0, r1 in wins)
    assert any(r0 * n < P2_31 < r1 * n for r0, r1 in wins)
    assert (m * k) % P2_32 < m * k and ((m - 1) * k) % P2_31 + k <= m * k  # a wrapped row lies inside the buffers
    assert 3 * m * k + m * k // 32 + (64 << 20) < 14 * GB
    c = _big_case(sum(r1 - r0 for r0, r1 in wins))
    hq, hs = host_quantize(c.x)
    p = mo.upload(c.img)
    torch.cuda.empty_cache()
    x = torch.empty(m, k, dtype=torch.bfloat16, device=DEV)
    q = s = y = None
    try:
        xs, a = c.x.to(DEV), 0
        for r0, r1 in wins:
            x[r0:r1] = xs[a: a + r1 - r0]
            a += r1 - r0
        q, s = ops.mxfp8_quantize_rows(x)
        torch.cuda.synchronize()
        del x
        torch.cuda.empty_cache()
        assert q.shape == (m, k) and s.shape == (m, 1) and q.data_ptr() % 16 == 0
        y = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)
        _core.mxfp4_linear_mx(p.data_ptr(), 2 * c.total, c.chunk, c.off, q.data_ptr(), s.data_ptr(), m, n, k, y.data_ptr(),
                              n, True, torch.cuda.current_stream().cuda_stream)
        a = 0
        for r0, r1 in wins:
            b = a + r1 - r0
            assert np.array_equal(q[r0:r1].cpu().numpy(), hq[a:b]) and np.array_equal(s[r0:r1].cpu().numpy(), hs[a:b]), (r0, r1)
            small = pe.run_linear(c, DEV, x=xs[a:b], img=p, act="mxfp8")
            le.assert_bf16_is_rounded(small, c.want[a:b])
            assert torch.equal(y[r0:r1].view(torch.int16), small.view(torch.int16)), (r0, r1)
            a = b
    finally:
        del q, s, y
        torch.cuda.empty_cache()


def test_rows_of_y_beyond_32_bits(gpu):
    """y of 2^22 + 5 rows with a row stride of 528 f32 in a 0xA5-filled buffer: m * ldy crosses 2^30
    (byte 2^32) and 2^31 elements. Peak 9.3 GB."""
    k, n, ld = BIG_K, BIG_N, 528
    m, wins = pe.big_y_rows(BM, ld)
    lead = 3 * ld + 8  # le.strided_out
    total = lead + (m + 3) * ld
    assert 4 * total + 3 * m * k + (64 << 20) < 10 * GB
    assert any(r0 * ld < 1 << 30 < r1 * ld for r0, r1 in wins) and any(r0 * ld < P2_31 < r1 * ld for r0, r1 in wins)
    assert ((m - 1) * ld) % P2_31 + lead + ld <= total and (4 * (m - 1) * ld) % P2_32 + 4 * (lead + ld) <= 4 * total
    c = _big_case(sum(r1 - r0 for r0, r1 in wins))
    p = mo.upload(c.img)
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
        hq, hs = host_quantize(c.x)
        q, s = ops.mxfp8_quantize_rows(x)
        a = 0
        for r0, r1 in wins:  # the quantizer's bytes on each window (its large index: the test above)
            b = a + r1 - r0
            assert np.array_equal(q[r0:r1].cpu().numpy(), hq[a:b]) and np.array_equal(s[r0:r1].cpu().numpy(), hs[a:b]), (r0, r1)
            a = b
        del q, s
        got = pe.run_linear(c, DEV, x=x, img=p, act="mxfp8", out=y)
        assert got.data_ptr() == y.data_ptr()
        words = buf.view(torch.int32)
        a5 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
        assert bool((words[:lead] == a5).all()) and bool((words[lead + m * ld:] == a5).all())
        full = words[lead: lead + m * ld].view(m, ld)
        a = 0
        for r0, r1 in wins:
            b = a + r1 - r0
            small = pe.run_linear(c, DEV, x=xs[a:b], img=p, act="mxfp8", out_dtype=torch.float32)
            le.assert_f32_equal(small, c.want[a:b])
            assert torch.equal(full[r0:r1, :n], small.view(torch.int32)), (r0, r1)
            assert bool((full[r0:r1, n:] == a5).all()), (r0, r1)
            a = b
    finally:
        del x, buf
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 7. rejections

def test_the_raw_launchers_reject_before_they_launch(gpu):
    """Codes off a 16-byte boundary, no scale bytes, a row stride of y below N, K beyond the
    launcher's limit: an error from the host-side checks, nothing is launched."""
    n, k, chunk = 64, 96, 1024
    total = 2 * n * k
    p = mo.upload(handmade_image(total, chunk, 1))
    q = torch.zeros(5 * k + 16, dtype=torch.uint8, device=DEV)
    s = torch.full((5, k // 32), 127, dtype=torch.uint8, device=DEV)
    y = torch.full((5, n), 7.0, dtype=torch.float32, device=DEV)
    assert q.data_ptr() % 16 == 0
    good = dict(x_codes=q.data_ptr(), x_scales=s.data_ptr(), m=5, n=n, k=k, y=y.data_ptr(), ldy=n, y_bf16=False)
    for fn, offs in ((gpu.mxfp4_linear_mx, dict(elem_off=32)), (gpu.mxfp4_swiglu_mx, dict(gate_off=32, up_off=n * k))):
        head = dict(packed=p.data_ptr(), src_bytes=2 * total, src_chunk=chunk, **offs)
        fn(**head, **good)
        torch.cuda.synchronize()
        assert bool((y == 0).all())  # zero codes: the good call ran
        y.fill_(7.0)
        for bad in (dict(x_codes=q.data_ptr() + 1), dict(x_codes=q.data_ptr() + 8), dict(x_scales=0), dict(ldy=n - 1),
                    dict(k=0x7FFFFFA0)):
            with pytest.raises(RuntimeError):
                fn(**head, **{**good, **bad})
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())  # nothing was written

