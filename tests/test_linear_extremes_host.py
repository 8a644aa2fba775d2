"""The cases of linear_extremes.py through the CPU route of ops.mxfp4_linear, ops.fp8_linear and
ops.mxfp4_swiglu (out_dtype=torch.float32): the builders and their float64 expectations are shown
to be right here, on a machine without a GPU, before test_gpu_linear_extremes.py holds the gfx950
kernels to them. The expectation never uses the ops: numpy ref_unpack per chunk, float64 matmul."""
import numpy as np
import pytest
import torch

import linear_extremes as le
from linear_extremes import SHAPES
from test_gpu_mxfp4_swiglu import check_exact_regimes

F32 = dict(out_dtype=torch.float32)
FMT_BLOCKS = [("mxfp4", 32), ("fp8", 32), ("fp8", 128)]
# s = 100: normal products; s = 0: f32-subnormal products and sums. MXFP4 weights reach 6 * 2^-124, so at
# s = 0 few of its sums are subnormal: s = -8 (products up to 1.5 * 2^-127) puts its accumulators there
LOW_CASES = [(f, b, s) for f, b in FMT_BLOCKS for s in (100, 0)] + [("mxfp4", 32, -8)]


def _cpu(c, **kw):
    return le.run_linear(c, "cpu", **F32, **kw)


# ---------------------------------------------------------------- 1. the bottom of the range

@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("fmt,block,s", LOW_CASES)
def test_subnormal_weights(fmt, block, s, m, n, k):
    c = le.subnormal_weights(fmt, m, n, k, s, block)
    u = le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    assert u == (2.0 ** (s - 128) if fmt == "mxfp4" else 2.0 ** (s - 133))
    assert (np.abs(c.wf) < 2.0 ** -126).mean() > 0.2 and np.abs(c.wf).max() <= 6 * 2.0 ** -124
    if fmt == "fp8":
        assert (np.abs(c.wf) < 2.0 ** -126).all()
        pairs = le.fp8_pairs(c)
        assert all((sign | code, e) in pairs for code, e in le.FP8_ROUNDED for sign in (0, 0x80))  # all 48
    if s <= 0:
        # what "f32-subnormal products and accumulators come through" rests on, counted on the reference:
        # products of the first row of x, running sums over the 32-element blocks of K (a stand-in for
        # what an accumulator holds between MFMAs) and outputs that are non-zero and below 2^-126
        prod, run, out = le.subnormal_shares(c)
        print(fmt, block, s, (m, n, k), "f32-subnormal products %.4f, running sums %.4f, outputs %.4f"
              % (prod, run, out))
        assert np.abs(c.want).max() < 2.0 ** -104 and (c.want != 0).mean() > 0.9
        if (fmt, s) == ("mxfp4", 0):  # weights up to 6 * 2^-124: some products only, the sums are mostly normal
            assert prod > 0.01
        else:
            assert prod > 0.5 and run > 0.05 and out > 0.03
    le.assert_f32_equal(_cpu(c), c.want)


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("fmt,block", FMT_BLOCKS)
def test_subnormal_activations(fmt, block, m, n, k):
    c = le.subnormal_activations(fmt, m, n, k, block)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    assert (np.abs(c.xf) < 2.0 ** -126).all() and (c.xf != 0).all()
    nz = np.abs(c.wf[c.wf != 0])
    assert nz.min() >= 2.0 ** 97 and (np.abs(c.want[c.want != 0]) >= 2.0 ** -36).all()  # normal weights and sums
    le.assert_f32_equal(_cpu(c), c.want)


def _prove_swiglu(c):
    le.prove_exact(c.xf, c.wg, c.ux, c.ug, c.g)
    le.prove_exact(c.xf, c.wu, c.ux, c.uu, c.u)


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("which", ["gate", "up"])
def test_swiglu_subnormal_weights(which, m, n, k):
    c = le.swiglu_subnormal(which, m, n, k)
    _prove_swiglu(c)
    low, other, wlow = (c.g, c.u, c.wg) if which == "gate" else (c.u, c.g, c.wu)
    assert (np.abs(wlow) <= 6 * 2.0 ** -124).all() and (np.abs(wlow) < 2.0 ** -126).mean() > 0.2
    nz = np.abs(low[low != 0])
    assert nz.min() >= 2.0 ** -20 and nz.max() <= 2.0 ** 20 and (low != 0).mean() > 0.9
    assert np.abs(other).max() < 2.0 ** 125  # finite in f32, and so is silu(g) * u
    check_exact_regimes(le.run_swiglu(c, "cpu", **F32), c.g, c.u)


# ---------------------------------------------------------------- 2. the top of the range

@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("zeros", [False, True])
def test_mxfp4_overflow_to_inf(zeros, m, n, k):
    c = le.mxfp4_overflow(m, n, k, zeros)
    cl = c.extra["clean"]
    le.prove_exact(cl.xf, cl.wf, cl.ux, cl.uw, cl.want)
    rows = c.extra["rows"]
    w = c.want[:, rows]
    if zeros:
        assert np.isnan(w[:, :2]).any()  # 0 * inf in rows whose weights are all of one sign
    else:
        assert (w[:, 0] == np.inf).all() and (w[:, 1] == -np.inf).all() and np.isnan(w[:, 2:]).all()
    y = _cpu(c)
    le.assert_f32_equal(y, c.want)
    le.assert_rows_bit_equal(y.t(), _cpu(cl).t(), c.extra["keep"])


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("block", [32, 128])
def test_fp8_sums_overflow_f32(block, m, n, k):
    c = le.fp8_overflow(m, n, k, block)
    keep = c.extra["keep"]
    le.prove_exact(c.xf, c.wf[keep], c.ux, c.uw, c.want[:, keep])
    le.prove_exact(c.xf, c.wf[c.extra["warm"]], 1.0, 2.0 ** 117, c.want[:, c.extra["warm"]])
    assert np.isinf(c.want[:, c.extra["rows"]]).all() and {np.inf, -np.inf} <= set(c.want[0, c.extra["rows"]])
    le.assert_f32_equal(_cpu(c), c.want)


@pytest.mark.parametrize("m,n,k", [(5, 48, 96), (17, 48, 160), (65, 528, 1056)])
@pytest.mark.parametrize("fmt", ["mxfp4", "fp8"])
def test_nonfinite_activations(fmt, m, n, k):
    c = le.nonfinite_activations(fmt, n, k, m)
    le.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    clean = _cpu(c)
    le.assert_f32_equal(clean, c.want)
    for xb, _, want in c.extra["bad"].values():
        y = _cpu(c, x=xb)
        le.assert_f32_equal(y, want)
        le.assert_rows_bit_equal(y, clean, c.extra["keep"])


@pytest.mark.parametrize("m,n,k", [(5, 48, 96), (17, 48, 160), (65, 528, 1056)])
def test_swiglu_nonfinite_activations(m, n, k):
    c = le.swiglu_nonfinite(n, k, m)
    _prove_swiglu(c)
    clean = le.run_swiglu(c, "cpu", **F32)
    check_exact_regimes(clean, c.g, c.u)
    for xb, g, u in c.extra["bad"].values():
        y = le.run_swiglu(c, "cpu", x=xb, **F32)
        r = c.extra["row"]
        want = le.silu_mul64(g[r], u[r])
        assert not np.isfinite(want).any()
        le.assert_f32_equal(y[r], le.expected_f32(want).astype(np.float64))
        le.assert_rows_bit_equal(y, clean, c.extra["keep"])


# ---------------------------------------------------------------- 3. far into a large layer

@pytest.mark.parametrize("fmt", ["mxfp4", "fp8"])
def test_far_into_a_large_layer(fmt):
    """70 000 chunks of 64 KiB that are never touched, then S: element offsets beyond 2^31, and for
    fp8 packed bytes beyond 2^31 (MXFP4: 1.2 GB)."""
    c = le.far_case(fmt, 70_000, 32 * 700, m=5)
    assert c.elem_offset > 2 ** 31 and (c.first_byte > 2 ** 31 or fmt == "mxfp4")
    buf = c.place("cpu")
    le.assert_f32_equal(le.far_linear(c, buf, **F32), c.want)
    assert np.array_equal(le.mx.bf16_tensor_bits(le.far_unpack(c, buf)), c.bits)


def test_far_swiglu():
    c = le.far_case("mxfp4", 70_000, 32 * 3, m=5, up_s=32 * 3 + le.FAR_N * le.FAR_K + 64)
    buf = c.place("cpu")
    check_exact_regimes(le.far_swiglu(c, buf, **F32), c.want, c.xf @ c.wu.T)


# ---------------------------------------------------------------- 4. views of x

@pytest.mark.parametrize("fmt", ["mxfp4", "fp8", "swiglu"])
def test_views_of_x(fmt):
    k, n = 160, 48
    if fmt == "swiglu":
        c = le.swiglu_clean(18, n, k)
        run = lambda x: le.run_swiglu(c, "cpu", x=x, **F32)
    else:
        c = le.clean_case(fmt, 18, n, k)
        run = lambda x: le.run_linear(c, "cpu", x=x, **F32)
    base = run(c.x)
    if fmt != "swiglu":
        le.assert_f32_equal(base, c.want)
    for name, v in le.x_views(c.x).items():
        y = run(v)
        assert tuple(y.shape) == tuple(v.shape[:-1]) + (n,), name
        assert torch.equal(y.reshape(18, n).view(torch.int32), base.view(torch.int32)), name

