"""The cases of mxfp6_linear_extremes.py through the CPU route of ops.mxfp6_linear
(out_dtype=torch.float32): the builders and their float64 expectations are shown to be right
here, on a machine without a GPU, before test_gpu_mxfp6_linear_extremes.py holds the gfx950 kernel
to them. The expectation never uses the ops: numpy ref_unpack per chunk, float64 matmul."""
import numpy as np
import pytest
import torch

import mxfp6_linear_extremes as e6
from mxfp6_linear_extremes import SHAPES

F32 = dict(out_dtype=torch.float32)


def _cpu(c, **kw):
    return e6.run_linear(c, "cpu", **F32, **kw)


# ---------------------------------------------------------------- 1. the bottom of the range

@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("s", [100, 0, -8])
def test_subnormal_weights(s, m, n, k):
    c = e6.subnormal_weights(m, n, k, s)
    u = e6.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    assert u == 2.0 ** (s - 130) >= 2.0 ** -149
    assert (np.abs(c.wf) < 2.0 ** -126).mean() > 0.2 and np.abs(c.wf).max() <= 7.5 * 2.0 ** -124
    assert np.abs(c.wf[c.wf != 0]).min() == 2.0 ** -130  # the smallest: code 1 under scale byte 0
    if s <= 0:  # f32-subnormal products; sums and outputs far below anything a flushed product would leave
        prod = np.abs(c.xf[0][None, :] * c.wf)
        assert (prod[prod != 0] < 2.0 ** -126).mean() > (0.5 if s < 0 else 0.01)
        assert np.abs(c.want).max() < 2.0 ** -100 and (c.want != 0).mean() > 0.9
    e6.assert_f32_equal(_cpu(c), c.want)


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_subnormal_activations(m, n, k):
    c = e6.subnormal_activations(m, n, k)
    e6.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    assert (np.abs(c.xf) < 2.0 ** -126).all() and (c.xf != 0).all()
    nz = np.abs(c.wf[c.wf != 0])
    assert nz.min() >= 2.0 ** 97 and (np.abs(c.want[c.want != 0]) >= 2.0 ** -36).all()  # normal weights and sums
    e6.assert_f32_equal(_cpu(c), c.want)


# ---------------------------------------------------------------- 2. the top of the range

@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("zeros", [False, True])
def test_overflow_to_inf(zeros, m, n, k):
    c = e6.overflow(m, n, k, zeros)
    cl = c.extra["clean"]
    e6.prove_exact(cl.xf, cl.wf, cl.ux, cl.uw, cl.want)
    rows = c.extra["rows"]
    w = c.want[:, rows]
    if zeros:
        assert np.isnan(w[:, :2]).any()  # 0 * inf in rows whose weights are all of one sign
    else:
        assert (w[:, 0] == np.inf).all() and (w[:, 1] == -np.inf).all() and np.isnan(w[:, 2:]).all()
    y = _cpu(c)
    e6.assert_f32_equal(y, c.want)
    e6.assert_rows_bit_equal(y.t(), _cpu(cl).t(), c.extra["keep"])


@pytest.mark.parametrize("m,n,k", [(5, 48, 96), (17, 48, 160), (65, 528, 1056)])
def test_nonfinite_activations(m, n, k):
    c = e6.nonfinite_activations(n, k, m)
    e6.prove_exact(c.xf, c.wf, c.ux, c.uw, c.want)
    clean = _cpu(c)
    e6.assert_f32_equal(clean, c.want)
    for xb, _, want in c.extra["bad"].values():
        y = _cpu(c, x=xb)
        e6.assert_f32_equal(y, want)
        e6.assert_rows_bit_equal(y, clean, c.extra["keep"])


# ---------------------------------------------------------------- 3. far into a large layer

def test_far_into_a_large_layer():
    """70 000 chunks of 64 KiB that are never touched, then S: element offsets beyond 2^31 (1.8 GB
    of packed bytes, allocated and not written)."""
    c = e6.far_case(70_000, 32 * 700, m=5)
    assert c.elem_offset > 2 ** 31 and c.total_s % (e6.FAR_CHUNK // 2) // 32 % 2 == 1
    e6.prove_exact(c.xf, c.wf, 1.0, 2.0 ** -4, c.want)
    buf = c.place("cpu")
    e6.assert_f32_equal(e6.far_linear(c, buf, **F32), c.want)
    assert np.array_equal(e6.m6.bf16_tensor_bits(e6.far_unpack(c, buf)), c.bits)


def test_far_cases_cross_the_boundaries_they_name():
    """The (c0, off_s) the GPU twin uses, on the reference alone."""
    c0, off_s = e6.crossing_c0(1 << 31, False)
    first = c0 * (e6.FAR_CHUNK // 2) + off_s
    assert first < 1 << 31 < first + e6.FAR_N * e6.FAR_K
    c0, off_s = e6.crossing_c0(1 << 32, True)
    total = c0 * (e6.FAR_CHUNK // 2) + 3 * (e6.FAR_CHUNK // 2) + 32 * 143
    first, last = (int(e6.mxfp6_index(total, e6.FAR_CHUNK, c0 * (e6.FAR_CHUNK // 2) + off_s + d)[0])
                   for d in (0, e6.FAR_N * e6.FAR_K - 1))
    assert first < 1 << 32 < last and off_s + e6.FAR_N * e6.FAR_K <= 3 * (e6.FAR_CHUNK // 2) + 32 * 143


# ---------------------------------------------------------------- 4. views of x

def test_views_of_x():
    k, n = 160, 48
    c = e6.clean_case(18, n, k)
    base = _cpu(c)
    e6.assert_f32_equal(base, c.want)
    for name, v in e6.x_views(c.x).items():
        y = _cpu(c, x=v)
        assert tuple(y.shape) == tuple(v.shape[:-1]) + (n,), name
        assert torch.equal(y.reshape(18, n).view(torch.int32), base.view(torch.int32)), name
