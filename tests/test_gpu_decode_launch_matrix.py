"""The six gfx950 decode kernels (csrc/kernels/{mxfp4,fp8,mxfp6}_{linear,swiglu}.hip) at every launch
shape their launchers choose: the matrix of decode_launch_matrix.py - every template instantiation at
1, 2, 3 slices, at its most and at every slice count a served model reaches, with K that give every
wave one step, an uneven split with idle waves, and four steps on every wave (16 real partials in the
LDS reduction at 16 slices). test_decode_launch_matrix_host.py shows on the CPU that the matrix holds
every served plan, that each case's forced arguments give the plan it names, and that its inputs are
exact in f32 in any summation order and any slicing.

Per case: the f32 output equals the float64 x W^T exactly (the gated kernels: check_exact_regimes on
exact g and u); the bf16 output is the f32 one rounded once; both are written into a strided `out`
inside a 0xA5-filled buffer whose every byte outside y[:m, :n] stays (an LDS or index overrun of the
reduction shows there first). At an instantiation's most slices a second call gives equal bits, and a
gated kernel's result is silu(g) * u of the linear kernel's g and u with the same forced split_k."""
import numpy as np
import pytest
import torch

import decode_launch_matrix as dm
import linear_extremes as le
from test_gpu_mxfp4_swiglu import check_exact_regimes, mixed_bound, silu_mul

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (kernel, format, mt, nt): the cases of one (n, k) lie in adjacent tests, which share its reference
PARAMS = [(kernel, f, mt, nt) for kernel in dm.KERNELS for f in dm.formats(kernel)
          for mt, nt in sorted(dm.INSTANTIATIONS[dm.kind(kernel)], key=lambda i: i[::-1])]
UNFORCED = [(kernel, f) for kernel in dm.KERNELS for f in dm.formats(kernel) if f.block != 512]


def _f64(y):
    return y.contiguous().cpu().numpy().astype(np.float64)


def _run_into_strided(b, p, dtype):
    """The case's result in a strided view of a 0xA5-filled buffer, and nothing written around it."""
    ld = b.n + 20
    buf, y = le.strided_out(b.m, b.n, ld, dtype, DEV)
    got = b.run(DEV, img=p, out=y)
    assert got.data_ptr() == y.data_ptr() and y.stride(0) == ld and y.dtype == dtype
    le.assert_untouched_outside(buf, b.m, b.n, ld, dtype)
    return y.contiguous()


def _check(kernel, f, case):
    b = dm.Built(kernel, f, case)
    p = torch.from_numpy(b.img).to(DEV)
    y32 = _run_into_strided(b, p, torch.float32)
    if b.gated:
        check_exact_regimes(y32, *b.wants)
    else:
        got, want = _f64(y32), b.wants[0]
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (case, len(bad), [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in bad[:6]])
    y16 = _run_into_strided(b, p, torch.bfloat16)
    le.assert_bf16_is_rounded(y16, _f64(y32))
    if not dm.at_most_slices(kernel, case):
        return
    again = b.run(DEV, img=p, out_dtype=torch.float32)
    assert torch.equal(again.view(torch.int32), y32.view(torch.int32)), case
    if b.gated:  # the K-partition contract: the fused kernel's sums are the linear kernel's
        g, u = (_f64(b.run(DEV, img=p, linear_of=i, out_dtype=torch.float32)) for i in (0, 1))
        assert np.array_equal(g, b.wants[0]) and np.array_equal(u, b.wants[1])
        ref = silu_mul(g, u)
        assert (np.abs(_f64(y32) - ref) <= mixed_bound(ref, u)).all(), case


@pytest.mark.parametrize("kernel,f,mt,nt", PARAMS, ids=[f"{k}-{f.id}-mt{mt}-nt{nt}" for k, f, mt, nt in PARAMS])
def test_instantiation_at_every_slice_count(gpu, kernel, f, mt, nt):
    cases = dm.cases_of(kernel, f, mt, nt)
    assert cases and {c[2] for c in cases} >= {dm.max_slices(kernel, mt, nt)}
    for case in sorted(cases, key=lambda c: c[5]):
        _check(kernel, f, case)
    print(kernel, f.id, (mt, nt), len(cases), "cases, slices", sorted({c[2] for c in cases}))


@pytest.mark.parametrize("kernel,f", UNFORCED, ids=[f"{k}-{f.id}" for k, f in UNFORCED])
def test_the_launchers_own_choice_where_n_alone_decides(gpu, kernel, f):
    """N = 4096 and 16384 with nothing forced: the launcher's rule itself takes 2 and 4 row tiles
    (gated: 1 and 2 pairs), as the host test asserts of the plan."""
    for case in dm.MATRIX[kernel]:
        if dm.is_unforced(case):
            _check(kernel, f, case)
