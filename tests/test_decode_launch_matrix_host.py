"""decode_launch_matrix.py on a machine without a GPU: the plan functions of the six decode
launchers (host code in csrc/kernels/*_linear.hip and *_swiglu.hip, bound as _core.*_plan) against
the matrix that test_gpu_decode_launch_matrix.py runs.

The condition that keeps the GPU file honest is the first test: every (mt, nt, slices) a launcher
picks for a projection of a served model, at any m of a pass, is a triple of the matrix - no share of
them may be missing. A retune of row_tiles() / pairs() / auto_slices() / max_slices() that leaves the
tested set fails here before anything is served untested. The rest shows that no case is clipped into
another instantiation, that the older *_slices bindings are the plan's third value, that every case's
inputs meet the exactness conditions on the inputs themselves, and that builders and float64
expectations agree with the ops' CPU route."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import _core

import decode_launch_matrix as dm
from test_gpu_mxfp4_swiglu import check_exact_regimes

F32 = dict(out_dtype=torch.float32)


def _triples(kernel):
    return {c[:3] for c in dm.MATRIX[kernel]}


@pytest.mark.parametrize("kernel", dm.KERNELS)
def test_every_served_plan_is_in_the_matrix(kernel):
    served = dm.served_plans(kernel)
    assert len(dm.served_shapes(kernel)) == (3 if dm.kind(kernel) == "swiglu" else 18) and len(served) >= 10
    missing = served - _triples(kernel)
    print(kernel, "served plans", sorted(served))
    assert not missing, sorted(missing)
    # and the table holds nothing stale: it is exactly what the served plans ask for beyond 1, 2, 3 and the most
    extra = {}
    for mt, nt, s in served:
        if s not in (1, 2, 3, dm.max_slices(kernel, mt, nt)):
            extra.setdefault((mt, nt), set()).add(s)
    assert extra == {i: set(v) for i, v in dm.SERVED_SLICES[kernel].items()}


@pytest.mark.parametrize("kernel", dm.KERNELS)
def test_every_instantiation_runs_at_one_slice_and_at_its_most(kernel):
    insts = dm.INSTANTIATIONS[dm.kind(kernel)]
    assert len(insts) == (6 if dm.kind(kernel) == "swiglu" else 10)
    for mt, nt in insts:
        top = dm.max_slices(kernel, mt, nt)
        assert top == dm.plan(kernel, 16 * mt, 48 * nt, 8192, 16, nt)[2]  # what the launcher clips a forced 16 to
        tiles = mt * nt * (2 if dm.kind(kernel) == "swiglu" else 1)  # accumulator tiles of a wave: 1 KiB of LDS each
        assert top * tiles <= 64 and top == (16 if tiles <= 2 else 8)
        assert {(mt, nt, 1), (mt, nt, 2), (mt, nt, 3), (mt, nt, top)} <= _triples(kernel)
        for s in dm.slice_counts(kernel, mt, nt):  # both m and every K of every slice count
            got = {c[3:6] for c in dm.MATRIX[kernel] if c[:3] == (mt, nt, s) and not dm.is_unforced(c)}
            assert got == {(m, 48 * nt, k) for m in (16 * mt - 3, 16 * mt) for k in dm.k_cases(s)}
    # no plan names an instantiation outside the switch
    assert {c[:2] for c in dm.MATRIX[kernel]} == set(insts) and {p[:2] for p in dm.served_plans(kernel)} <= set(insts)


@pytest.mark.parametrize("kernel", dm.KERNELS)
def test_every_case_gets_the_plan_it_names(kernel):
    """With the case's forced arguments the launcher's plan is the case's triple: nothing is clipped
    into another instantiation or slice count. The K of a case place the steps as the matrix says."""
    for mt, nt, s, m, n, k, split_k, row_tiles in dm.MATRIX[kernel]:
        assert dm.plan(kernel, m, n, k, split_k, row_tiles) == (mt, nt, s)
        assert mt == (m + 15) // 16 and n % (16 * nt) == 0 and k % 32 == 0 and k <= dm.K_LONGEST
    for s in range(1, 17):
        shape = [(k // 128, k // 32 % 4, -(-(k // 128) // s)) for k in dm.k_cases(s)[:3]]  # (steps, tail, per wave)
        assert shape == [(s, 1, 1), (2 * s + 1, 3, 3), (4 * s, 0, 4)]
        assert s < 4 or -(-(2 * s + 1) // 3) < s  # waves without a step behind the uneven one
    if dm.max_slices(kernel, 1, 1) == 16:
        assert dm.k_cases(16)[3] == 8288 == max(c[5] for c in dm.MATRIX[kernel])


@pytest.mark.parametrize("kernel", dm.KERNELS)
def test_the_two_cases_that_n_alone_decides(kernel):
    small, large = [c for c in dm.MATRIX[kernel] if dm.is_unforced(c)]
    assert small[3:6] == (13, 4096, 288) and large[3:6] == (13, 16384, 288)
    if dm.kind(kernel) == "linear":
        assert (small[1], large[1]) == (2, 4)
    else:  # 2 N / 16 tiles against 1024: 512 at N = 4096
        assert (small[1], large[1]) == (1, 2)


@pytest.mark.parametrize("kernel", dm.KERNELS)
def test_slices_binding_is_the_plans_third_value(kernel):
    slices = getattr(_core, kernel + "_slices")
    for _, _, n, k in dm.served_shapes(kernel):
        for m in list(range(1, 66)) + [127, 128, 129, 4096]:
            assert slices(m, n, k) == dm.plan(kernel, min(m, 64), n, k, 0, 0)[2]


@pytest.mark.parametrize("kernel", dm.KERNELS)
def test_plan_rejects_what_the_launcher_rejects(kernel):
    for bad in [(0, 48, 160, 0, 0), (65, 48, 160, 0, 0), (5, 40, 160, 0, 0), (5, 48, 144, 0, 0), (5, 48, 160, 17, 0),
                (5, 48, 160, 0, 3), (5, 48, 160, 0, 2)]:
        with pytest.raises(ValueError):
            dm.plan(kernel, *bad)


def _params():
    return [(kernel, f) for kernel in dm.KERNELS for f in dm.formats(kernel)]


@pytest.mark.parametrize("kernel,f", _params(), ids=[f"{k}-{f.id}" for k, f in _params()])
def test_cases_are_exact_and_agree_with_the_cpu_route(kernel, f):
    """Every case this format runs: exact by the conditions on its own inputs, and the CPU route of
    the op gives the float64 expectation (the gated kernels: in the exact regimes of the epilogue).
    The CPU route takes no launch shape and the cases of one (n, k) take the first m rows of one x, so
    one run at the largest m covers them all."""
    cases = [c for c in dm.MATRIX[kernel] if f.block != 512 or dm.at_most_slices(kernel, c)]
    assert cases
    narrowed, seen = 0, set()
    for c in sorted(cases, key=lambda c: (c[4], c[5], -c[3])):
        if c[4:6] in seen:
            continue
        seen.add(c[4:6])
        b = dm.Built(kernel, f, c)
        b.prove()
        narrowed += b.hi == 2
        first = b.offs[0] + b.k * np.arange(b.n, dtype=np.int64)  # rows straddle chunks, the layer goes on behind
        assert b.offs[0] > 0 and (first // (b.chunk // 2) != (first + b.k - 1) // (b.chunk // 2)).any()
        assert b.total >= b.offs[-1] + b.n * b.k + 32
        y = b.run("cpu", **F32)
        if b.gated:
            check_exact_regimes(y, *b.wants)
        else:
            assert np.array_equal(y.numpy().astype(np.float64), b.wants[0])
    assert (narrowed > 0) == (f.name == "fp8")  # x in [-2, 2] only where fp8's bound asks for it
