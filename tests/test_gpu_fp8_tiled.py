"""The many-row fp8 kernels (csrc/kernels/fp8_tiled.hip; ops.fp8_linear and ops.fp8_swiglu with
tiled=True), at scale blocks 32 and 128 and, on three shapes, 512. The bodies, and what they prove,
are in packed_tiled_gpu.py."""
import pytest
import torch

from distributed_llm_dissemination_amd import _core

import packed_tiled_gpu as t
import test_gpu_fp8_linear as lin
from packed_swiglu_gpu import Fmt

pytestmark = pytest.mark.gpu

FMTS = [Fmt("fp8", 32), Fmt("fp8", 128)]
IDS = [f.id for f in FMTS]
BM, BN = _core.fp8_tiled_tile()
EXACT = t.exact_list(BM, BN)
EXACT_512 = [(BM + 1, 528, 1056), (17, 48, 160), (2 * BM + 5, BN + 16, 96)]
RANDOM = t.random_shapes(BM)


@pytest.mark.parametrize("m,n,k", EXACT)
@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_exact_on_integer_inputs(gpu, f, m, n, k):
    """The parameter at element 96: off the scale-block grid for a block above 32."""
    t.exact_on_integer_inputs(f, m, n, k, off=96)


@pytest.mark.parametrize("m,n,k", EXACT_512)
def test_exact_on_integer_inputs_block_512(gpu, m, n, k):
    t.exact_on_integer_inputs(Fmt("fp8", 512), m, n, k, off=96)


@pytest.mark.parametrize("m,n,k", [(BM + 1, 48, 96), (17, 528, 160)])
@pytest.mark.parametrize("layout", list(lin.LAYOUTS))
def test_exact_across_chunk_layouts(gpu, layout, m, n, k):
    chunk, block, off, behind = lin.LAYOUTS[layout]
    t.exact_across_chunk_layouts(Fmt("fp8", block), chunk, off, behind, m, n, k, image_is_all=behind == 0)


@pytest.fixture(scope="module")
def random_case(gpu):
    return {f.id: t.random_case(f) for f in FMTS}


@pytest.mark.parametrize("m,n,k", RANDOM[:2])
@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_random_within_f32_accumulation_error(gpu, random_case, f, m, n, k):
    t.random_within_f32_accumulation_error(f, random_case[f.id][m, n, k])


@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_one_row_alone_gives_the_bits_of_the_full_call(gpu, random_case, f):
    t.one_row_alone_gives_the_bits_of_the_full_call(f, random_case[f.id])


@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_a_window_of_weight_rows_gives_its_columns(gpu, random_case, f):
    t.a_window_of_weight_rows_gives_its_columns(f, random_case[f.id])


@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_merged_qkv_equals_three_calls(gpu, random_case, f):
    t.merged_qkv_equals_three_calls(f, random_case[f.id])


@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_deterministic(gpu, random_case, f):
    t.deterministic(f, random_case[f.id])


@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_agrees_with_the_decode_kernel(gpu, random_case, f):
    t.agrees_with_the_decode_kernel(f, random_case[f.id])


@pytest.mark.parametrize("m,n,k,layout", t.gated_list(BM, BN))
@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_gated_exact_on_integer_inputs(gpu, f, m, n, k, layout):
    t.gated_exact_on_integer_inputs(f, m, n, k, layout)


@pytest.mark.parametrize("m,n,k", RANDOM[:2])
@pytest.mark.parametrize("up_first", [False, True])
@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_gated_epilogue_on_the_tiled_linears_sums(gpu, random_case, f, m, n, k, up_first):
    t.gated_epilogue_on_the_tiled_linears_sums(f, random_case[f.id][m, n, k], m, n, k, up_first)


@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_nan_code_poisons_only_its_column(gpu, f):
    t.nan_weight_poisons_only_its_column(f)


@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_non_finite_rows_of_x_as_the_untiled_op(gpu, f):
    t.non_finite_rows_of_x_as_the_untiled_op(f)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_writes_only_its_output(gpu, f, dtype, gated):
    t.writes_only_its_output(f, dtype, gated)


@pytest.mark.parametrize("f", FMTS, ids=IDS)
def test_rejects_bad_gpu_arguments(gpu, f):
    t.rejects_bad_gpu_arguments(f)


@pytest.mark.parametrize("fmt_name", ["fp8b32-5k", "fp8b128-5k", "fp8b512-4k"])
@pytest.mark.parametrize("spec_name", ["tiny", "uneven"])
def test_decoder_forward_tiled(gpu, monkeypatch, spec_name, fmt_name):
    t.decoder_forward_tiled(monkeypatch, spec_name, fmt_name)
