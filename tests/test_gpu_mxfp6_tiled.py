"""The many-row MXFP6 kernels (csrc/kernels/mxfp6_tiled.hip; ops.mxfp6_linear and ops.mxfp6_swiglu
with tiled=True). The bodies, and what they prove, are in packed_tiled_gpu.py."""
import pytest
import torch

from distributed_llm_dissemination_amd import _core

import packed_tiled_gpu as t
import test_gpu_mxfp6_linear as lin
from packed_swiglu_gpu import Fmt

pytestmark = pytest.mark.gpu

F = Fmt("mxfp6")
BM, BN = _core.mxfp6_tiled_tile()
EXACT = t.exact_list(BM, BN)
RANDOM = t.random_shapes(BM)


@pytest.mark.parametrize("i", range(len(EXACT)), ids=[f"{m}-{n}-{k}" for m, n, k in EXACT])
def test_exact_on_integer_inputs(gpu, i):
    """The parameter at block 3 and at block 4 of the layer, in turn: 8-B- and 16-B-aligned codes,
    alternating row by row where K / 32 is odd."""
    t.exact_on_integer_inputs(F, *EXACT[i], off=32 * (3 + i % 2))


@pytest.mark.parametrize("m,n,k", [(BM + 1, 48, 96), (17, 528, 160)])
@pytest.mark.parametrize("layout", list(lin.LAYOUTS))
def test_exact_across_chunk_layouts(gpu, layout, m, n, k):
    chunk, off, behind = lin.LAYOUTS[layout]
    t.exact_across_chunk_layouts(F, chunk, off, behind, m, n, k, image_is_all="tail chunk" in layout)


@pytest.fixture(scope="module")
def random_case(gpu):
    return t.random_case(F)


@pytest.mark.parametrize("m,n,k", RANDOM[:2])
def test_random_within_f32_accumulation_error(gpu, random_case, m, n, k):
    t.random_within_f32_accumulation_error(F, random_case[m, n, k])


def test_one_row_alone_gives_the_bits_of_the_full_call(gpu, random_case):
    t.one_row_alone_gives_the_bits_of_the_full_call(F, random_case)


def test_a_window_of_weight_rows_gives_its_columns(gpu, random_case):
    t.a_window_of_weight_rows_gives_its_columns(F, random_case)


def test_merged_qkv_equals_three_calls(gpu, random_case):
    t.merged_qkv_equals_three_calls(F, random_case)


def test_deterministic(gpu, random_case):
    t.deterministic(F, random_case)


def test_agrees_with_the_decode_kernel(gpu, random_case):
    t.agrees_with_the_decode_kernel(F, random_case)


@pytest.mark.parametrize("m,n,k,layout", t.gated_list(BM, BN))
def test_gated_exact_on_integer_inputs(gpu, m, n, k, layout):
    t.gated_exact_on_integer_inputs(F, m, n, k, layout)


@pytest.mark.parametrize("m,n,k", RANDOM[:2])
@pytest.mark.parametrize("up_first", [False, True])
def test_gated_epilogue_on_the_tiled_linears_sums(gpu, random_case, m, n, k, up_first):
    t.gated_epilogue_on_the_tiled_linears_sums(F, random_case[m, n, k], m, n, k, up_first)


def test_nan_block_poisons_only_its_column(gpu):
    t.nan_weight_poisons_only_its_column(F)


def test_non_finite_rows_of_x_as_the_untiled_op(gpu):
    t.non_finite_rows_of_x_as_the_untiled_op(F)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gated", [False, True])
def test_writes_only_its_output(gpu, dtype, gated):
    t.writes_only_its_output(F, dtype, gated)


def test_rejects_bad_gpu_arguments(gpu):
    t.rejects_bad_gpu_arguments(F)


@pytest.mark.parametrize("spec_name", ["tiny", "uneven"])
def test_decoder_forward_tiled(gpu, monkeypatch, spec_name):
    t.decoder_forward_tiled(monkeypatch, spec_name, "mxfp6-5k")
