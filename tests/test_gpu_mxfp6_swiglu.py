"""The gfx950 fused gated MLP from an MXFP6-packed layer (csrc/kernels/mxfp6_swiglu.hip,
ops.mxfp6_swiglu): silu(x Wg^T) * (x Wu^T) with both weights read in place, against the numpy
reference of test_mxfp6_linear_host.py, case for case what test_gpu_mxfp4_swiglu.py asks of the
MXFP4 kernel, and decoder_forward's opt-in route (fuse_gated=True) in a session whose layers stay
packed in HBM. The bodies, and what they bound and why, are in packed_swiglu_gpu.py."""
import pytest
import torch

import packed_swiglu_gpu as ps

pytestmark = pytest.mark.gpu

F = ps.Fmt("mxfp6")


@pytest.mark.parametrize("m,n,k,split_k,row_tiles", ps.EXACT)
def test_exact_on_integer_inputs(gpu, m, n, k, split_k, row_tiles):
    ps.exact_on_integer_inputs(F, m, n, k, split_k, row_tiles)


@pytest.mark.parametrize("m,n,k", ps.LAYOUT_SHAPES)
@pytest.mark.parametrize("layout", list(ps.LAYOUTS))
def test_exact_across_chunk_layouts(gpu, layout, m, n, k):
    ps.exact_across_chunk_layouts(F, layout, m, n, k)


@pytest.fixture(scope="module")
def random_case(gpu):
    return ps.random_case(F)


@pytest.mark.parametrize("split_k", ps.SPLITS)
@pytest.mark.parametrize("m,n,k", ps.RANDOM_SHAPES)
def test_epilogue_on_the_linear_kernels_sums(gpu, random_case, m, n, k, split_k):
    ps.epilogue_on_the_linear_kernels_sums(F, random_case[m, n, k], m, n, k, split_k)


@pytest.mark.parametrize("m,n,k,split_k", [(5, 48, 160, 1), (64, 528, 1056, 4), (1, 528, 128, 16)])
def test_epilogue_with_inf_and_nan_in_x(gpu, random_case, m, n, k, split_k):
    ps.epilogue_on_the_linear_kernels_sums(F, random_case[m, n, k], m, n, k, split_k, specials=True)


@pytest.mark.parametrize("m,n,k", [(5, 48, 160), (64, 528, 1056)])
def test_bf16_output_is_the_rounded_f32_output(gpu, random_case, m, n, k):
    ps.bf16_output_is_the_rounded_f32_output(F, random_case[m, n, k])


def test_deterministic(gpu, random_case):
    ps.deterministic(F, gpu, random_case)


def test_nan_block_poisons_only_its_column(gpu):
    ps.nan_weight_poisons_only_its_column(F)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("split_k", [1, 4])
def test_writes_only_its_output(gpu, dtype, split_k):
    ps.writes_only_its_output(F, dtype, split_k)


def test_rejects_bad_gpu_arguments(gpu):
    ps.rejects_bad_gpu_arguments(F, gpu)


def test_fused_forward_from_the_packed_hbm_slot(gpu):
    ps.fused_forward_from_the_packed_hbm_slot(F)


@pytest.mark.parametrize("case_key", ps.reference_cases(F), ids=ps.dp.case_id)
def test_fuse_gated_pass_matches_float64(gpu, case_key):
    ps.fuse_gated_pass_matches_float64(case_key)
