"""The gfx950 fused gated MLP from an fp8-packed layer (csrc/kernels/fp8_swiglu.hip,
ops.fp8_swiglu): silu(x Wg^T) * (x Wu^T) with both weights read in place, against the numpy
reference of test_fp8_linear_host.py, case for case what test_gpu_mxfp4_swiglu.py asks of the MXFP4
kernel - with scale blocks of 32 and 128 everywhere and of 512 on three shapes - and
decoder_forward's opt-in route (fuse_gated=True) in a session whose layers stay packed in HBM. The
bodies, and what they bound and why, are in packed_swiglu_gpu.py."""
import pytest
import torch

import packed_swiglu_gpu as ps

pytestmark = pytest.mark.gpu

FMTS = {b: ps.Fmt("fp8", b) for b in (32, 128, 512)}
BLOCKS = [32, 128]


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("m,n,k,split_k,row_tiles", ps.EXACT)
def test_exact_on_integer_inputs(gpu, m, n, k, split_k, row_tiles, block):
    ps.exact_on_integer_inputs(FMTS[block], m, n, k, split_k, row_tiles)


@pytest.mark.parametrize("m,n,k,split_k,row_tiles", ps.EXACT_512)
def test_exact_on_integer_inputs_with_block_512(gpu, m, n, k, split_k, row_tiles):
    ps.exact_on_integer_inputs(FMTS[512], m, n, k, split_k, row_tiles)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("m,n,k", ps.LAYOUT_SHAPES)
@pytest.mark.parametrize("layout", list(ps.LAYOUTS))
def test_exact_across_chunk_layouts(gpu, layout, m, n, k, block):
    ps.exact_across_chunk_layouts(FMTS[block], layout, m, n, k)


@pytest.fixture(scope="module")
def random_case(gpu):
    return {b: ps.random_case(FMTS[b]) for b in BLOCKS}


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("split_k", ps.SPLITS)
@pytest.mark.parametrize("m,n,k", ps.RANDOM_SHAPES)
def test_epilogue_on_the_linear_kernels_sums(gpu, random_case, m, n, k, split_k, block):
    ps.epilogue_on_the_linear_kernels_sums(FMTS[block], random_case[block][m, n, k], m, n, k, split_k)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("m,n,k,split_k", [(5, 48, 160, 1), (64, 528, 1056, 4), (1, 528, 128, 16)])
def test_epilogue_with_inf_and_nan_in_x(gpu, random_case, m, n, k, split_k, block):
    ps.epilogue_on_the_linear_kernels_sums(FMTS[block], random_case[block][m, n, k], m, n, k, split_k, specials=True)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("m,n,k", [(5, 48, 160), (64, 528, 1056)])
def test_bf16_output_is_the_rounded_f32_output(gpu, random_case, m, n, k, block):
    ps.bf16_output_is_the_rounded_f32_output(FMTS[block], random_case[block][m, n, k])


@pytest.mark.parametrize("block", BLOCKS)
def test_deterministic(gpu, random_case, block):
    ps.deterministic(FMTS[block], gpu, random_case[block])


@pytest.mark.parametrize("block", BLOCKS)
def test_nan_code_poisons_only_its_column(gpu, block):
    ps.nan_weight_poisons_only_its_column(FMTS[block])


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("split_k", [1, 4])
def test_writes_only_its_output(gpu, dtype, split_k, block):
    ps.writes_only_its_output(FMTS[block], dtype, split_k)


@pytest.mark.parametrize("block", BLOCKS)
def test_rejects_bad_gpu_arguments(gpu, block):
    ps.rejects_bad_gpu_arguments(FMTS[block], gpu)


def test_rejects_a_bad_block_in_the_launcher(gpu):
    f = FMTS[128]
    n, k, chunk = 48, 96, 1024
    total = 2 * n * k
    p = torch.from_numpy(f.image(total, chunk, 1)).cuda()
    x = torch.zeros(5, k, dtype=torch.bfloat16, device="cuda")
    y = torch.empty(5, n, dtype=torch.float32, device="cuda")
    for block in (48, 16, 512):  # no block size; chunk_bytes is no multiple of 8 * 512
        with pytest.raises(RuntimeError):
            gpu.fp8_swiglu(p.data_ptr(), 2 * total, chunk, block, 0, n * k, x.data_ptr(), 5, n, k, y.data_ptr(), n,
                           False, 0, 0, 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("block", BLOCKS)
def test_fused_forward_from_the_packed_hbm_slot(gpu, block):
    ps.fused_forward_from_the_packed_hbm_slot(FMTS[block])


@pytest.mark.parametrize("case_key", [c for b in FMTS for c in ps.reference_cases(FMTS[b])], ids=ps.dp.case_id)
def test_fuse_gated_pass_matches_float64(gpu, case_key):
    ps.fuse_gated_pass_matches_float64(case_key)
