"""What the packed decoder-pass checks of decoder_packed_reference.py rest on, and the ops' CPU
routes through the same harness (the gfx950 kernels go through it in
test_gpu_decoder_packed_reference.py).

On the reference alone:
  the block-scaled weights tell scale blocks apart: at least 60 % of adjacent 32-blocks of every
  projection have different amax binades in the host codec's image (77 to 85 % measured; plain
  random_layer weights give nearly one scale byte for the whole image);
  the noise floor e16 is a bf16 floor, and plain torch on the CPU over the dequantized weights
  (d_cpu) stays within the 20 e16 that test_decoder_reference.py grants torch (0.96 to 1.03 measured);
  check A discriminates: each mistake of `mistakes` applied to the float64 reference lies at least
  5 tol away, tol = 2 max(e16, d_cpu). The nearest is a projection's last 16-row tile lost. The
  one exception is stated as such: with seq = 1 the attention output is v whatever q and k hold, so
  a mistake confined to q, k or the rotary embedding lies exactly 0 away there, which is asserted
  instead; at M = 1 only check B sees q and k.
  Check A cannot see a single wrong output row or scale block; check B does (see the helper module).

Through the CPU routes (PackedParams on CPU tensors; q/k/v is merged on the GPU only, so fuse=True
gives 7 linears for fp8 and MXFP6 and 5 linears + 1 SwiGLU for MXFP4):
  the launch list, check A for fuse=True and fuse=False, and every recorded launch again with
  out_dtype=float32 within the f32 accumulation bound of float64 x W^T. The bf16 results are not
  compared with the rounded f32 results here: the CPU route multiplies in bf16 by design."""
import numpy as np
import pytest

import decoder_packed_reference as dp

ALL = pytest.mark.parametrize("cid", dp.CASES, ids=dp.case_id)
LAYERS = [(s, f) for s in dp.SPECS for f in dp.FORMATS]


@pytest.mark.parametrize("spec_name,fmt_name", LAYERS)
def test_adjacent_scale_blocks_differ(spec_name, fmt_name):
    L = dp.layer(spec_name, fmt_name)
    scales = dp.scale_exponents(L) if L.block == 32 else None  # the image's own scales, one per 32-block
    assert scales is None or scales.size == L.src // 2 // 32
    for p in dp.PROJECTIONS:
        b = dp.amax_binades(L, p)
        frac = float((b[1:] != b[:-1]).mean())
        print(spec_name, fmt_name, p, "adjacent 32-blocks with different amax binades", round(frac, 3))
        assert frac >= 0.6
        if scales is not None:
            e = scales[L.off[p][0] // 32: (L.off[p][0] + L.w[p].size) // 32]
            frac = float((e[1:] != e[:-1]).mean())
            print(spec_name, fmt_name, p, "adjacent scales of the image that differ", round(frac, 3))
            assert e.size == b.size and frac >= 0.6


def test_the_5k_chunk_cuts_rows_and_scale_blocks():
    """What the chunk sizes are chosen for, from layer_params alone. A chunk is a multiple of 512
    elements and every row of `tiny` (256 or 512 elements) starts at a multiple of its own length:
    no chunk size can cut one of its rows. In `uneven` a 5 KiB chunk cuts rows of every projection."""
    for spec_name, cut in [("tiny", False), ("uneven", True)]:
        L = dp.layer(spec_name, "fp8b128-5k")
        ce = L.chunk // 2
        assert ce == 2560
        for p in dp.PROJECTIONS:  # a chunk edge inside a row
            first, (n, k) = L.off[p]
            assert any((e - first) % k for e in range(-(-first // ce) * ce, first + n * k, ce)) == cut, p
        assert L.off["post_attention_layernorm"][0] % ce  # dequantized from mid-chunk
    assert dp.layer("uneven", "fp8b128-5k").off["q_proj"][0] == 192  # 1.5 fp8 blocks of 128 into the image


@ALL
def test_the_noise_floor_and_plain_torch(cid):
    c = dp.case(*cid)
    print(c.id, "e16", c.e16, "d_cpu / e16", c.d_cpu / c.e16, "rows: worst d_cpu / its e16",
          float((c.row_d_cpu / c.row_e16).max()))
    assert 1e-4 < c.e16 < 2e-2
    assert c.d_cpu <= dp.CONTROL_FACTOR * c.e16
    assert c.row_d_cpu.max() <= dp.CONTROL_FACTOR * c.row_e16.max()


@pytest.mark.parametrize("cid,mistake", [(cid, m) for cid in dp.CASES for m in dp.mistakes(cid[0])],
                         ids=lambda v: v if isinstance(v, str) else dp.case_id(v))
def test_check_a_discriminates(cid, mistake):
    c = dp.case(*cid)
    dist = dp.rel(dp.mistaken(c, mistake), c.y64)
    print(c.id, mistake, "distance / e16", dist / c.e16, "tolerances", dist / c.tol())
    if c.seq == 1 and dp.blind_at_one_position(mistake):
        assert dist == 0  # by the layer's definition: see blind_at_one_position
    else:
        assert dist >= 5 * c.tol()


@pytest.fixture(scope="module", params=dp.CASES, ids=dp.case_id)
def passes(request):
    """Per case: the packed parameters on the CPU and both routes' (output, recorded launches)."""
    c = dp.case(*request.param)
    params = c.layer.packed_params()
    packed = params["q_proj"].packed
    return c, packed, {fuse: dp.run_captured(c.xt, params, c.spec, fuse) for fuse in (True, False)}


@pytest.mark.parametrize("fuse", [True, False])
def test_cpu_route_matches_float64(passes, fuse):
    c, _, out = passes
    dp.check_a(c, out[fuse][0], f"cpu fuse={fuse}")


@pytest.mark.parametrize("fuse", [True, False])
def test_cpu_launch_list(passes, fuse):
    c, packed, out = passes
    expected = dp.expected_launches(c, fuse, merged_qkv=False)
    assert len(expected) == (6 if fuse and c.layer.fmt == "mxfp4" else 7)
    dp.check_launch_list(c, out[fuse][1], expected, packed)


@pytest.mark.parametrize("fuse", [True, False])
def test_cpu_launches_in_situ(passes, fuse):
    c, _, out = passes
    for r, e in zip(out[fuse][1], dp.expected_launches(c, fuse, merged_qkv=False)):
        print(c.id, f"fuse={fuse}", e[0], e[1], "worst err / bound", dp.check_launch(c, r, e, rounded_f32=False))


@pytest.mark.parametrize("spec_name,fmt_name", LAYERS)
def test_check_b_sees_one_doubled_scale(spec_name, fmt_name):
    """The harness on a planted fault: the ops are handed an image in which one scale, of a block in
    the middle of one projection (the last block of a row: the K tail where there is one), is twice
    what the reference's image holds. Step 2 must fail for exactly the launches that read that
    projection, for every projection in turn. Check A is asked too, and its answer printed: it is
    not expected to see one scale block."""
    c = dp.case(spec_name, (3, 7), fmt_name)
    L = c.layer
    expected = dp.expected_launches(c, True, merged_qkv=False)
    for p in dp.PROJECTIONS:
        first, (n, k) = L.off[p]
        img = dp.image_with_a_doubled_scale(L, first + (n // 2) * k + k - 32)
        params = dp.unflatten_packed(dp.torch.from_numpy(img), c.spec, L.chunk, L.fmt, L.block)
        y, rec = dp.run_captured(c.xt, params, c.spec, True)
        failed = []
        for r, e in zip(rec, expected):
            try:
                dp.check_launch(c, r, e, rounded_f32=False)
            except AssertionError as err:
                failed.append((e[1], float(str(err).split()[0])))
        print(c.id, p, "launches that failed step 2 (offsets, worst err / bound):", failed,
              "check A distance / tol:", dp.rel(y.float().numpy(), c.y64) / c.tol())
        assert [offs for offs, _ in failed] == [e[1] for e in expected if first in e[1]]
