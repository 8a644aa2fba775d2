"""The many-row MXFP4 kernels (csrc/kernels/mxfp4_tiled.hip) as seen without a GPU: the bindings
exist, `tiled=True` leaves the ops' CPU routes and decoder_forward on the CPU bit for bit as they
are, it excludes `split_k` and `row_tiles`, and the launchers refuse bad arguments before they
touch a device, with the error of the untiled pair. The kernels themselves are tested in
test_gpu_mxfp4_tiled.py."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models.weights import PRESETS, decoder_forward, flatten, random_layer, unflatten_packed

from test_mxfp4_linear_host import bf16_tensor_bits, handmade_image, int_x

KiB = 1 << 10


def test_core_has_the_tiled_launchers():
    assert callable(_core.mxfp4_linear_tiled) and callable(_core.mxfp4_swiglu_tiled)
    bm, bn = _core.mxfp4_tiled_tile()
    assert bm >= 128 and bm % 16 == 0 and bn >= 16 and bn % 16 == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tiled_changes_nothing_on_the_cpu(dtype):
    m, n, k, chunk, gate = 17, 48, 160, 1024, 32 * 7
    up = gate + n * k + 64
    total = up + n * k
    p = torch.from_numpy(handmade_image(total, chunk, 5))
    x, _ = int_x(m, k, 6)
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk, out_dtype=dtype)
    a = ops.mxfp4_linear(x, p, n, k, elem_offset=up, **kw)
    b = ops.mxfp4_linear(x, p, n, k, elem_offset=up, tiled=True, **kw)
    assert b.dtype == dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    a = ops.mxfp4_swiglu(x, p, n, k, gate_offset=gate, up_offset=up, **kw)
    b = ops.mxfp4_swiglu(x, p, n, k, gate_offset=gate, up_offset=up, tiled=True, **kw)
    assert b.dtype == dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_tiled_excludes_split_k_and_row_tiles():
    n, k, chunk = 64, 96, 1024  # 4 tiles: row_tiles=2 is valid for the untiled kernels
    total = 2 * n * k
    p = torch.from_numpy(handmade_image(total, chunk, 1))
    x = torch.zeros(5, k, dtype=torch.bfloat16)
    kw = dict(src_bytes=2 * total, chunk_bytes=chunk)
    for arg in ("split_k", "row_tiles"):
        with pytest.raises(ValueError, match=arg):
            ops.mxfp4_linear(x, p, n, k, tiled=True, **{arg: 2}, **kw)
        with pytest.raises(ValueError, match=arg):
            ops.mxfp4_swiglu(x, p, n, k, gate_offset=0, up_offset=n * k, tiled=True, **{arg: 2}, **kw)
        ops.mxfp4_linear(x, p, n, k, tiled=False, **{arg: 2}, **kw)  # as before
        ops.mxfp4_swiglu(x, p, n, k, gate_offset=0, up_offset=n * k, tiled=False, **{arg: 2}, **kw)


@pytest.mark.parametrize("fuse", [True, False])
def test_decoder_forward_tiled_on_the_cpu(fuse):
    spec = PRESETS["tiny"]
    blob = flatten(random_layer(spec, 3), spec)
    packed = _core.mxfp4_pack_layer_host(blob.numpy().tobytes(), 64 * KiB)
    p = unflatten_packed(torch.frombuffer(bytearray(packed), dtype=torch.uint8), spec, 64 * KiB)
    x = torch.randn(2, 9, spec.hidden, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    a = decoder_forward(x, p, spec, fuse=fuse)
    b = decoder_forward(x, p, spec, fuse=fuse, tiled=True)
    assert np.array_equal(bf16_tensor_bits(a), bf16_tensor_bits(b))


def _raises(fn, *a):
    with pytest.raises(RuntimeError) as e:
        fn(*a)
    return str(e.value).split(": ", 1)[1]


def test_launchers_refuse_bad_arguments_like_the_untiled_pair():
    """Every check precedes the launch, so no device is needed: the error text after the
    launcher's name is the untiled launcher's for the same arguments."""
    n, k, chunk = 48, 96, 1024
    total = 2 * n * k
    src = 2 * total
    p = torch.from_numpy(handmade_image(total, chunk, 1))
    buf = torch.zeros(p.numel() + 16, dtype=torch.uint8)
    a16 = buf.data_ptr() + (-buf.data_ptr()) % 16
    x = torch.zeros(5, k, dtype=torch.bfloat16)
    y = torch.zeros(5, n, dtype=torch.float32)
    assert p.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    # (packed, src_bytes, src_chunk, offset, n, k, ldy)
    good = (p.data_ptr(), src, chunk, 0, n, k, n)
    bad = {
        "K not a multiple of 32": (p.data_ptr(), src, chunk, 0, n, 80, n),
        "N not a multiple of 16": (p.data_ptr(), src, chunk, 0, 40, k, 40),
        "ldy < N": (p.data_ptr(), src, chunk, 0, n, k, n - 1),
        "parameter past the layer": (p.data_ptr(), src, chunk, n * k + 32, n, k, n),
        "offset off the block grid": (p.data_ptr(), src, chunk, 16, n, k, n),
        "misaligned packed": (a16 + 4, src, chunk, 0, n, k, n),
        "chunk not a multiple of 1024": (p.data_ptr(), src, 1536, 0, n, k, n),
        "no rows": None,
    }
    for what, args in bad.items():
        m = 5
        if args is None:
            args, m = good, 0
        pk, sb, ck, off, nn, kk, ld = args
        lin = (pk, sb, ck, off, x.data_ptr(), m, nn, kk, y.data_ptr(), ld, False)
        want = _raises(_core.mxfp4_linear, *lin, 0, 0, 0)
        assert _raises(_core.mxfp4_linear_tiled, *lin, 0) == want, what
        for gate, up in ((off, 0), (0, off)):
            glu = (pk, sb, ck, gate, up, x.data_ptr(), m, nn, kk, y.data_ptr(), ld, False)
            want = _raises(_core.mxfp4_swiglu, *glu, 0, 0, 0)
            assert _raises(_core.mxfp4_swiglu_tiled, *glu, 0) == want, what
