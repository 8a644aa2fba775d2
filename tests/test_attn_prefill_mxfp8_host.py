"""ops.attn_prefill and ops.rope_append_seq on an MXFP8 KV cache (k_scale=, v_scale=) and
decoder_forward(attn="mfma_mxfp8") without a GPU: the cases test_gpu_attn_prefill_mxfp8.py shares, the
condition on the reference, the CPU routes and the errors.

A case is test_attn_prefill_host.case for d in (64, 128) with scale bytes that differ, made as
test_attn_mxfp8_host.sequence makes them - K's d-block j times 2^(j - 1) and q's times 2^(1 - j), which leaves
every score what it was; V's block j at position t times 2^((3 t + j) % 7 - 3) - and each sequence's valid prefix
[0, start[b] + S) quantized by the host codec. Behind it the codes are NaN codes (0x7F / 0xFF) and the scale
bytes 0xFF; `kd`, `vd` hold the dequantized prefix (exact in bf16) and NaN / inf bf16 patterns behind it. The
float64 reference and the bound are test_attn_prefill_host's, unchanged, on the dequantized values. The
condition, on the reference alone: every marked position still carries a weight of at least 0.1 after
quantization (measured: the smallest 0.2466, the bf16 cases' 0.247).
The rope shapes are test_attn_decode_host.ROPE_SHAPES at the d the format serves (d = 32 is an error case)
and test_attn_mxfp8_host's shape of two workgroups a token."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import ops
from distributed_llm_dissemination_amd.models import weights as W
from distributed_llm_dissemination_amd.models.weights import KVCache, decoder_forward, decoder_step

import test_attn_decode_host as dh
import test_attn_mxfp8_host as mx
import test_attn_prefill_host as ph
from attn_decode_cases import garbage, to_bits

CASES = [c for c in ph.CASES if c[0] in (64, 128)]
ROPE_SHAPES = {**{n: s for n, s in dh.ROPE_SHAPES.items() if s[2] in (64, 128)}, **mx.ROPE_SHAPES}


@functools.lru_cache(maxsize=None)
def case(d, group, s):
    """dict on the CPU: q, start, marks of the bf16 case; codes kc, vc and scale bytes ks, vs [4, KVH, T, d or
    d / 32]; kd, vd bf16 [4, KVH, T, d]; the float64 y64, bound and weights p on kd, vd."""
    c = ph.case(d, group, s)
    shape, j = c["k"].shape, torch.arange(d) // 32
    q = (c["q"].float() * 2.0 ** (1 - j)).to(torch.bfloat16)
    k = (c["k"].float() * 2.0 ** (j - 1)).to(torch.bfloat16)
    v = (c["v"].float() * 2.0 ** ((3 * torch.arange(shape[2])[:, None] + j[None, :]) % 7 - 3)).to(torch.bfloat16)
    rng = np.random.default_rng(s)
    kc, vc = (torch.from_numpy(rng.choice(np.array([0x7F, 0xFF], dtype=np.uint8), size=tuple(shape))) for _ in range(2))
    ks, vs = (torch.full(tuple(shape[:3]) + (d // 32,), 0xFF, dtype=torch.uint8) for _ in range(2))
    kd, vd = garbage(shape, 71), garbage(shape, 72)
    for b, st in enumerate(ph.STARTS):
        for codes, scales, deq, src in ((kc, ks, kd, k), (vc, vs, vd, v)):
            codes[b, :, : st + s], scales[b, :, : st + s] = mx.quantize(src[b, :, : st + s])
            deq[b, :, : st + s] = mx.dequant(codes[b, :, : st + s], scales[b, :, : st + s])
    y64, bound, p = ph.reference(q, kd, vd, ph.STARTS)
    return dict(id=c["id"], q=q, kc=kc, ks=ks, vc=vc, vs=vs, kd=kd, vd=vd, start=c["start"], marks=c["marks"], y64=y64,
                bound=bound, p=p)


def prefill(c, dev="cpu", cut=None, **kw):
    """ops.attn_prefill on the case's codes on `dev`, T cut to `cut` positions."""
    kc, ks, vc, vs = (c[n][:, :, :cut].contiguous().to(dev) for n in ("kc", "ks", "vc", "vs"))
    return ops.attn_prefill(c["q"].to(dev), kc, vc, c["start"].to(dev), k_scale=ks, v_scale=vs, **kw)


@pytest.mark.parametrize("c", CASES, ids=ph.case_id)
def test_marked_positions_carry_weight_and_cpu_route_matches_float64(c):
    cc = case(*c)
    w = min(cc["p"][(b, h)][row, j] for b, row, h, j in cc["marks"])
    print(cc["id"], "smallest marked weight after quantization", w)
    assert w >= 0.1
    for b, st in enumerate(ph.STARTS):  # the scale bytes do differ
        assert all(len(set(t[b, :, : st + c[2]].flatten().tolist())) > 1 for t in (cc["ks"], cc["vs"]))
    y32, y16 = prefill(cc, out_dtype=torch.float32), prefill(cc)
    assert y32.dtype == torch.float32 and y16.dtype == torch.bfloat16 and tuple(y32.shape) == tuple(y16.shape) == cc["y64"].shape
    w32, w16 = ph.err_over_bound(y32, cc, False), ph.err_over_bound(y16, cc, True)
    print(cc["id"], "cpu route err / bound: f32", w32, "bf16", w16)
    assert w32 <= 1 and w16 <= 1
    yc = prefill(cc, cut=ph.BK + 5 + c[2] - 2, out_dtype=torch.float32)  # sequence 3's last two rows have no position
    assert not yc[3, -2:].any() and torch.equal(yc[:3], y32[:3]) and torch.equal(yc[3, :-2], y32[3, :-2])


def check_rope_append_seq(heads, kvh, d, device, merged):
    """rope_append_seq(k_scale=, v_scale=) on `device`: the four tensors' bytes are those of S successive
    rope_append(k_scale=, v_scale=) calls into copies of the same random bytes, q the bf16 route's."""
    cap, s, start = 37, 7, [0, 5, 33, -2]
    b = len(start)
    g = torch.Generator().manual_seed(3)
    y = torch.randn(b, s, (heads + 2 * kvh) * d, generator=g)
    y = (y * 2.0 ** (torch.arange(y.shape[-1]) // 32 % 5 - 2)).to(torch.bfloat16).to(device)  # block scales differ
    q, k, v = y[..., : heads * d], y[..., heads * d: (heads + kvh) * d], y[..., (heads + kvh) * d:]
    if not merged:
        q, k, v = q.clone(), k.clone(), v.clone()
    cos, sin = W._rope_tables(cap, d, 500000.0, device)
    st = torch.tensor(start, dtype=torch.int32, device=device)
    before = [torch.randint(0, 256, (b, kvh, cap, n), generator=g, dtype=torch.uint8).to(device) for n in (d, d // 32, d, d // 32)]
    kc, ks, vc, vs = (t.clone() for t in before)
    q_out = ops.rope_append_seq(q, k, v, cos, sin, kc, vc, st, k_scale=ks, v_scale=vs)
    wk, wks, wv, wvs = before
    for i in range(s):
        ops.rope_append(q[:, i], k[:, i], v[:, i], cos, sin, wk, wv, st + i, k_scale=wks, v_scale=wvs)
    for name, got, want in zip(("k codes", "k scales", "v codes", "v scales"), (kc, ks, vc, vs), before):
        assert torch.equal(got, want), name
    kb, vb = (torch.zeros(b, kvh, cap, d, dtype=torch.bfloat16, device=device) for _ in range(2))
    assert np.array_equal(to_bits(q_out), to_bits(ops.rope_append_seq(q, k, v, cos, sin, kb, vb, st)))
    outside = [(i, t) for i, p in enumerate(start) for t in range(s) if not 0 <= p + t < cap]
    assert len(outside) == 5 and not any(to_bits(q_out[i, t]).any() for i, t in outside)


@pytest.mark.parametrize("merged", [True, False], ids=["merged", "separate"])
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=list(ROPE_SHAPES))
def test_rope_append_seq_cpu_route_writes_the_bytes_of_successive_appends(shape, merged):
    check_rope_append_seq(*ROPE_SHAPES[shape], "cpu", merged)


def check_forward(device):
    """decoder_forward(attn="mfma_mxfp8"): prefill 5, extend 4, one decoder_step, against the emulation of
    test_attn_mxfp8_host.prefill_and_steps(mx=False) on `device`: a bf16 cache, the bf16 ops, every appended row
    through the host codec and back (the GPU quantizers write the host codec's bytes)."""
    c, p, _ = dh.step_params("plain", "tiny", device)
    spec, x, nb, first, more = c.spec, c.xt.to(device), dh.STEP_B, dh.PREFILL, 4
    real = KVCache.allocate(spec, nb, first + more + 3, device, kv_format="mxfp8")
    emu = KVCache.allocate(spec, nb, first + more + 3, device)
    tail = lambda xt, a: W._attn_tail(xt, a, p, spec, True, False, False, None)  # noqa: E731
    qkv = lambda xt: W._qkv(W._rms_norm(xt, W._dense(p["input_layernorm"]), spec.eps), p, True, False, None)  # noqa: E731

    def through_codec(lo, hi):
        for t in (emu.k, emu.v):
            t[:, :, lo:hi] = mx.dequant(*mx.quantize(t[:, :, lo:hi].cpu())).to(device)

    for lo, hi, kw in ((0, first, {}), (first, first + more, dict(extend=True))):
        y = decoder_forward(x[:, lo:hi], p, spec, cache=real, attn="mfma_mxfp8", **kw)
        assert real.lens.tolist() == [hi] * nb and real.max_len == hi
        start = emu.lens if kw else None
        q = ops.rope_append_seq(*qkv(x[:, lo:hi]), emu.cos, emu.sin, emu.k, emu.v, start)
        through_codec(lo, hi)
        assert torch.equal(y, tail(x[:, lo:hi], ops.attn_prefill(q, emu.k, emu.v, start))), (lo, hi)
        emu.lens.fill_(hi)
    n = first + more
    xt = x[:, n - 1: n]  # one more token, the values of the last
    y = decoder_step(xt, p, spec, real)
    q = ops.rope_append(*qkv(xt), emu.cos, emu.sin, emu.k, emu.v, emu.lens)
    through_codec(n, n + 1)
    a = ops.attn_decode(q, emu.k, emu.v, emu.lens + 1, max_len=n + 1)
    assert real.lens.tolist() == [n + 1] * nb and real.max_len == n + 1
    for name in ("k", "v"):
        got = mx.dequant(getattr(real, name)[:, :, : n + 1].cpu(), getattr(real, name + "_scale")[:, :, : n + 1].cpu())
        assert torch.equal(got, getattr(emu, name)[:, :, : n + 1].cpu()), name
    assert torch.equal(y, tail(xt, a.view(nb, 1, -1)))
    plain, ctl = (KVCache.allocate(spec, nb, first + 2, device, kv_format="mxfp8") for _ in range(2))
    decoder_forward(x[:, :first], p, spec, cache=plain, attn="mfma_mxfp8")
    decoder_forward(x[:, :first], p, spec, cache=ctl)  # the default route's bytes
    for name in ("k", "v", "k_scale", "v_scale"):
        assert torch.equal(getattr(plain, name)[:, :, :first], getattr(ctl, name)[:, :, :first]), name


def test_forward_mfma_mxfp8_cpu_is_the_emulation_on_the_dequantized_cache():
    check_forward("cpu")


def error_cases(device):
    """[(name, thunk)]: every call must raise ValueError before any launch."""
    b, kvh, t_len, d, s = 2, 2, 16, 64, 3
    z = lambda *shape, dtype=torch.uint8: torch.zeros(*shape, dtype=dtype, device=device)  # noqa: E731
    kc, ks = z(b, kvh, t_len, d), z(b, kvh, t_len, d // 32)
    bad = {
        "no scales": (kc, d, {}),
        "one scale": (kc, d, dict(k_scale=ks)),
        "scales with bf16 tensors": (kc.to(torch.bfloat16), d, dict(k_scale=ks, v_scale=ks)),
        "scale shape": (kc, d, dict(k_scale=ks, v_scale=ks[..., :1])),
        "scale dtype": (kc, d, dict(k_scale=ks, v_scale=ks.to(torch.int8))),
        "scale layout": (kc, d, dict(k_scale=ks, v_scale=z(b, kvh, d // 32, t_len).transpose(2, 3))),
        "d 32": (kc[..., :32].contiguous(), 32, dict(k_scale=ks[..., :1].contiguous(), v_scale=ks[..., :1].contiguous())),
    }
    out = []
    for name, (c, dd, kw) in bad.items():
        q, rk = z(b, s, 4, dd, dtype=torch.bfloat16), z(b, s, kvh * dd, dtype=torch.bfloat16)
        tables = W._rope_tables(t_len, dd, 1e4, device)
        out.append(("attn: " + name, lambda q=q, c=c, kw=kw: ops.attn_prefill(q, c, c.clone(), **kw)))
        out.append(("rope: " + name, lambda q=q, rk=rk, c=c, kw=kw, tables=tables: ops.rope_append_seq(
            q.view(b, s, -1), rk, rk, *tables, c, c.clone(), **kw)))
    spec = W.PRESETS["tiny"]
    wt = {n: w.to(device) for n, w in W.random_layer(spec, 1).items()}
    x = z(b, s, spec.hidden, dtype=torch.bfloat16)
    cache = lambda fmt, max_len=0: KVCache(**{**vars(KVCache.allocate(spec, b, 8, device, kv_format=fmt)), "max_len": max_len})  # noqa: E731
    return out + [
        ("forward: no cache", lambda: decoder_forward(x, wt, spec, attn="mfma_mxfp8")),
        ("forward: a bf16 cache", lambda: decoder_forward(x, wt, spec, attn="mfma_mxfp8", cache=cache("bf16"))),
        ("forward: extend past the capacity", lambda: decoder_forward(x, wt, spec, attn="mfma_mxfp8", cache=cache("mxfp8", 6), extend=True)),
        ("forward: mfma with an MXFP8 cache", lambda: decoder_forward(x, wt, spec, attn="mfma", cache=cache("mxfp8"))),
    ]


def check_errors(device):
    for name, thunk in error_cases(device):
        with pytest.raises(ValueError):
            thunk()
            pytest.fail(f"{name}: no ValueError")


def test_errors_cpu():
    check_errors("cpu")


def test_selftest_under_asan_and_ubsan():
    """csrc/tests/attn_prefill_mxfp8_selftest.cc, a stand-alone program without a GPU: the two grids' index
    arithmetic over exact-size buffers."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-C", root, "sanitize-attn-prefill-mxfp8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "attn_prefill_mxfp8_selftest ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
