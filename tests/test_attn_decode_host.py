"""The decode step against a KV cache without a GPU: what rests on the float64 reference of
attn_decode_cases.py alone, the CPU routes of ops.rope_append and ops.attn_decode, decoder_step on the
CPU, and decoder_forward without a cache.

On the reference alone (so that the GPU test's bound means something): every boundary position has a
softmax weight of at least 0.1 in its head; a lost first, last or chunk-edge position and rotated
heads lie at least 10 bounds away in every case they apply to, an omitted 1 / sqrt(d) at least 5 from
len >= C - 1. Measured: weights from 0.158; drop_first 58 .. 8e4, drop_last 61 .. 5e4,
drop_chunk_edge 51 .. 219, head_swap from 300, no_scale 5.6 .. 539 bounds.

The CPU routes: ops.attn_decode within the same bound of float64 in f32 and bf16 (measured: at most
2e-4 bounds in f32 - the route is f32 throughout - and 0.40 in bf16), garbage behind the lengths never read;
ops.rope_append bit for bit `_rope` and nothing else of the caches touched.

decoder_step: prefill of 5 positions through decoder_forward(..., cache=), then 4 steps, B = 3, over
plain tensors and the packed CPU routes; every step's row within check A's tolerance
(decoder_packed_reference.py) of row t of ref_decoder in float64 over all 9 tokens. For act="mxfp8"
the control decoder_forward(..., act="mxfp8") joins the tolerance as d_ctl does on the GPU: that
route computes the layer of the quantized activations."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_llm_dissemination_amd import ops
from distributed_llm_dissemination_amd.models import weights as W
from distributed_llm_dissemination_amd.models.weights import KVCache, decoder_forward, decoder_step, random_layer

import attn_decode_cases as ac
import decoder_packed_reference as dp
from test_decoder_reference import BATCH, SEQ, SPECS

C = ac.C
STEP_ROUTES = {  # name: (format of decoder_packed_reference.FORMATS, packed, kwargs)
    "plain": ("mxfp4-5k", False, {}),
    "mxfp4": ("mxfp4-5k", True, {}),
    "mxfp4-act": ("mxfp4-5k", True, {"act": "mxfp8"}),
    "mxfp6-gated": ("mxfp6-5k", True, {"fuse_gated": True}),
    "fp8-gated": ("fp8b128-5k", True, {"fuse_gated": True}),
}
STEP_B, PREFILL, STEPS = 3, 5, 4


# ---------------------------------------------------------------- the reference alone

@pytest.mark.parametrize("c", ac.CASES, ids=ac.case_id)
def test_boundary_positions_carry_weight(c):
    for s in ac.sequences(*c):
        for (kv, pos), h in s.spike_head.items():
            assert s.p[h, pos] >= 0.1, (s.n, kv, pos, h, s.p[h, pos])
        if s.n > C:
            assert {0, C - 1, C, s.n - 1} <= {pos for _, pos in s.spike_head}


@pytest.mark.parametrize("mistake", ac.MISTAKES)
@pytest.mark.parametrize("c", ac.CASES, ids=ac.case_id)
def test_the_inputs_discriminate(c, mistake):
    need = 5 if mistake == "no_scale" else 10
    seen = 0
    for s in ac.sequences(*c):
        if ac.applies(mistake, s):
            r = float((np.abs(ac.mistaken(s, mistake) - s.y64) / s.bound).max())
            print(ac.case_id(c), "len", s.n, mistake, "bounds away", r)
            assert r >= need
            seen += 1
    assert seen or (mistake == "head_swap" and c[1] == 1)


def test_lengths_meet_every_chunk_edge():
    assert set(ac.LENGTHS) == {0, 1, 2, C - 1, C, C + 1, 2 * C + 3} and ac.CAPACITY % C and ac.CAPACITY >= 2 * C + 3


# ---------------------------------------------------------------- the ops' CPU routes

@pytest.mark.parametrize("c", ac.CASES, ids=ac.case_id)
def test_attn_decode_cpu_route_matches_float64(c):
    seqs = ac.sequences(*c)
    q, kc, vc, lens = ac.caches(seqs)
    y32 = ops.attn_decode(q, kc, vc, lens, out_dtype=torch.float32)
    y16 = ops.attn_decode(q, kc, vc, lens, max_len=2 * C + 3)
    assert y32.dtype == torch.float32 and y16.dtype == torch.bfloat16
    assert tuple(y32.shape) == tuple(y16.shape) == (len(seqs), seqs[0].heads * c[0])
    w32, w16 = ac.err_over_bound(y32, seqs, False), ac.err_over_bound(y16, seqs, True)
    print(ac.case_id(c), "cpu route err / bound: f32", w32, "bf16", w16)
    assert w32 <= 1 and w16 <= 1
    # alone, every sequence gives the same values (the CPU route is per sequence)
    for b, s in enumerate(seqs):
        qa, ka, va, la = ac.caches([s], capacity=max(s.n, 1) + 3, seed=5)
        assert torch.equal(ops.attn_decode(qa, ka, va, la, out_dtype=torch.float32)[0], y32[b])


def rope_inputs(heads, kvh, d, b, seed, merged):
    g = torch.Generator().manual_seed(seed)
    n = (heads + 2 * kvh) * d
    y = torch.randn(b, 1, n, generator=g).to(torch.bfloat16)
    q, k, v = y[..., : heads * d], y[..., heads * d: (heads + kvh) * d], y[..., (heads + kvh) * d:]
    return (q, k, v) if merged else (q.clone(), k.clone(), v.clone())


def rope_expected(x, nh, d, pos, theta):
    """`_rope` at each row's position: the row placed at index pos of a sequence of pos + 1."""
    out = []
    for i, p in enumerate(pos):
        seq = torch.zeros(1, nh, p + 1, d, dtype=torch.bfloat16, device=x.device)
        seq[0, :, p] = x[i].reshape(nh, d)
        out.append(W._rope(seq, theta)[0, :, p])
    return torch.stack(out)


def check_rope_append(spec_heads, kvh, d, device, merged, theta=500000.0):
    """rope_append on `device` against `_rope` on that device, bit for bit, and every other byte of
    the caches unchanged; positions 0, 1, capacity - 1, in between, and one outside the cache."""
    cap = 37
    pos = [0, 1, cap - 1, 17, 5, cap]
    b = len(pos)
    q, k, v = (t.to(device) for t in rope_inputs(spec_heads, kvh, d, b, 3, merged))
    if merged:  # .to() of a view makes it contiguous: slice the moved buffer instead
        y = torch.cat([q, k, v], -1)
        q, k, v = y[..., : spec_heads * d], y[..., spec_heads * d: (spec_heads + kvh) * d], y[..., (spec_heads + kvh) * d:]
        assert q.stride(0) == (spec_heads + 2 * kvh) * d
    cos, sin = W._rope_tables(cap, d, theta, device)
    fill = torch.Generator().manual_seed(9)
    k0 = torch.randn(b, kvh, cap, d, generator=fill).to(torch.bfloat16).to(device)
    v0 = torch.randn(b, kvh, cap, d, generator=fill).to(torch.bfloat16).to(device)
    kc, vc = k0.clone(), v0.clone()
    q_out = ops.rope_append(q, k, v, cos, sin, kc, vc, torch.tensor(pos, dtype=torch.int32, device=device))
    assert q_out.dtype == torch.bfloat16 and tuple(q_out.shape) == (b, spec_heads, d)
    ok = [i for i, p in enumerate(pos) if p < cap]
    want_q = rope_expected(q[ok], spec_heads, d, [pos[i] for i in ok], theta)
    want_k = rope_expected(k[ok], kvh, d, [pos[i] for i in ok], theta)
    assert np.array_equal(ac.to_bits(q_out[ok]), ac.to_bits(want_q))
    assert not ac.to_bits(q_out[b - 1]).any()  # outside the cache: a zero row
    ek, ev = k0.clone(), v0.clone()
    for j, i in enumerate(ok):
        ek[i, :, pos[i]] = want_k[j]
        ev[i, :, pos[i]] = v[i].reshape(kvh, d)
    assert np.array_equal(ac.to_bits(kc), ac.to_bits(ek))
    assert np.array_equal(ac.to_bits(vc), ac.to_bits(ev))


ROPE_SHAPES = {"tiny": (4, 2, 64), "uneven": (6, 3, 32), "d128": (8, 2, 128)}


@pytest.mark.parametrize("merged", [True, False], ids=["merged", "separate"])
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=list(ROPE_SHAPES))
def test_rope_append_cpu_route_is_rope_bit_for_bit(shape, merged):
    check_rope_append(*ROPE_SHAPES[shape], "cpu", merged)


# ---------------------------------------------------------------- decoder_step

def step_params(route, spec_name, device="cpu"):
    fmt, packed, kw = STEP_ROUTES[route]
    c = dp.case(spec_name, (STEP_B, PREFILL + STEPS), fmt)
    p = c.layer.packed_params(device) if packed else {k: v.to(device) for k, v in c.layer.dense.items()}
    return c, p, kw


def run_steps(c, p, kw, device="cpu", advance=True):
    """Prefill and steps: ([batch, 1, hidden] per step, the cache)."""
    x = c.xt.to(device)
    cache = KVCache.allocate(c.spec, STEP_B, PREFILL + STEPS + 2, device)
    y0 = decoder_forward(x[:, :PREFILL], p, c.spec, cache=cache, **kw)
    assert cache.max_len == PREFILL and cache.lens.tolist() == [PREFILL] * STEP_B
    assert torch.equal(y0, decoder_forward(x[:, :PREFILL], p, c.spec, **kw))
    out = []
    for t in range(PREFILL, PREFILL + STEPS):
        out.append(decoder_step(x[:, t: t + 1], p, c.spec, cache, advance=advance, **kw))
        if not advance:
            assert cache.max_len == t and cache.lens.tolist() == [t] * STEP_B
            cache.lens.add_(1)
            cache.max_len += 1
    return out, cache


def check_steps(c, ys, what, row_d_ctl=0.0):
    """Every step's rows against row t of the float64 reference, per token row, within check A's
    tolerance 2 max(e16, d_cpu or d_ctl)."""
    row_tol = 2 * max(c.row_e16.max(), np.max(row_d_ctl)) if np.max(row_d_ctl) > 0 else c.row_tol()
    worst = 0.0
    for i, y in enumerate(ys):
        t = PREFILL + i
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (STEP_B, 1, c.spec.hidden)
        rows = dp.row_rel(y.float().cpu().numpy()[:, 0], c.y64[:, t])
        worst = max(worst, float(rows.max()))
        assert (rows <= row_tol).all(), (what, t, rows, row_tol)
    print(c.id, what, "worst step row dist / worst row e16", worst / c.row_e16.max(), "tolerance / worst row e16",
          row_tol / c.row_e16.max())
    return worst


@pytest.mark.parametrize("route", STEP_ROUTES, ids=list(STEP_ROUTES))
@pytest.mark.parametrize("spec_name", SPECS, ids=list(SPECS))
@dp.one_thread
def test_decoder_step_cpu_matches_float64(spec_name, route):
    c, p, kw = step_params(route, spec_name)
    ys, cache = run_steps(c, p, kw)
    assert cache.lens.tolist() == [PREFILL + STEPS] * STEP_B and cache.max_len == PREFILL + STEPS
    row_d_ctl = 0.0
    if "act" in kw:
        row_d_ctl = dp.row_rel(decoder_forward(c.xt, p, c.spec, **kw).float().numpy(), c.y64)
    check_steps(c, ys, f"cpu {route}", row_d_ctl)
    ys2, cache2 = run_steps(c, p, kw, advance=False)
    assert all(torch.equal(a, b) for a, b in zip(ys, ys2))
    assert torch.equal(cache.k[:, :, : PREFILL + STEPS], cache2.k[:, :, : PREFILL + STEPS])


@pytest.mark.parametrize("spec_name", SPECS, ids=list(SPECS))
def test_prefill_rows_are_the_forward_pass_own_k_and_v(spec_name):
    check_prefill_rows("plain", spec_name, "cpu")


def check_prefill_rows(route, spec_name, device):
    c, p, kw = step_params(route, spec_name, device)
    spec, x = c.spec, c.xt.to(device)[:, :PREFILL]
    cache = KVCache.allocate(spec, STEP_B, PREFILL + 3, device)
    k0, v0 = cache.k.fill_(7.0).clone(), cache.v.fill_(-7.0).clone()
    decoder_forward(x, p, spec, cache=cache, **kw)
    h = W._rms_norm(x, W._dense(p["input_layernorm"]), spec.eps)
    _, k, v = W._qkv(h, p, True, False, kw.get("act"))
    k = W._rope(k.view(STEP_B, PREFILL, spec.kv_heads, spec.head_dim).transpose(1, 2), spec.rope_theta)
    v = v.view(STEP_B, PREFILL, spec.kv_heads, spec.head_dim).transpose(1, 2)
    assert np.array_equal(ac.to_bits(cache.k[:, :, :PREFILL]), ac.to_bits(k))
    assert np.array_equal(ac.to_bits(cache.v[:, :, :PREFILL]), ac.to_bits(v))
    assert torch.equal(cache.k[:, :, PREFILL:], k0[:, :, PREFILL:]) and torch.equal(cache.v[:, :, PREFILL:], v0[:, :, PREFILL:])


def forward_as_it_was(x, p, spec):
    """decoder_forward over plain tensors as it stood before it took a cache."""
    b, s, _ = x.shape
    hd, nh, nkv = spec.head_dim, spec.heads, spec.kv_heads
    h = W._rms_norm(x, p["input_layernorm"], spec.eps)
    q, k, v = F.linear(h, p["q_proj"]), F.linear(h, p["k_proj"]), F.linear(h, p["v_proj"])
    q = q.view(b, s, nh, hd).transpose(1, 2)
    k = k.view(b, s, nkv, hd).transpose(1, 2)
    v = v.view(b, s, nkv, hd).transpose(1, 2)
    q, k = W._rope(q, spec.rope_theta), W._rope(k, spec.rope_theta)
    k = k.repeat_interleave(nh // nkv, dim=1)
    v = v.repeat_interleave(nh // nkv, dim=1)
    a = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    x = x + F.linear(a.transpose(1, 2).reshape(b, s, nh * hd), p["o_proj"])
    h = W._rms_norm(x, p["post_attention_layernorm"], spec.eps)
    return x + F.linear(F.silu(F.linear(h, p["gate_proj"])) * F.linear(h, p["up_proj"]), p["down_proj"])


@pytest.mark.parametrize("spec_name", SPECS, ids=list(SPECS))
@dp.one_thread
def test_forward_without_a_cache_is_what_it_was(spec_name):
    """The reference cases of test_decoder_reference.py: the same bits with cache=None, and with a
    cache as well."""
    spec = SPECS[spec_name]
    wt = random_layer(spec, 1)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(BATCH, SEQ, spec.hidden, generator=g).to(torch.bfloat16)
    for xx, ww in ((x, wt), (x.float(), {k: v.float() for k, v in wt.items()})):
        want = forward_as_it_was(xx, ww, spec)
        assert torch.equal(decoder_forward(xx, ww, spec), want)
        assert torch.equal(decoder_forward(xx, ww, spec, cache=None), want)
    assert torch.equal(decoder_forward(x, wt, spec, cache=KVCache.allocate(spec, BATCH, SEQ)), forward_as_it_was(x, wt, spec))


# ---------------------------------------------------------------- errors

def error_cases(device):
    """[(name, thunk)]: every call must raise ValueError before any launch."""
    d, kvh, cap, b = 64, 2, 16, 2
    dev = torch.device(device)
    bf = dict(dtype=torch.bfloat16, device=dev)

    def caches(dd=d, kv=kvh, c=cap, **kw):
        return torch.zeros(b, kv, c, dd, **{**bf, **kw}), torch.zeros(b, kv, c, dd, **{**bf, **kw})

    def q(heads=4, dd=d, **kw):
        return torch.zeros(b, heads, dd, **{**bf, **kw})

    lens = torch.ones(b, dtype=torch.int32, device=dev)
    kc, vc = caches()
    tables = W._rope_tables(cap, d, 1e4, dev)
    rows = lambda n: torch.zeros(b, 1, n * d, **bf)  # noqa: E731
    other = torch.device("cpu") if dev.type == "cuda" else None
    out = [
        ("unsupported d", lambda: ops.attn_decode(q(dd=48), *caches(dd=48), lens)),
        ("d 256", lambda: ops.attn_decode(q(dd=256), *caches(dd=256), lens)),
        ("group above 16", lambda: ops.attn_decode(q(heads=34), kc, vc, lens)),
        ("heads % kv_heads", lambda: ops.attn_decode(q(heads=5), kc, vc, lens)),
        ("q dtype", lambda: ops.attn_decode(q(dtype=torch.float16), kc, vc, lens)),
        ("cache dtype", lambda: ops.attn_decode(q(), *caches(dtype=torch.float32), lens)),
        ("non-contiguous cache", lambda: ops.attn_decode(q(), kc.transpose(1, 2), vc.transpose(1, 2), lens)),
        ("sliced cache", lambda: ops.attn_decode(q(), torch.zeros(b, kvh, cap, 2 * d, **bf)[..., :d], vc, lens)),
        ("caches differ", lambda: ops.attn_decode(q(), kc, caches(c=cap + 1)[1], lens)),
        ("lens length", lambda: ops.attn_decode(q(), kc, vc, torch.ones(b + 1, dtype=torch.int32, device=dev))),
        ("lens dtype", lambda: ops.attn_decode(q(), kc, vc, lens.long())),
        ("max_len > capacity", lambda: ops.attn_decode(q(), kc, vc, lens, max_len=cap + 1)),
        ("max_len 0", lambda: ops.attn_decode(q(), kc, vc, lens, max_len=0)),
        ("out_dtype", lambda: ops.attn_decode(q(), kc, vc, lens, out_dtype=torch.float16)),
        ("q batch", lambda: ops.attn_decode(torch.zeros(b + 1, 4, d, **bf), kc, vc, lens)),
        ("rope: pos dtype", lambda: ops.rope_append(rows(4), rows(2), rows(2), *tables, kc, vc, lens.long())),
        ("rope: table shape", lambda: ops.rope_append(rows(4), rows(2), rows(2), tables[0][:-1], tables[1][:-1], kc, vc, lens)),
        ("rope: table dtype", lambda: ops.rope_append(rows(4), rows(2), rows(2), tables[0].double(), tables[1], kc, vc, lens)),
        ("rope: k width", lambda: ops.rope_append(rows(4), rows(1), rows(2), *tables, kc, vc, lens)),
        ("rope: q dtype", lambda: ops.rope_append(rows(4).float(), rows(2), rows(2), *tables, kc, vc, lens)),
        ("rope: heads % kv_heads", lambda: ops.rope_append(rows(5), rows(2), rows(2), *tables, kc, vc, lens)),
        ("rope: unsupported d", lambda: ops.rope_append(torch.zeros(b, 4 * 48, **bf), torch.zeros(b, 2 * 48, **bf),
                                                        torch.zeros(b, 2 * 48, **bf), *W._rope_tables(cap, 48, 1e4, dev),
                                                        *caches(dd=48), lens)),
    ]
    if other is not None:
        out += [
            ("lens device", lambda: ops.attn_decode(q(), kc, vc, lens.to(other))),
            ("q device", lambda: ops.attn_decode(q().to(other), kc, vc, lens)),
            ("cache devices", lambda: ops.attn_decode(q(), kc, vc.to(other), lens)),
            ("rope: pos device", lambda: ops.rope_append(rows(4), rows(2), rows(2), *tables, kc, vc, lens.to(other))),
            ("rope: q device", lambda: ops.rope_append(rows(4).to(other), rows(2), rows(2), *tables, kc, vc, lens)),
        ]
    spec = SPECS["tiny"]
    wt = {k: v.to(dev) for k, v in random_layer(spec, 1).items()}
    x = torch.zeros(b, 1, spec.hidden, **bf)

    def cache(batch=b, c=cap, max_len=3):
        kv = KVCache.allocate(spec, batch, c, dev)
        kv.max_len = max_len
        return kv

    out += [
        ("step: seq != 1", lambda: decoder_step(torch.zeros(b, 2, spec.hidden, **bf), wt, spec, cache())),
        ("step: batch", lambda: decoder_step(x, wt, spec, cache(batch=b + 1))),
        ("step: full cache", lambda: decoder_step(x, wt, spec, cache(max_len=cap))),
        ("step: other spec", lambda: decoder_step(torch.zeros(b, 1, SPECS["uneven"].hidden, **bf),
                                                  {k: v.to(dev) for k, v in random_layer(SPECS["uneven"], 1).items()},
                                                  SPECS["uneven"], cache())),
        ("step: act", lambda: decoder_step(x, wt, spec, cache(), act="fp8")),
        ("forward: prefill too long", lambda: decoder_forward(torch.zeros(b, 5, spec.hidden, **bf), wt, spec,
                                                              cache=cache(c=4))),
    ]
    return out


def check_errors(device):
    for name, thunk in error_cases(device):
        with pytest.raises(ValueError):
            thunk()
            pytest.fail(f"{name}: no ValueError")


def test_errors_cpu():
    check_errors("cpu")
