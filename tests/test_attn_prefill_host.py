"""ops.attn_prefill, ops.rope_append_seq and decoder_forward(attn="mfma", extend=) without a GPU: the
cases and the float64 reference that test_gpu_attn_prefill.py shares, the condition on the reference,
and the ops' CPU routes.

A case is d in (32, 64, 128) x group in (1, 2, 8) with 2 KV heads x S in (1, BK + 1, BQ + 1, 2 BQ + 3),
(BQ, BK) = _core.attn_prefill_tiles(): one batch of 4 sequences with start = (0, 1, BK - 1, BK + 5) and T
= BK + 5 + S + 3. q, K, V are seeded bf16 normals; the key at every position j >= start[b] is 8 sqrt(d)
q / |q|^2 for the q of row j - start[b] and head j % group of the KV head's group (that row and head
score 8 on their diagonal); below start[b] the keys at 0 and at the first and last position of every BK
tile are made the same way for row 0; everything at or behind start[b] + S is NaN and +-inf.
The condition (on the float64 reference alone): each such position carries a softmax weight of at
least 0.1 in its (row, head). The bound is attn_decode_cases.py's: 2^-7 sum_j p_j |v_j| per element for
an f32 result, 2^-9 |y64| more for bf16.
Measured: the smallest marked weight 0.247; CPU routes err / bound at most 2.3e-4 in f32 (the route is f32
throughout) and 0.40 in bf16."""
import functools

import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd import _core, ops
from distributed_llm_dissemination_amd.models import weights as W
from distributed_llm_dissemination_amd.models.weights import KVCache, decoder_forward, decoder_step, random_layer

import decoder_packed_reference as dp
from attn_decode_cases import f64, garbage, to_bits
from test_attn_decode_host import PREFILL, ROPE_SHAPES, STEP_B, step_params
from test_decoder_reference import SPECS

BQ, BK = _core.attn_prefill_tiles()
KVH = 2
STARTS = (0, 1, BK - 1, BK + 5)
CASES = [(d, g, s) for d in (32, 64, 128) for g in (1, 2, 8) for s in (1, BK + 1, BQ + 1, 2 * BQ + 3)]


def case_id(c):
    return f"d{c[0]}-g{c[1]}-s{c[2]}"


@functools.lru_cache(maxsize=None)
def case(d, group, s):
    """dict: q [4, S, heads, d], k, v [4, KVH, T, d] (CPU bf16), start, marks [(b, row, head, position)] and
    the float64 y64, bound [4, S, heads * d]."""
    t_len, heads = BK + 5 + s + 3, KVH * group
    g = torch.Generator().manual_seed(100 * d + 10 * group + s)
    q = torch.randn(4, s, heads, d, generator=g).to(torch.bfloat16)
    k = torch.randn(4, KVH, t_len, d, generator=g).to(torch.bfloat16)
    v = torch.randn(4, KVH, t_len, d, generator=g).to(torch.bfloat16)
    marks = []
    for b, st in enumerate(STARTS):
        edges = {0} | {j for j in range(st) if j % BK in (0, BK - 1)}
        for j, row in [(j, 0) for j in sorted(edges) if j < st] + [(st + i, i) for i in range(s)]:
            for kv in range(KVH):
                h = kv * group + j % group
                qh = q[b, row, h].double()
                k[b, kv, j] = (8.0 * d ** 0.5 * qh / (qh * qh).sum()).to(torch.bfloat16)
                marks.append((b, row, h, j))
        k[b, :, st + s:] = garbage((KVH, t_len - st - s, d), 3 * b + 1)
        v[b, :, st + s:] = garbage((KVH, t_len - st - s, d), 3 * b + 2)
    y64, bound, p = reference(q, k, v, STARTS)
    return dict(id=case_id((d, group, s)), q=q, k=k, v=v, start=torch.tensor(STARTS, dtype=torch.int32), marks=marks,
                y64=y64, bound=bound, p=p)


def reference(q, k, v, starts):
    """float64 from the definition, causal, per row: (y64, bound [B, S, heads * d], p {(b, h): [S, n]})."""
    nb, s, heads, d = q.shape
    group = heads // k.shape[1]
    q64, k64, v64 = f64(q), f64(k), f64(v)
    y, bound, ps = np.zeros((nb, s, heads, d)), np.zeros((nb, s, heads, d)), {}
    for b, st in enumerate(starts):
        n = st + s
        seen = np.arange(n)[None, :] <= (st + np.arange(s))[:, None]
        for h in range(heads):
            sc = np.where(seen, q64[b, :, h] @ k64[b, h // group, :n].T / np.sqrt(d), -np.inf)
            e = np.exp(sc - sc.max(-1, keepdims=True))
            p = e / e.sum(-1, keepdims=True)
            y[b, :, h] = p @ v64[b, h // group, :n]
            bound[b, :, h] = 2.0 ** -7 * (p @ np.abs(v64[b, h // group, :n]))
            ps[(b, h)] = p
    return y.reshape(nb, s, heads * d), bound.reshape(nb, s, heads * d), ps


def err_over_bound(y, c, bf16):
    """Worst |y - y64| / bound of y [4, S, heads * d]; asserts no NaN."""
    got = y.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    bound = c["bound"] + (2.0 ** -9 * np.abs(c["y64"]) if bf16 else 0.0)
    assert (bound > 0).all()
    return float((np.abs(got - c["y64"]) / bound).max())


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_marked_positions_carry_weight(c):
    cc = case(*c)
    w = min(cc["p"][(b, h)][row, j] for b, row, h, j in cc["marks"])
    print(cc["id"], "smallest marked weight", w)
    assert w >= 0.1
    assert max(STARTS) + c[2] < 350 and (BK + 5 + c[2] + 3) % BK and {j for b, _, _, j in cc["marks"] if b == 3} >= {0, BK - 1, BK}


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_attn_prefill_cpu_route_matches_float64(c):
    cc = case(*c)
    y32 = ops.attn_prefill(cc["q"], cc["k"], cc["v"], cc["start"], out_dtype=torch.float32)
    y16 = ops.attn_prefill(cc["q"], cc["k"], cc["v"], cc["start"])
    assert y32.dtype == torch.float32 and y16.dtype == torch.bfloat16 and tuple(y32.shape) == tuple(y16.shape) == cc["y64"].shape
    w32, w16 = err_over_bound(y32, cc, False), err_over_bound(y16, cc, True)
    print(cc["id"], "cpu route err / bound: f32", w32, "bf16", w16)
    assert w32 <= 1 and w16 <= 1
    assert torch.equal(ops.attn_prefill(cc["q"][:1], cc["k"][:1], cc["v"][:1], out_dtype=torch.float32)[0], y32[0])  # start None
    cut = BK + 5 + c[2] - 2  # T cut short: sequence 3's last two rows have no position
    yc = ops.attn_prefill(cc["q"], cc["k"][:, :, :cut], cc["v"][:, :, :cut], cc["start"], out_dtype=torch.float32)
    assert not yc[3, -2:].any() and torch.equal(yc[:3], y32[:3]) and torch.equal(yc[3, :-2], y32[3, :-2])


# ---------------------------------------------------------------- rope_append_seq

def check_rope_append_seq(heads, kvh, d, device, merged, theta=500000.0):
    """rope_append_seq on `device` against `_rope` on that device at positions start[b] + i, bit for bit, the V
    rows v, every other byte of the caches unchanged; one start pushes the tail outside the capacity."""
    cap, s, start = 37, 7, [0, 5, 33, -2]
    b = len(start)
    g = torch.Generator().manual_seed(3)
    y = torch.randn(b, s, (heads + 2 * kvh) * d, generator=g).to(torch.bfloat16).to(device)
    q, k, v = y[..., : heads * d], y[..., heads * d: (heads + kvh) * d], y[..., (heads + kvh) * d:]
    if not merged:
        q, k, v = q.clone(), k.clone(), v.clone()
    cos, sin = W._rope_tables(cap, d, theta, device)
    k0 = torch.randn(b, kvh, cap, d, generator=g).to(torch.bfloat16).to(device)
    v0 = torch.randn(b, kvh, cap, d, generator=g).to(torch.bfloat16).to(device)
    kc, vc = k0.clone(), v0.clone()
    q_out = ops.rope_append_seq(q, k, v, cos, sin, kc, vc, torch.tensor(start, dtype=torch.int32, device=device))
    assert q_out.dtype == torch.bfloat16 and tuple(q_out.shape) == (b, s, heads, d)
    ek, ev = k0.clone(), v0.clone()
    for i, st in enumerate(start):
        for x, nh, out in ((q, heads, None), (k, kvh, ek)):
            seq = torch.zeros(1, nh, cap + s, d, dtype=torch.bfloat16, device=device)  # row t at position st + t
            ok = [t for t in range(s) if 0 <= st + t < cap]
            pos = [st + t for t in ok]
            seq[0][:, pos] = x[i, ok].reshape(len(ok), nh, d).transpose(0, 1)
            want = W._rope(seq, theta)[0][:, pos]  # [nh, ok, d]
            if out is None:
                assert np.array_equal(to_bits(q_out[i, ok]), to_bits(want.transpose(0, 1)))
                assert not to_bits(q_out[i, [t for t in range(s) if t not in ok]]).any()  # outside: zero rows
            else:
                out[i][:, pos] = want
                ev[i][:, pos] = v[i, ok].reshape(len(ok), kvh, d).transpose(0, 1)
    assert np.array_equal(to_bits(kc), to_bits(ek)) and np.array_equal(to_bits(vc), to_bits(ev))


@pytest.mark.parametrize("merged", [True, False], ids=["merged", "separate"])
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=list(ROPE_SHAPES))
def test_rope_append_seq_cpu_route_is_rope_bit_for_bit(shape, merged):
    check_rope_append_seq(*ROPE_SHAPES[shape], "cpu", merged)


# ---------------------------------------------------------------- decoder_forward(attn="mfma")

def check_forward_mfma(route, spec_name, device):
    """Every row within 2 max(e16, d_ctl) of the float64 ref_decoder over 9 tokens, d_ctl the default route's
    distance on the same device and parameters (on the CPU also d_cpu, check A's tolerance); cache rows the
    default route's bit for bit; prefill 5 + extend 4; prefill 4 + extend 4 + one decoder_step."""
    c, p, kw = step_params(route, spec_name, device)
    spec, x = c.spec, c.xt.to(device)
    n = x.shape[1]
    dist = lambda y, lo=0: dp.row_rel(y.float().cpu().numpy(), c.y64[:, lo: lo + y.shape[1]])  # noqa: E731
    ctl_cache = KVCache.allocate(spec, STEP_B, n + 2, device)
    d_ctl = dist(decoder_forward(x, p, spec, cache=ctl_cache, **kw))
    tol = 2 * max(c.row_e16.max(), d_ctl.max()) if device != "cpu" else c.row_tol(d_ctl)
    cache = KVCache.allocate(spec, STEP_B, n + 2, device)
    for what, y in (("no cache", decoder_forward(x, p, spec, attn="mfma", **kw)),
                    ("cache", decoder_forward(x, p, spec, attn="mfma", cache=cache, **kw))):
        print(c.id, route, what, "worst row dist / tolerance", dist(y).max() / tol)
        assert y.dtype == torch.bfloat16 and (dist(y) <= tol).all()
    assert cache.max_len == n and cache.lens.tolist() == [n] * STEP_B
    assert np.array_equal(to_bits(cache.k[:, :, :n]), to_bits(ctl_cache.k[:, :, :n]))
    assert np.array_equal(to_bits(cache.v[:, :, :n]), to_bits(ctl_cache.v[:, :, :n]))
    for first, more, step in ((PREFILL, n - PREFILL, False), (4, 4, True)):
        cache = KVCache.allocate(spec, STEP_B, n + 2, device)
        decoder_forward(x[:, :first], p, spec, attn="mfma", cache=cache, **kw)
        y = decoder_forward(x[:, first: first + more], p, spec, attn="mfma", cache=cache, extend=True, **kw)
        print(c.id, route, "extend", more, "worst row dist / tolerance", dist(y, first).max() / tol)
        assert (dist(y, first) <= tol).all()
        assert cache.max_len == first + more and cache.lens.tolist() == [first + more] * STEP_B
        if step:
            ys = decoder_step(x[:, 8:9], p, spec, cache, **kw)
            assert (dist(ys, 8) <= tol).all() and cache.lens.tolist() == [9] * STEP_B
        else:
            assert np.array_equal(to_bits(cache.k[:, :, :n]), to_bits(ctl_cache.k[:, :, :n]))


@pytest.mark.parametrize("route", ["plain", "mxfp4"])
@pytest.mark.parametrize("spec_name", SPECS, ids=list(SPECS))
@dp.one_thread
def test_forward_mfma_cpu_matches_float64(spec_name, route):
    check_forward_mfma(route, spec_name, "cpu")


# ---------------------------------------------------------------- errors

def error_cases(device):
    """[(name, thunk)]: every call must raise ValueError before any launch."""
    d, kvh, t_len, b, s = 64, 2, 16, 2, 3
    dev = torch.device(device)
    bf = dict(dtype=torch.bfloat16, device=dev)
    z = lambda *shape, **kw: torch.zeros(*shape, **{**bf, **kw})  # noqa: E731
    q, k, start = z(b, s, 4, d), z(b, kvh, t_len, d), torch.zeros(b, dtype=torch.int32, device=dev)
    tables = W._rope_tables(t_len, d, 1e4, dev)
    rq, rk = z(b, s, 4 * d), z(b, s, kvh * d)
    spec = SPECS["tiny"]
    wt = {n: w.to(dev) for n, w in random_layer(spec, 1).items()}
    x = z(b, s, spec.hidden)
    cache = lambda cap=8, max_len=0: KVCache(**{**vars(KVCache.allocate(spec, b, cap, dev)), "max_len": max_len})  # noqa: E731
    ks = (kvh * t_len * d, t_len * d, d)
    raw = lambda kst, dd=d: _core.attn_prefill(q.data_ptr(), k.data_ptr(), k.data_ptr(), 0, b, s, 4, kvh, dd, t_len, kst, ks,  # noqa: E731
                                               z(b, s, 4 * d).data_ptr(), True, 0)
    out = [
        ("q dtype", lambda: ops.attn_prefill(q.float(), k, k)),
        ("k dtype", lambda: ops.attn_prefill(q, k.float(), k.float())),
        ("k, v shapes", lambda: ops.attn_prefill(q, k, z(b, kvh, t_len + 1, d))),
        ("d 48", lambda: ops.attn_prefill(z(b, s, 4, 48), z(b, kvh, t_len, 48), z(b, kvh, t_len, 48))),
        ("heads % kv_heads", lambda: ops.attn_prefill(z(b, s, 5, d), k, k)),
        ("start dtype", lambda: ops.attn_prefill(q, k, k, start.long())),
        ("out_dtype", lambda: ops.attn_prefill(q, k, k, out_dtype=torch.float16)),
        ("stride % 8 at the binding", lambda: raw((ks[0], ks[1], d + 4))),
        ("rope: q dtype", lambda: ops.rope_append_seq(rq.float(), rk, rk, *tables, k, k.clone(), start)),
        ("rope: k width", lambda: ops.rope_append_seq(rq, z(b, s, d), rk, *tables, k, k.clone(), start)),
        ("rope: heads % kv_heads", lambda: ops.rope_append_seq(z(b, s, 5 * d), rk, rk, *tables, k, k.clone(), start)),
        ("rope: sliced cache", lambda: ops.rope_append_seq(rq, rk, rk, *tables, z(b, kvh, t_len, 2 * d)[..., :d], k, start)),
        ("forward: unknown attn", lambda: decoder_forward(x, wt, spec, attn="flash")),
        ("forward: extend without a cache", lambda: decoder_forward(x, wt, spec, attn="mfma", extend=True)),
        ("forward: extend without mfma", lambda: decoder_forward(x, wt, spec, cache=cache(), extend=True)),
        ("forward: extend past the capacity", lambda: decoder_forward(x, wt, spec, attn="mfma", cache=cache(8, 6), extend=True)),
        ("forward: prefill too long", lambda: decoder_forward(x, wt, spec, attn="mfma", cache=cache(2))),
    ]
    if dev.type == "cuda":
        out += [
            ("k device", lambda: ops.attn_prefill(q, k.cpu(), k.cpu())),
            ("start device", lambda: ops.attn_prefill(q, k, k, start.cpu())),
            ("rope: q device", lambda: ops.rope_append_seq(rq.cpu(), rk, rk, *tables, k, k.clone(), start)),
        ]
    return out


def check_errors(device):
    for name, thunk in error_cases(device):
        with pytest.raises(ValueError):
            thunk()
            pytest.fail(f"{name}: no ValueError")


def test_errors_cpu():
    check_errors("cpu")
