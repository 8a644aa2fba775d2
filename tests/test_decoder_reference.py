"""An independent reference for models/weights.py decoder_forward, which every forward-pass test
otherwise only compares with itself. A decoder layer written from the definition in numpy, with
explicit loops over heads and positions and none of weights.py's helpers:

  RMSNorm         x / sqrt(mean(x^2) + eps) * w
  RoPE            rotate-half: the pairs (i, i + d/2), angle pos * theta^(-2i/d)
  attention       query head h reads KV head h // (heads // kv_heads); causal softmax of q.k / sqrt(d)
  MLP             down(silu(gate(h)) * up(h))
  both residuals

The tolerance comes from the reference alone: the same code evaluated in np.float32 lies e32
(relative L2) from the float64 evaluation - the f32 noise floor - and decoder_forward in float32
must be within 20 e32 (the factor covers torch's other summation order and its fused attention).
The inputs discriminate: the float64 reference with each of five plausible mistakes lies at least
100 tolerances away. For bf16 the bound is taken the same way from a twin of the reference that
rounds to bf16 wherever decoder_forward does."""
import numpy as np
import pytest
import torch

from distributed_llm_dissemination_amd.models.weights import PRESETS, DecoderSpec, decoder_forward, random_layer

SPECS = {
    "tiny": PRESETS["tiny"],  # hidden 256, 4 heads, 2 KV heads
    "uneven": DecoderSpec("uneven", 192, 320, 6, 3, 1),  # nothing square: head_dim 32, 2 query heads per KV head
}
BATCH, SEQ = 2, 8
MISTAKES = ("interleaved_rope", "kv_modulo", "no_causal_mask", "eps_outside_sqrt", "silu_on_up")


def bf16_round(a):
    """float64/float32 array -> the nearest bf16 value (ties to even), in the array's dtype."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return r.astype(np.asarray(a).dtype)


def ref_decoder(x, w, spec, dtype=np.float64, mistake=None, rnd=lambda a: a):
    """One decoder layer on x [batch, seq, hidden]; w: {name: array}. Everything is computed in
    `dtype`; `rnd` is applied where decoder_forward rounds to its working dtype; `mistake` swaps in
    one wrong convention."""
    assert mistake is None or mistake in MISTAKES
    x = np.asarray(x, dtype=dtype)
    w = {k: np.asarray(v, dtype=dtype) for k, v in w.items()}
    nb, ns, hid = x.shape
    nh, nkv, d = spec.heads, spec.kv_heads, spec.hidden // spec.heads
    eps, one = dtype(spec.eps), dtype(1)

    def rms(v, g):
        ms = (v * v).mean(dtype=dtype)
        den = np.sqrt(ms) + eps if mistake == "eps_outside_sqrt" else np.sqrt(ms + eps)
        return rnd(v / den * g)

    def rope(v, pos):
        out = np.empty_like(v)
        for i in range(d // 2):
            ang = dtype(pos) * dtype(spec.rope_theta) ** dtype(-2.0 * i / d)
            c, s = np.cos(ang), np.sin(ang)
            a, b = (2 * i, 2 * i + 1) if mistake == "interleaved_rope" else (i, i + d // 2)
            out[a] = v[a] * c - v[b] * s
            out[b] = v[b] * c + v[a] * s
        return rnd(out)

    def silu(v):
        return v / (one + np.exp(-v))

    y = np.empty_like(x)
    for b in range(nb):
        h = np.stack([rms(x[b, t], w["input_layernorm"]) for t in range(ns)])
        q, k, v = rnd(h @ w["q_proj"].T), rnd(h @ w["k_proj"].T), rnd(h @ w["v_proj"].T)
        att = np.empty((ns, nh * d), dtype=dtype)
        for hq in range(nh):
            hk = hq % nkv if mistake == "kv_modulo" else hq // (nh // nkv)
            qs = [rope(q[t, hq * d: (hq + 1) * d], t) for t in range(ns)]
            ks = [rope(k[t, hk * d: (hk + 1) * d], t) for t in range(ns)]
            for t in range(ns):
                last = ns if mistake == "no_causal_mask" else t + 1
                sc = np.array([qs[t] @ ks[j] for j in range(last)], dtype=dtype) / np.sqrt(dtype(d))
                p = np.exp(sc - sc.max())
                p = p / p.sum(dtype=dtype)
                att[t, hq * d: (hq + 1) * d] = sum(p[j] * v[j, hk * d: (hk + 1) * d] for j in range(last))
        x1 = rnd(x[b] + rnd(rnd(att) @ w["o_proj"].T))
        h2 = np.stack([rms(x1[t], w["post_attention_layernorm"]) for t in range(ns)])
        g, u = rnd(h2 @ w["gate_proj"].T), rnd(h2 @ w["up_proj"].T)
        act = rnd(rnd(silu(u)) * g) if mistake == "silu_on_up" else rnd(rnd(silu(g)) * u)
        y[b] = rnd(x1 + rnd(act @ w["down_proj"].T))
    return y


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.fixture(scope="module", params=list(SPECS))
def case(request):
    """Per spec: bf16-representable weights and inputs (so that every precision sees the same
    numbers), the float64 reference and e32. The positions of x have scales from 0.003 to 1: with
    mean(x^2) near eps, where eps stands matters."""
    spec = SPECS[request.param]
    wt = random_layer(spec, 3)  # bf16
    g = torch.Generator().manual_seed(11)
    scale = torch.logspace(-2.5, 0, SEQ)[torch.randperm(SEQ, generator=g)]
    xt = (torch.randn(BATCH, SEQ, spec.hidden, generator=g) * scale[None, :, None]).to(torch.bfloat16)
    w = {k: v.float().numpy().astype(np.float64) for k, v in wt.items()}
    x = xt.float().numpy().astype(np.float64)
    y64 = ref_decoder(x, w, spec)
    e32 = rel(ref_decoder(x, w, spec, np.float32), y64)
    return dict(name=request.param, spec=spec, wt=wt, xt=xt, w=w, x=x, y64=y64, e32=e32, tol=20 * e32)


def test_float32_forward_matches_the_reference(case):
    y = decoder_forward(case["xt"].float(), {k: v.float() for k, v in case["wt"].items()}, case["spec"])
    dist = rel(y.numpy(), case["y64"])
    print(case["name"], "e32", case["e32"], "decoder_forward float32 distance", dist, "tolerance", case["tol"])
    assert 1e-8 < case["e32"] < 1e-6  # an f32 noise floor
    assert dist <= case["tol"]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_inputs_discriminate(case, mistake):
    dist = rel(ref_decoder(case["x"], case["w"], case["spec"], mistake=mistake), case["y64"])
    print(case["name"], mistake, "distance", dist, "tolerances", dist / case["tol"])
    assert dist >= 100 * case["tol"]


def test_bfloat16_forward_matches_the_reference(case):
    """decoder_forward on bf16 tensors against the float64 reference on the same (bf16-valued)
    weights; e16 is the distance of the reference that rounds to bf16 where decoder_forward does."""
    e16 = rel(ref_decoder(case["x"], case["w"], case["spec"], rnd=bf16_round), case["y64"])
    y = decoder_forward(case["xt"], case["wt"], case["spec"])
    assert y.dtype == torch.bfloat16
    dist = rel(y.float().numpy(), case["y64"])
    print(case["name"], "e16", e16, "decoder_forward bfloat16 distance", dist, "tolerance", 20 * e16)
    assert 1e-4 < e16 < 2e-2
    assert dist <= 20 * e16
