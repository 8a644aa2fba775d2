#!/usr/bin/env python3
"""ops.attn_prefill on an MXFP8 KV cache (k_scale=, v_scale=; csrc/kernels/attn_prefill_mxfp8.hip) against
the bf16 kernel on the same, dequantized cache, and decoder_forward(attn="mfma_mxfp8") against the default
route's prefill of an MXFP8 cache, in one process and run (one MI355X).

Per model (llama3-70b: 64 heads, 8 KV heads, d 128; llama3-8b: 32 / 8 / 128), the shapes of
scripts/attn_prefill_bench.py - batch B in {1, 8} and S in {512, 2048, 8192} at start 0, plus the extend
rows (S 512 at start 7680) - the columns:

  (a)  mxfp8   ops.attn_prefill(q, k_codes, v_codes, start, k_scale=, v_scale=)
  (b)  bf16    ops.attn_prefill(q, dequant(K), dequant(V), start): attn_prefill.hip, whose generated code
               this kernel's file leaves as it was
  (a') (b')    each with its append from the merged q/k/v buffer: ops.rope_append_seq with and without scales

and, for one llama3-8b layer of random plain weights at B = 1 (--layer-seqs), the whole
decoder_forward(x, attn="mfma_mxfp8", cache=) against decoder_forward(x, cache=) on an MXFP8 cache: the
default route, SDPA on the fresh bf16 k and v plus ops.mxfp8_quantize_rows into the cache.

Rounds are interleaved over the columns; a round times `reps` calls between two device events, `reps`
chosen per column so that a round lasts about --window-ms. Printed: the median microseconds per call and
the spread (max - min over the rounds, relative to the median) of every column, a / b, whether (a) and (b)
have the same bits, and whether a / b leaves 1 by more than the larger spread.

    python scripts/attn_prefill_mxfp8_bench.py [--rounds 5] [--window-ms 40] [--out FILE]
"""

import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from distributed_llm_dissemination_amd import ops  # noqa: E402
from distributed_llm_dissemination_amd.models.weights import (PRESETS, KVCache, _rope_tables, decoder_forward,  # noqa: E402
                                                              random_layer)

MODELS = ["llama3-70b", "llama3-8b"]
SHAPES = [(b, s, 0) for b in (1, 8) for s in (512, 2048, 8192)] + [(1, 512, 7680), (8, 512, 7680)]


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps  # microseconds per call


def dequant(codes, scales):
    """code * 2^(byte - 127) as bf16 on the codes' device (exact for what the quantizer writes)."""
    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(codes.device)
    return torch.ldexp(lut[codes.long()], scales.int().repeat_interleave(32, -1) - 127).to(torch.bfloat16)


def measure(cases, rounds, window_ms):
    """{column: (median us, spread)} of interleaved rounds."""
    reps = {}
    for c, fn in cases.items():  # warm-up of every column, and its reps from a first timing
        fn()
        torch.cuda.synchronize()
        reps[c] = max(2, min(200, int(window_ms * 1e3 / max(timed(fn, 2), 1.0))))
    times = {c: [] for c in cases}
    for _ in range(rounds):
        for c, fn in cases.items():
            times[c].append(timed(fn, reps[c]))
    return {c: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for c, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--models", default="", help="comma-separated subset of " + ",".join(MODELS))
    ap.add_argument("--max-tokens", type=int, default=1 << 30, help="skip shapes with more than this many B * S")
    ap.add_argument("--layer-seqs", default="512,2048,8192", help="S of the decoder_forward rows; empty for none")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_prefill_mxfp8_bench needs a GPU")
    rows, lines = [], []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    cols = ["a", "b", "a'", "b'"]
    emit(f"{'model':11s} {'B':>2s} {'S':>5s} {'start':>5s} " + " ".join(f"{'(' + c + ') us':>10s} {'sprd':>5s}" for c in cols) +
         f" {'a/b':>6s} {'a`/b`':>6s}  bits  a/b beyond the spread")
    for model in (args.models.split(",") if args.models else MODELS):
        spec = PRESETS[model]
        heads, kvh, d = spec.heads, spec.kv_heads, spec.head_dim
        n_all = (heads + 2 * kvh) * d
        for b, s, st in SHAPES:
            if b * s > args.max_tokens:
                continue
            g = torch.Generator(device="cuda").manual_seed(b + s + st)
            cap = st + s
            y = torch.randn(b, s, n_all, device="cuda", generator=g).to(torch.bfloat16)  # one merged q/k/v projection
            qm, km, vm = y[..., : heads * d], y[..., heads * d: (heads + kvh) * d], y[..., (heads + kvh) * d:]
            (kc, ks), (vc, vs) = (ops.mxfp8_quantize_rows(torch.randn(b, kvh, cap, d, device="cuda", generator=g).to(torch.bfloat16))
                                  for _ in range(2))
            cos, sin = _rope_tables(cap, d, spec.rope_theta, "cuda")
            start = torch.full((b,), st, dtype=torch.int32, device="cuda")
            mxkw = dict(k_scale=ks, v_scale=vs)
            q_rot = ops.rope_append_seq(qm, km, vm, cos, sin, kc, vc, start, **mxkw)  # the caches now hold these tokens
            kd, vd = dequant(kc, ks), dequant(vc, vs)
            cases = {
                "a": lambda: ops.attn_prefill(q_rot, kc, vc, start, **mxkw),
                "b": lambda: ops.attn_prefill(q_rot, kd, vd, start),
                "a'": lambda: ops.attn_prefill(ops.rope_append_seq(qm, km, vm, cos, sin, kc, vc, start, **mxkw), kc, vc, start, **mxkw),
                "b'": lambda: ops.attn_prefill(ops.rope_append_seq(qm, km, vm, cos, sin, kd, vd, start), kd, vd, start),
            }
            same = bool(torch.equal(cases["a"]().view(torch.int16), cases["b"]().view(torch.int16)))
            m = measure(cases, args.rounds, args.window_ms)
            ratio, ratio2 = m["a"][0] / m["b"][0], m["a'"][0] / m["b'"][0]
            beyond = abs(m["a"][0] - m["b"][0]) > max(m["a"][1] * m["a"][0], m["b"][1] * m["b"][0])
            rows.append({"model": model, "heads": heads, "kv_heads": kvh, "d": d, "B": b, "S": s, "start": st,
                         "us": {c: round(m[c][0], 2) for c in cols}, "spread": {c: round(m[c][1], 3) for c in cols},
                         "a_over_b": round(ratio, 3), "a2_over_b2": round(ratio2, 3), "same_bits": same,
                         "a_b_differ_beyond_spread": bool(beyond)})
            emit(f"{model:11s} {b:2d} {s:5d} {st:5d} " + " ".join(f"{m[c][0]:10.1f} {m[c][1]:5.2f}" for c in cols) +
                 f" {ratio:6.3f} {ratio2:6.3f}  {'same' if same else 'DIFFER'}  {'yes' if beyond else 'no'}")
            del y, kc, ks, vc, vs, kd, vd, q_rot, cases
            torch.cuda.empty_cache()
    seqs = [int(n) for n in args.layer_seqs.split(",") if n]
    if seqs:
        spec = PRESETS["llama3-8b"]
        w = {n: t.cuda() for n, t in random_layer(spec, 7).items()}
        emit("decoder_forward, one llama3-8b layer, plain weights, B 1, an MXFP8 cache: (m) attn='mfma_mxfp8'  (d) the default route")
        for s in seqs:
            x = torch.randn(1, s, spec.hidden, device="cuda", generator=torch.Generator(device="cuda").manual_seed(s)).to(torch.bfloat16)
            cache = KVCache.allocate(spec, 1, s, "cuda", kv_format="mxfp8")
            m = measure({"m": lambda: decoder_forward(x, w, spec, cache=cache, attn="mfma_mxfp8"),
                         "d": lambda: decoder_forward(x, w, spec, cache=cache)}, args.rounds, args.window_ms)
            rows.append({"model": "llama3-8b layer", "B": 1, "S": s, "us": {c: round(m[c][0], 1) for c in m},
                         "spread": {c: round(m[c][1], 3) for c in m}, "m_over_d": round(m["m"][0] / m["d"][0], 3)})
            emit(f"  S {s:5d}  (m) {m['m'][0]:10.1f} us {m['m'][1]:5.2f}  (d) {m['d'][0]:10.1f} us {m['d'][1]:5.2f}  m/d {m['m'][0] / m['d'][0]:6.3f}")
    out = {"rounds": args.rounds, "window_ms": args.window_ms, "torch": torch.__version__,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
