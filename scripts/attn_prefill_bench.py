#!/usr/bin/env python3
"""ops.attn_prefill (causal GQA prefill / extend attention that reads the KV cache) against the ways plain
torch attends S new tokens, in one process and run (one MI355X).

Per model (llama3-70b: 64 heads, 8 KV heads, d 128; llama3-8b: 32 / 8 / 128), batch B in {1, 8} and S in
{512, 2048, 8192} at start 0, plus one extend row (S 512 at start 7680), the columns:

  (a)  attn_prefill  ops.attn_prefill(q, k_cache, v_cache, start) reading the cache
  (b)  repeat+sdpa   the baseline, what decoder_forward does: repeat_interleave of K and V by heads //
                     kv_heads, then F.scaled_dot_product_attention(is_causal=True) (extend: a boolean mask)
  (c)  sdpa gqa      F.scaled_dot_product_attention(..., enable_gqa=True), where this torch has it
  (a') (b')          (a) and (b) each with its rope and cache write: ops.rope_append_seq from the merged
                     q/k/v buffer, against `_rope` of q and k plus the slice-assign into the cache - the
                     stage as the layer sees it

Rounds are interleaved over the columns; a round times `reps` calls between two device events, `reps`
chosen per column so that a round lasts about --window-ms. Printed: the median microseconds per call and
the spread (max - min over the rounds, relative to the median) of every column, TFLOP/s of (a) and (b)
counting 4 d heads B (S start + S (S + 1) / 2) flops, the ratios, and whether (a') beats (b') by more than
the larger of the two spreads.

    python scripts/attn_prefill_bench.py [--rounds 5] [--window-ms 40] [--out FILE]
"""

import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from distributed_llm_dissemination_amd import _core, ops  # noqa: E402
from distributed_llm_dissemination_amd.models.weights import PRESETS, _rope_tables  # noqa: E402

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


def rope_at(x, cos, sin):
    """`_rope`'s expression over [B, heads, S, d] with the table rows of the tokens' positions."""
    d = x.shape[-1]
    xf = x.float()
    return (xf * cos + torch.cat([-xf[..., d // 2:], xf[..., : d // 2]], -1) * sin).to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--models", default="", help="comma-separated subset of " + ",".join(MODELS))
    ap.add_argument("--max-tokens", type=int, default=1 << 30, help="skip shapes with more than this many B * S")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_prefill_bench needs a GPU")
    try:
        F.scaled_dot_product_attention(*(torch.zeros(1, n, 4, 32, dtype=torch.bfloat16, device="cuda") for n in (2, 1, 1)),
                                       enable_gqa=True)
        have_gqa = True
    except (TypeError, RuntimeError):
        have_gqa = False
    rows, lines = [], []
    cols = ["a", "b"] + (["c"] if have_gqa else []) + ["a'", "b'"]
    head = f"{'model':11s} {'B':>2s} {'S':>5s} {'start':>5s} " + " ".join(f"{'(' + c + ') us':>10s} {'sprd':>5s}" for c in cols) + \
        f" {'a TF/s':>7s} {'b TF/s':>7s} {'b/a':>6s} {'c/a':>6s} {'b`/a`':>6s}  a' beats b'"
    lines.append(head)
    print(head, flush=True)
    for model in (args.models.split(",") if args.models else MODELS):
        spec = PRESETS[model]
        heads, kvh, d = spec.heads, spec.kv_heads, spec.head_dim
        group, n_all = heads // kvh, (heads + 2 * kvh) * d
        for b, s, st in SHAPES:
            if b * s > args.max_tokens:
                continue
            g = torch.Generator(device="cuda").manual_seed(b + s + st)
            cap = st + s
            y = torch.randn(b, s, n_all, device="cuda", generator=g).to(torch.bfloat16)  # one merged q/k/v projection
            qm, km, vm = y[..., : heads * d], y[..., heads * d: (heads + kvh) * d], y[..., (heads + kvh) * d:]
            kc = torch.randn(b, kvh, cap, d, device="cuda", generator=g).to(torch.bfloat16)
            vc = torch.randn(b, kvh, cap, d, device="cuda", generator=g).to(torch.bfloat16)
            cos, sin = _rope_tables(cap, d, spec.rope_theta, "cuda")
            start = torch.full((b,), st, dtype=torch.int32, device="cuda")
            q_rot = ops.rope_append_seq(qm, km, vm, cos, sin, kc, vc, start)  # the caches now hold these tokens
            q4 = q_rot.transpose(1, 2)  # [B, heads, S, d]
            mask = None
            if st:
                mask = torch.arange(cap, device="cuda")[None, :] <= (st + torch.arange(s, device="cuda"))[:, None]
            kw = dict(attn_mask=mask) if st else dict(is_causal=True)

            def run_a():
                return ops.attn_prefill(q_rot, kc, vc, start)

            def run_b(q=q4):
                return F.scaled_dot_product_attention(q, kc.repeat_interleave(group, dim=1), vc.repeat_interleave(group, dim=1), **kw)

            def run_c():
                return F.scaled_dot_product_attention(q4, kc, vc, enable_gqa=True, **kw)

            def run_a2():
                return ops.attn_prefill(ops.rope_append_seq(qm, km, vm, cos, sin, kc, vc, start), kc, vc, start)

            def run_b2():
                q = rope_at(qm.view(b, s, heads, d).transpose(1, 2), cos[st:], sin[st:])
                kc[:, :, st:] = rope_at(km.view(b, s, kvh, d).transpose(1, 2), cos[st:], sin[st:])
                vc[:, :, st:] = vm.view(b, s, kvh, d).transpose(1, 2)
                return run_b(q)

            cases = {"a": run_a, "b": run_b, "c": run_c, "a'": run_a2, "b'": run_b2}
            cases = {c: cases[c] for c in cols}
            ya, yb = run_a().float().view(b, s, heads, d), run_b().float().transpose(1, 2)
            rel = float((ya - yb).norm() / yb.norm())
            reps = {}
            for c, fn in cases.items():  # warm-up of every column, and its reps from a first timing
                fn()
                torch.cuda.synchronize()
                reps[c] = max(2, min(200, int(args.window_ms * 1e3 / max(timed(fn, 2), 1.0))))
            times = {c: [] for c in cases}
            for _ in range(args.rounds):
                for c, fn in cases.items():
                    times[c].append(timed(fn, reps[c]))
            med = {c: statistics.median(t) for c, t in times.items()}
            spread = {c: (max(t) - min(t)) / med[c] for c, t in times.items()}
            flops = 4 * d * heads * b * (s * st + s * (s + 1) // 2)
            beats = med["b'"] - med["a'"] > max(spread["a'"] * med["a'"], spread["b'"] * med["b'"])
            row = {"model": model, "heads": heads, "kv_heads": kvh, "d": d, "B": b, "S": s, "start": st,
                   "workgroups": b * heads * -(-s // _core.attn_prefill_tiles()[0]), "flops": flops,
                   "us": {c: round(med[c], 2) for c in cols}, "spread": {c: round(spread[c], 3) for c in cols},
                   "a_TFLOPs": round(flops / med["a"] / 1e6, 1), "b_TFLOPs": round(flops / med["b"] / 1e6, 1),
                   "b_over_a": round(med["b"] / med["a"], 2), "c_over_a": round(med["c"] / med["a"], 2) if have_gqa else None,
                   "b2_over_a2": round(med["b'"] / med["a'"], 2), "a2_beats_b2_beyond_spread": bool(beats),
                   "a_vs_b_rel_err": rel, "reps": reps}
            rows.append(row)
            line = f"{model:11s} {b:2d} {s:5d} {st:5d} " + " ".join(f"{med[c]:10.1f} {spread[c]:5.2f}" for c in cols) + \
                (f" {row['a_TFLOPs']:7.1f} {row['b_TFLOPs']:7.1f} {row['b_over_a']:6.2f} "
                 f"{row['c_over_a'] if have_gqa else float('nan'):6.2f} {row['b2_over_a2']:6.2f}  {'yes' if beats else 'NO'}")
            lines.append(line)
            print(line, flush=True)
            del y, kc, vc, q_rot, q4, ya, yb, mask
            torch.cuda.empty_cache()
    out = {"rounds": args.rounds, "window_ms": args.window_ms, "tiles": list(_core.attn_prefill_tiles()),
           "sdpa_enable_gqa": have_gqa, "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
