#!/usr/bin/env python3
"""ops.attn_decode (grouped-query single-token attention, K and V read once per KV head) against
the ways plain torch attends one token to a KV cache, in one process and run (one MI355X).

Per model (llama3-70b: 64 heads, 8 KV heads, d 128; llama3-8b: 32 heads, 8 KV heads, d 128), batch
B in {1, 8, 64} and context in {1 k, 8 k, 32 k} (every sequence at the full context, the caches'
capacity), three columns:

  (a) attn_decode  ops.attn_decode(q, k_cache, v_cache, lens, max_len=context)
  (b) repeat+sdpa  the baseline, what decoder_forward does: repeat_interleave of cache[:, :, :len] by
                   heads // kv_heads, then F.scaled_dot_product_attention of the one-row query
  (c) sdpa gqa     F.scaled_dot_product_attention(..., enable_gqa=True) on cache[:, :, :len], where
                   this torch has it ("-" where it does not)

Every call takes the next of a pool of distinct (K, V) cache pairs, and a pool is at least
--pool-mib large (default 768 MiB, three times the 256 MiB Infinity Cache; never fewer than two
pairs), so no call finds its KV rows in a cache. Rounds are interleaved over the columns; a round
times `reps` calls between two device events, `reps` chosen per column so that a round lasts about
--window-ms. Printed: the median microseconds per call and the spread (max - min over the rounds,
relative to the median) of every column, (a)'s KV bytes per second (the K and V rows of the valid
prefix, once), the ratios (b)/(a) and (c)/(a), and whether (a) beats (b) by more than the larger of
the two columns' spreads.

    python scripts/attn_decode_bench.py [--rounds 7] [--window-ms 40] [--out FILE]
"""

import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from distributed_llm_dissemination_amd import _core, ops  # noqa: E402
from distributed_llm_dissemination_amd.models.weights import PRESETS  # noqa: E402

MODELS = ["llama3-70b", "llama3-8b"]
BATCHES = [1, 8, 64]
CONTEXTS = [1 << 10, 8 << 10, 32 << 10]


def gqa_sdpa_available():
    q = torch.zeros(1, 2, 1, 32, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(1, 1, 4, 32, dtype=torch.bfloat16, device="cuda")
    try:
        F.scaled_dot_product_attention(q, k, k, enable_gqa=True)
        return True
    except (TypeError, RuntimeError):
        return False


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--pool-mib", type=int, default=768)
    ap.add_argument("--models", default="", help="comma-separated subset of " + ",".join(MODELS))
    ap.add_argument("--batches", default="", help="comma-separated subset of " + ",".join(map(str, BATCHES)))
    ap.add_argument("--contexts", default="", help="comma-separated subset of " + ",".join(map(str, CONTEXTS)))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_decode_bench needs a GPU")
    models = args.models.split(",") if args.models else MODELS
    batches = [int(v) for v in args.batches.split(",")] if args.batches else BATCHES
    contexts = [int(v) for v in args.contexts.split(",")] if args.contexts else CONTEXTS
    have_gqa = gqa_sdpa_available()
    rows, lines = [], []
    head = (f"{'model':11s} {'B':>3s} {'ctx':>6s} {'pairs':>5s} {'(a) us':>9s} {'sprd':>5s} {'(b) us':>10s} {'sprd':>5s} "
            f"{'(c) us':>10s} {'sprd':>5s} {'(a) TB/s':>8s} {'b/a':>7s} {'c/a':>7s}  a beats b")
    lines.append(head)
    print(head, flush=True)
    for model in models:
        spec = PRESETS[model]
        heads, kvh, d = spec.heads, spec.kv_heads, spec.head_dim
        group = heads // kvh
        for b in batches:
            for ctx in contexts:
                g = torch.Generator(device="cuda").manual_seed(b + ctx)
                pair_bytes = 2 * b * kvh * ctx * d * 2
                pairs = max(2, -(-(args.pool_mib << 20) // pair_bytes))
                pool = []
                for _ in range(pairs):
                    kc = torch.empty(b, kvh, ctx, d, dtype=torch.bfloat16, device="cuda").normal_(generator=g)
                    vc = torch.empty(b, kvh, ctx, d, dtype=torch.bfloat16, device="cuda").normal_(generator=g)
                    pool.append((kc, vc))
                q = torch.randn(b, heads, d, device="cuda", generator=g).to(torch.bfloat16)
                q4 = q.view(b, heads, 1, d)
                lens = torch.full((b,), ctx, dtype=torch.int32, device="cuda")
                cnt = {"a": 0, "b": 0, "c": 0}

                def run_a():
                    cnt["a"] += 1
                    kc, vc = pool[cnt["a"] % pairs]
                    return ops.attn_decode(q, kc, vc, lens, max_len=ctx)

                def run_b():
                    cnt["b"] += 1
                    kc, vc = pool[cnt["b"] % pairs]
                    k = kc[:, :, :ctx].repeat_interleave(group, dim=1)
                    v = vc[:, :, :ctx].repeat_interleave(group, dim=1)
                    return F.scaled_dot_product_attention(q4, k, v)

                def run_c():
                    cnt["c"] += 1
                    kc, vc = pool[cnt["c"] % pairs]
                    return F.scaled_dot_product_attention(q4, kc[:, :, :ctx], vc[:, :, :ctx], enable_gqa=True)

                cases = {"a": run_a, "b": run_b}
                if have_gqa:
                    cases["c"] = run_c
                cnt["a"] = cnt["b"] = -1  # the same pair for the comparison
                ya, yb = run_a().float().view(b, heads, d), run_b().float().view(b, heads, d)
                rel = float((ya - yb).norm() / yb.norm())
                reps = {}
                for c, fn in cases.items():  # warm-up of every column, and its reps from a first timing
                    fn()
                    torch.cuda.synchronize()
                    reps[c] = max(3, min(200, int(args.window_ms * 1e3 / max(timed(fn, 3), 1.0))))
                times = {c: [] for c in cases}
                for _ in range(args.rounds):
                    for c, fn in cases.items():
                        times[c].append(timed(fn, reps[c]))
                med = {c: statistics.median(t) for c, t in times.items()}
                spread = {c: max(t) - min(t) for c, t in times.items()}
                kv_bytes = 2 * b * kvh * ctx * d * 2
                beats = med["b"] - med["a"] > max(spread["a"], spread["b"])
                row = {"model": model, "heads": heads, "kv_heads": kvh, "d": d, "B": b, "context": ctx, "pairs": pairs,
                       "pool_MiB": round(pairs * pair_bytes / 2 ** 20, 1),
                       "workgroups": b * kvh * -(-ctx // _core.attn_decode_chunk()),
                       "a_us": round(med["a"], 2), "a_spread": round(spread["a"] / med["a"], 3),
                       "b_us": round(med["b"], 2), "b_spread": round(spread["b"] / med["b"], 3),
                       "c_us": round(med["c"], 2) if have_gqa else None,
                       "c_spread": round(spread["c"] / med["c"], 3) if have_gqa else None,
                       "a_kv_TBps": round(kv_bytes / med["a"] / 1e6, 3), "b_over_a": round(med["b"] / med["a"], 2),
                       "c_over_a": round(med["c"] / med["a"], 2) if have_gqa else None,
                       "a_beats_b_beyond_spread": bool(beats), "a_vs_b_rel_err": rel, "reps": reps}
                rows.append(row)
                cs = (f"{row['c_us']:10.2f} {row['c_spread']:5.2f}" if have_gqa else f"{'-':>10s} {'-':>5s}")
                ca = f"{row['c_over_a']:7.2f}" if have_gqa else f"{'-':>7s}"
                line = (f"{model:11s} {b:3d} {ctx:6d} {pairs:5d} {row['a_us']:9.2f} {row['a_spread']:5.2f} "
                        f"{row['b_us']:10.2f} {row['b_spread']:5.2f} {cs} {row['a_kv_TBps']:8.3f} "
                        f"{row['b_over_a']:7.2f} {ca}  {'yes' if beats else 'NO'}")
                lines.append(line)
                print(line, flush=True)
                del pool, q, q4, ya, yb
                torch.cuda.empty_cache()
    out = {"rounds": args.rounds, "window_ms": args.window_ms, "pool_MiB": args.pool_mib,
           "chunk": _core.attn_decode_chunk(), "sdpa_enable_gqa": have_gqa, "torch": torch.__version__,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
