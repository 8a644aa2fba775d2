#!/usr/bin/env python3
"""The many-row fp8 and MXFP6 kernels (ops.fp8_linear / ops.fp8_swiglu / ops.mxfp6_linear /
ops.mxfp6_swiglu with tiled=True) against the other ways to multiply many rows by such a packed
weight, in one process and run (one MI355X). scripts/mxfp4_tiled_bench.py is the MXFP4 twin.

Per format (MXFP6, fp8 with scale block 128, fp8 with scale block 32), shape (llama3-70b q_proj,
the merged q/k/v of N = 10240, gate_proj, down_proj, and the fused gate/up SwiGLU) and M in
{64, 128, 256, 512, 2048}, five columns:

  (a) tiled     tiled=True: one launch, W read and dequantized once per BM rows of x
  (p) untiled   tiled=False, the same op: one launch per 64 rows, W read once per launch. This is
                the baseline: code this kernel family does not touch, timed in the same process
  (b) unpack+mm ops.*_unpack_range into a bf16 buffer, then F.linear (for gate/up: both weights,
                then F.silu(g) * u): what a packed store allows without these kernels
  (c) bf16 mm   F.linear on a bf16 weight unpacked beforehand: what --store bf16 buys
  (d) mxfp4     ops.mxfp4_linear / ops.mxfp4_swiglu with tiled=True on the same shape, the weights
                packed as MXFP4: the same design at 17/64 of the bytes

The weight is the [out, in] parameter at element 8192 of a packed layer (64 MiB chunks; for
gate/up two parameters one behind the other). Every call takes the next of a pool of distinct
copies, and a pool is at least --pool-mib large (default 768 MiB, three times the 256 MiB Infinity
Cache), so no call finds its weight in a cache from the call before. Rounds are interleaved over
the columns; a round times --reps calls between two device events. Printed: the median
microseconds per call and the spread (max - min over the rounds, relative to the median) of (a)
and (p), (a)'s TFLOP/s and its share of the 2.5 PFLOP/s bf16 dense peak, and the ratios (p)/(a),
(b)/(a), (c)/(a), (d)/(a). `a<p` says whether (a) beats (p) by more than the larger of the two
spreads.

    python scripts/packed_tiled_bench.py [--rounds 7] [--reps 10] [--formats mxfp6,fp8b128,fp8b32] [--out FILE]
"""

import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from distributed_llm_dissemination_amd import _core, ops  # noqa: E402

# (name, N, K, gated)
SHAPES = [("q_proj", 8192, 8192, False), ("qkv", 10240, 8192, False), ("gate_proj", 28672, 8192, False),
          ("down_proj", 8192, 28672, False), ("gate_up", 28672, 8192, True)]
MS = [64, 128, 256, 512, 2048]
FORMATS = {"mxfp6": ("mxfp6", 32), "fp8b128": ("fp8", 128), "fp8b32": ("fp8", 32)}
CHUNK = 64 << 20
OFFSET = 8192  # a norm weight ahead of the parameter, as in a layer blob
PEAK_TFLOPS = 2500.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pool-mib", type=int, default=768)
    ap.add_argument("--formats", default="", help="comma-separated subset of " + ",".join(FORMATS))
    ap.add_argument("--shapes", default="", help="comma-separated subset of " + ",".join(s[0] for s in SHAPES))
    ap.add_argument("--ms", default="", help="comma-separated subset of the row counts")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("packed_tiled_bench needs a GPU")
    fmts = args.formats.split(",") if args.formats else list(FORMATS)
    want = set(args.shapes.split(",")) if args.shapes else None
    ms = [int(v) for v in args.ms.split(",")] if args.ms else MS
    pool_bytes = args.pool_mib << 20
    tiles = {"mxfp6": _core.mxfp6_tiled_tile(), "fp8": _core.fp8_tiled_tile(), "mxfp4": _core.mxfp4_tiled_tile()}
    rows, lines = [], []
    head = (f"{'format':8s} {'shape':10s} {'N':>6s} {'K':>6s} {'M':>5s} {'(a) us':>9s} {'sprd':>5s} {'(p) us':>9s} "
            f"{'sprd':>5s} {'(b) us':>9s} {'(c) us':>9s} {'(d) us':>9s} {'(a) TF/s':>9s} {'peak':>5s} {'p/a':>6s} "
            f"{'b/a':>6s} {'c/a':>6s} {'d/a':>6s} {'a<p':>4s}")
    lines.append("tile BM x BN: " + ", ".join(f"{k} {v[0]} x {v[1]}" for k, v in tiles.items()))
    lines.append(head)
    print(lines[0], flush=True)
    print(head, flush=True)
    for fid in fmts:
        fmt, block = FORMATS[fid]
        for name, n, k, gated in SHAPES:
            if want and name not in want:
                continue
            nw = 2 if gated else 1
            total = OFFSET + nw * n * k
            src = 2 * total
            g = torch.Generator(device="cuda").manual_seed(n + k)
            layer = torch.empty(total, dtype=torch.bfloat16, device="cuda")
            layer[:OFFSET] = 1.0
            layer[OFFSET:] = (torch.randn(nw * n * k, device="cuda", generator=g) / k ** 0.5).to(torch.bfloat16)
            kw = dict(src_bytes=src, chunk_bytes=CHUNK)
            if fmt == "fp8":
                packed0 = ops.fp8_pack_layer(layer, CHUNK, block)
                fkw = dict(kw, block=block)
                lin, glu = ops.fp8_linear, ops.fp8_swiglu

                def unpack(p):
                    return ops.fp8_unpack_range(p, src, CHUNK, OFFSET, nw * n * k, block).view(nw * n, k)
            else:
                packed0 = ops.mxfp6_pack_layer(layer, CHUNK)
                fkw = kw
                lin, glu = ops.mxfp6_linear, ops.mxfp6_swiglu

                def unpack(p):
                    return ops.mxfp6_unpack_range(p, src, CHUNK, OFFSET, nw * n * k).view(nw * n, k)
            packed40 = ops.mxfp4_pack_layer(layer, CHUNK)
            del layer
            np_, nb = max(2, -(-pool_bytes // packed0.numel())), max(2, -(-pool_bytes // (2 * nw * n * k)))
            np4 = max(2, -(-pool_bytes // packed40.numel()))
            packed = [packed0] + [packed0.clone() for _ in range(np_ - 1)]
            packed4 = [packed40] + [packed40.clone() for _ in range(np4 - 1)]
            dense0 = unpack(packed0)
            dense = [dense0] + [dense0.clone() for _ in range(nb - 1)]

            def packed_op(x, p, tiled):
                if gated:
                    return glu(x, p, n, k, gate_offset=OFFSET, up_offset=OFFSET + n * k, tiled=tiled, **fkw)
                return lin(x, p, n, k, elem_offset=OFFSET, tiled=tiled, **fkw)

            def mxfp4_op(x, p):
                if gated:
                    return ops.mxfp4_swiglu(x, p, n, k, gate_offset=OFFSET, up_offset=OFFSET + n * k, tiled=True, **kw)
                return ops.mxfp4_linear(x, p, n, k, elem_offset=OFFSET, tiled=True, **kw)

            def dense_op(x, w):
                if gated:
                    return F.silu(F.linear(x, w[:n])) * F.linear(x, w[n:])
                return F.linear(x, w)

            for m in ms:
                x = torch.randn(m, k, device="cuda", generator=g).to(torch.bfloat16)
                cnt = {"a": 0, "p": 0, "b": 0, "c": 0, "d": 0}

                def run_a():
                    cnt["a"] += 1
                    return packed_op(x, packed[cnt["a"] % np_], True)

                def run_p():
                    cnt["p"] += 1
                    return packed_op(x, packed[cnt["p"] % np_], False)

                def run_b():
                    cnt["b"] += 1
                    return dense_op(x, unpack(packed[cnt["b"] % np_]))

                def run_c():
                    cnt["c"] += 1
                    return dense_op(x, dense[cnt["c"] % nb])

                def run_d():
                    cnt["d"] += 1
                    return mxfp4_op(x, packed4[cnt["d"] % np4])

                cases = {"a": run_a, "p": run_p, "b": run_b, "c": run_c, "d": run_d}
                ya, yc = run_a().float(), run_c().float()  # also the warm-up of every column
                for fn in cases.values():
                    fn()
                torch.cuda.synchronize()
                rel = float((ya - yc).norm() / yc.norm())
                del ya, yc
                times = {c: [] for c in cases}
                for _ in range(args.rounds):
                    for c, fn in cases.items():
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        for _ in range(args.reps):
                            fn()
                        e.record()
                        torch.cuda.synchronize()
                        times[c].append(s.elapsed_time(e) * 1e3 / args.reps)
                med = {c: statistics.median(t) for c, t in times.items()}
                spread = {c: (max(t) - min(t)) / med[c] for c, t in times.items()}
                tf = 2.0 * nw * m * n * k / med["a"] / 1e6
                wins = med["a"] < med["p"] * (1 - max(spread["a"], spread["p"]))
                row = {"format": fid, "shape": name, "N": n, "K": k, "M": m, "a_us": round(med["a"], 2),
                       "p_us": round(med["p"], 2), "b_us": round(med["b"], 2), "c_us": round(med["c"], 2),
                       "d_us": round(med["d"], 2), "a_spread": round(spread["a"], 3), "p_spread": round(spread["p"], 3),
                       "a_TFLOPs": round(tf, 1), "a_of_peak": round(tf / PEAK_TFLOPS, 3),
                       "p_over_a": round(med["p"] / med["a"], 2), "b_over_a": round(med["b"] / med["a"], 2),
                       "c_over_a": round(med["c"] / med["a"], 2), "d_over_a": round(med["d"] / med["a"], 2),
                       "a_beats_p_beyond_spread": bool(wins), "a_vs_c_rel_err": rel, "packed_copies": np_,
                       "bf16_copies": nb, "mxfp4_copies": np4}
                rows.append(row)
                line = (f"{fid:8s} {name:10s} {n:6d} {k:6d} {m:5d} {row['a_us']:9.2f} {row['a_spread']:5.2f} "
                        f"{row['p_us']:9.2f} {row['p_spread']:5.2f} {row['b_us']:9.2f} {row['c_us']:9.2f} "
                        f"{row['d_us']:9.2f} {row['a_TFLOPs']:9.1f} {row['a_of_peak']:5.2f} {row['p_over_a']:6.2f} "
                        f"{row['b_over_a']:6.2f} {row['c_over_a']:6.2f} {row['d_over_a']:6.2f} "
                        f"{'yes' if wins else 'no':>4s}")
                lines.append(line)
                print(line, flush=True)
            del packed, packed4, dense, packed0, packed40, dense0
            torch.cuda.empty_cache()
    out = {"rounds": args.rounds, "reps": args.reps, "pool_MiB": args.pool_mib, "chunk_MiB": CHUNK >> 20,
           "tiles": {k: list(v) for k, v in tiles.items()}, "device": torch.cuda.get_device_name(0), "rows": rows}
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
