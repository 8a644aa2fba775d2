#!/usr/bin/env python3
"""W4A8 on the block-scaled MFMA (ops.mxfp4_linear / ops.mxfp4_swiglu with act="mxfp8") against
the W4A16 many-row kernel and the library GEMM, in one process and run (one MI355X).

Per shape (llama3-70b q_proj, merged q/k/v of N = 10240, gate_proj, down_proj and the fused
gate/up SwiGLU) and M in {128, 256, 512, 2048}, four columns:

  (a)  act="mxfp8" end to end: ops.mxfp8_quantize_rows, then the native kernel (two launches)
  (a') the native kernel alone on x quantized beforehand (_core.mxfp4_linear_mx / _swiglu_mx)
  (p)  the same op with tiled=True: W4A16 on the bf16 MFMA, the baseline
  (c)  F.linear on a bf16 weight unpacked beforehand (for gate/up: both, then F.silu(g) * u)

The weight is the [out, in] parameter at element 8192 of a packed layer (64 MiB chunks; for
gate/up two parameters one behind the other). Every call takes the next of a pool of distinct
copies, and a pool is at least --pool-mib large (default 768 MiB, three times the 256 MiB Infinity
Cache), so no call finds its weight in a cache from the call before. Rounds are interleaved over
the columns; a round times --reps calls between two device events. Printed: the median
microseconds per call and the spread (max - min over the rounds, relative to the median) of (a)
and (p), the quantizer's own time (a fifth column of the same rounds), (a')'s TFLOP/s, the
ratios (a)/(p) and (a)/(c), and `a<p`: whether (a) beats (p) by more than the larger of the two
spreads. Accuracy, on x ~ N(0, 1) and W ~ N(0, 1/K): the relative error (Frobenius) of (a) and of
(p) against a float64 product of the UNQUANTIZED x with the dequantized weight, over the first
--err-rows rows and --err-cols columns.

    python scripts/mxfp4_mx_bench.py [--rounds 7] [--reps 10] [--out FILE]
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
MS = [128, 256, 512, 2048]
CHUNK = 64 << 20
OFFSET = 8192  # a norm weight ahead of the parameter, as in a layer blob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pool-mib", type=int, default=768)
    ap.add_argument("--err-rows", type=int, default=128)
    ap.add_argument("--err-cols", type=int, default=512)
    ap.add_argument("--shapes", default="", help="comma-separated subset of " + ",".join(s[0] for s in SHAPES))
    ap.add_argument("--ms", default="", help="comma-separated subset of the row counts")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mxfp4_mx_bench needs a GPU")
    want = set(args.shapes.split(",")) if args.shapes else None
    ms = [int(v) for v in args.ms.split(",")] if args.ms else MS
    pool_bytes = args.pool_mib << 20
    bm, bn = _core.mxfp4_mx_tile()
    rows, lines = [], []
    head = (f"{'shape':10s} {'N':>6s} {'K':>6s} {'M':>5s} {'(a) us':>9s} {'sprd':>5s} {'(a`) us':>9s} {'quant us':>9s} "
            f"{'(p) us':>9s} {'sprd':>5s} {'(c) us':>9s} {'(a`) TF/s':>9s} {'a/p':>6s} {'a/c':>6s} {'a<p':>4s} "
            f"{'err (a)':>9s} {'err (p)':>9s}")
    lines.append(f"tile BM x BN = {bm} x {bn}")
    lines.append(head)
    print(lines[0], flush=True)
    print(head, flush=True)
    stream = torch.cuda.current_stream().cuda_stream
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
        packed0 = ops.mxfp4_pack_layer(layer, CHUNK)
        del layer
        np_, nb = max(2, -(-pool_bytes // packed0.numel())), max(2, -(-pool_bytes // (2 * nw * n * k)))
        packed = [packed0] + [packed0.clone() for _ in range(np_ - 1)]
        dense0 = ops.mxfp4_unpack_range(packed0, src, CHUNK, OFFSET, nw * n * k).view(nw * n, k)
        dense = [dense0] + [dense0.clone() for _ in range(nb - 1)]
        kw = dict(src_bytes=src, chunk_bytes=CHUNK)

        def packed_op(x, p, **how):
            if gated:
                return ops.mxfp4_swiglu(x, p, n, k, gate_offset=OFFSET, up_offset=OFFSET + n * k, **how, **kw)
            return ops.mxfp4_linear(x, p, n, k, elem_offset=OFFSET, **how, **kw)

        def dense_op(x, w):
            if gated:
                return F.silu(F.linear(x, w[:n])) * F.linear(x, w[n:])
            return F.linear(x, w)

        for m in ms:
            x = torch.randn(m, k, device="cuda", generator=g).to(torch.bfloat16)
            xq, xs = ops.mxfp8_quantize_rows(x)
            y = torch.empty(m, n, dtype=torch.bfloat16, device="cuda")
            cnt = {"a": 0, "a1": 0, "p": 0, "c": 0}

            def run_a():
                cnt["a"] += 1
                return packed_op(x, packed[cnt["a"] % np_], act="mxfp8")

            def run_a1():
                cnt["a1"] += 1
                p = packed[cnt["a1"] % np_]
                if gated:
                    _core.mxfp4_swiglu_mx(p.data_ptr(), src, CHUNK, OFFSET, OFFSET + n * k, xq.data_ptr(), xs.data_ptr(), m,
                                          n, k, y.data_ptr(), n, True, stream)
                else:
                    _core.mxfp4_linear_mx(p.data_ptr(), src, CHUNK, OFFSET, xq.data_ptr(), xs.data_ptr(), m, n, k,
                                          y.data_ptr(), n, True, stream)
                return y

            def run_q():
                return ops.mxfp8_quantize_rows(x)

            def run_p():
                cnt["p"] += 1
                return packed_op(x, packed[cnt["p"] % np_], tiled=True)

            def run_c():
                cnt["c"] += 1
                return dense_op(x, dense[cnt["c"] % nb])

            cases = {"a": run_a, "a1": run_a1, "q": run_q, "p": run_p, "c": run_c}
            # accuracy against float64 of the unquantized x, on a corner of the result
            er, ec = min(m, args.err_rows), min(n, args.err_cols)
            wd = dense0.double()
            x64 = x[:er].double()
            if gated:
                g64, u64 = x64 @ wd[:ec].T, x64 @ wd[n:n + ec].T
                ref = g64 / (1 + torch.exp(-g64)) * u64
            else:
                ref = x64 @ wd[:ec].T
            del wd
            err = {c: float((cases[c]()[:er, :ec].double() - ref).norm() / ref.norm()) for c in ("a", "p")}
            assert torch.equal(run_a(), run_a1())  # the two ways to the native kernel agree
            for fn in cases.values():  # the warm-up of every column
                fn()
            torch.cuda.synchronize()
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
            tf = 2.0 * nw * m * n * k / med["a1"] / 1e6
            wins = med["a"] < med["p"] * (1 - max(spread["a"], spread["p"]))
            row = {"shape": name, "N": n, "K": k, "M": m, "a_us": round(med["a"], 2), "a1_us": round(med["a1"], 2),
                   "quant_us": round(med["q"], 2), "p_us": round(med["p"], 2), "c_us": round(med["c"], 2),
                   "a_spread": round(spread["a"], 3), "a1_spread": round(spread["a1"], 3),
                   "p_spread": round(spread["p"], 3), "c_spread": round(spread["c"], 3), "a1_TFLOPs": round(tf, 1),
                   "a_over_p": round(med["a"] / med["p"], 3), "a_over_c": round(med["a"] / med["c"], 3),
                   "a_beats_p_beyond_spread": bool(wins), "a_rel_err_vs_f64": err["a"], "p_rel_err_vs_f64": err["p"],
                   "packed_copies": np_, "bf16_copies": nb}
            rows.append(row)
            line = (f"{name:10s} {n:6d} {k:6d} {m:5d} {row['a_us']:9.2f} {row['a_spread']:5.2f} {row['a1_us']:9.2f} "
                    f"{row['quant_us']:9.2f} {row['p_us']:9.2f} {row['p_spread']:5.2f} {row['c_us']:9.2f} "
                    f"{row['a1_TFLOPs']:9.1f} {row['a_over_p']:6.2f} {row['a_over_c']:6.2f} {'yes' if wins else 'no':>4s} "
                    f"{err['a']:9.2e} {err['p']:9.2e}")
            lines.append(line)
            print(line, flush=True)
        del packed, dense, packed0, dense0
        torch.cuda.empty_cache()
    out = {"rounds": args.rounds, "reps": args.reps, "pool_MiB": args.pool_mib, "chunk_MiB": CHUNK >> 20,
           "tile": [bm, bn], "device": torch.cuda.get_device_name(0), "rows": rows}
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
