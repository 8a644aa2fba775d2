#!/usr/bin/env python3
"""ops.mxfp4_linear (W4A16 from the packed layer in place) against the two other ways to
multiply by an MXFP4-packed weight, in one process and run (one MI355X).

Per shape (llama3-70b projections) and M in {1, 8, 16, 64}, three columns:

  (a) linear    ops.mxfp4_linear: reads the packed weight (17/64 of the bf16 bytes) once
  (b) unpack+mm ops.mxfp4_unpack_range into a bf16 buffer, then F.linear: what a packed store
                allows without this kernel (reads 17/64, writes 1, reads 1 of the bf16 bytes)
  (c) bf16 mm   F.linear on a bf16 weight unpacked beforehand: what --store bf16 buys, at 64/17
                of the HBM

The weight is the [out, in] parameter at element 8192 of a packed layer (64 MiB chunks). Every
call takes the next of a pool of distinct copies of the weight, and a pool is at least --pool-mib
large (default 768 MiB, three times the 256 MiB Infinity Cache), so no call finds its weight in
a cache. Rounds are interleaved over the columns; a round times --reps calls between two device
events. Printed: the median microseconds per call, the spread over the rounds, (a)'s packed
bytes per second, and the ratios (b)/(a) and (c)/(a).

    python scripts/mxfp4_linear_bench.py [--rounds 7] [--reps 20] [--out FILE]
"""

import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from distributed_llm_dissemination_amd import _core, ops  # noqa: E402

SHAPES = [("q_proj", 8192, 8192), ("k_proj", 1024, 8192), ("gate_proj", 28672, 8192), ("down_proj", 8192, 28672)]
MS = [1, 8, 16, 64]
CHUNK = 64 << 20
OFFSET = 8192  # a norm weight ahead of the parameter, as in a layer blob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pool-mib", type=int, default=768)
    ap.add_argument("--shapes", default="", help="comma-separated subset of " + ",".join(s[0] for s in SHAPES))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mxfp4_linear_bench needs a GPU")
    want = set(args.shapes.split(",")) if args.shapes else None
    pool_bytes = args.pool_mib << 20
    rows, lines = [], []
    head = (f"{'shape':10s} {'N':>6s} {'K':>6s} {'M':>3s} {'split':>5s} {'(a) us':>8s} {'sprd':>5s} {'(b) us':>8s} "
            f"{'(c) us':>8s} {'(a) GB/s':>9s} {'b/a':>6s} {'c/a':>6s}")
    lines.append(head)
    print(head, flush=True)
    for name, n, k in SHAPES:
        if want and name not in want:
            continue
        total = OFFSET + n * k
        src = 2 * total
        g = torch.Generator(device="cuda").manual_seed(n + k)
        layer = torch.empty(total, dtype=torch.bfloat16, device="cuda")
        layer[:OFFSET] = 1.0
        layer[OFFSET:] = (torch.randn(n * k, device="cuda", generator=g) / k ** 0.5).to(torch.bfloat16)
        packed0 = ops.mxfp4_pack_layer(layer, CHUNK)
        del layer
        wbytes = n * k * 17 // 32  # the parameter's codes and scales
        np_, nb = max(2, -(-pool_bytes // packed0.numel())), max(2, -(-pool_bytes // (2 * n * k)))
        packed = [packed0] + [packed0.clone() for _ in range(np_ - 1)]
        dense0 = ops.mxfp4_unpack_range(packed0, src, CHUNK, OFFSET, n * k).view(n, k)
        dense = [dense0] + [dense0.clone() for _ in range(nb - 1)]
        for m in MS:
            x = torch.randn(m, k, device="cuda", generator=g).to(torch.bfloat16)
            cnt = {"a": 0, "b": 0, "c": 0}

            def run_a():
                cnt["a"] += 1
                return ops.mxfp4_linear(x, packed[cnt["a"] % np_], n, k, src_bytes=src, chunk_bytes=CHUNK,
                                        elem_offset=OFFSET)

            def run_b():
                cnt["b"] += 1
                w = ops.mxfp4_unpack_range(packed[cnt["b"] % np_], src, CHUNK, OFFSET, n * k).view(n, k)
                return F.linear(x, w)

            def run_c():
                cnt["c"] += 1
                return F.linear(x, dense[cnt["c"] % nb])

            cases = {"a": run_a, "b": run_b, "c": run_c}
            ya, yc = run_a().float(), run_c().float()  # also the warm-up of every column
            run_b()
            for fn in cases.values():
                fn()
            torch.cuda.synchronize()
            rel = float((ya - yc).norm() / yc.norm())
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
            row = {"shape": name, "N": n, "K": k, "M": m, "split_k": _core.mxfp4_linear_slices(m, n, k),
                   "a_us": round(med["a"], 2), "b_us": round(med["b"], 2), "c_us": round(med["c"], 2),
                   "a_spread": round((max(times["a"]) - min(times["a"])) / med["a"], 3),
                   "a_packed_GBps": round(wbytes / med["a"] / 1e3, 1), "b_over_a": round(med["b"] / med["a"], 2),
                   "c_over_a": round(med["c"] / med["a"], 2), "a_vs_c_rel_err": rel,
                   "packed_copies": np_, "bf16_copies": nb}
            rows.append(row)
            line = (f"{name:10s} {n:6d} {k:6d} {m:3d} {row['split_k']:5d} {row['a_us']:8.2f} {row['a_spread']:5.2f} "
                    f"{row['b_us']:8.2f} {row['c_us']:8.2f} {row['a_packed_GBps']:9.1f} {row['b_over_a']:6.2f} "
                    f"{row['c_over_a']:6.2f}")
            lines.append(line)
            print(line, flush=True)
        del packed, dense, packed0, dense0
        torch.cuda.empty_cache()
    out = {"rounds": args.rounds, "reps": args.reps, "pool_MiB": args.pool_mib, "chunk_MiB": CHUNK >> 20,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
