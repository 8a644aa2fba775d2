#!/usr/bin/env python3
"""ops.fp8_linear (W8A16 from the fp8-packed layer in place) against the other ways to multiply
by an fp8-packed weight, in one process and run (one MI355X).

Per shape (llama3-70b projections), scale block (128, 32) and M in {1, 8, 16, 64}, four columns:

  (a) linear    ops.fp8_linear: reads the packed weight (33/64 of the bf16 bytes at block 128,
                36/64 at block 32) once
  (b) unpack+mm ops.fp8_unpack_range into a bf16 buffer, then F.linear: what a packed store
                allows without this kernel (reads the packed bytes, writes and reads the bf16 ones)
  (c) bf16 mm   F.linear on a bf16 weight unpacked beforehand: what --store bf16 buys, at about
                twice the HBM
  (d) mxfp4     ops.mxfp4_linear on the same weight MXFP4-packed (17/64 of the bf16 bytes), as
                context: the other packed format

The weight is the [out, in] parameter at element 8192 of a packed layer (64 MiB chunks). Every
call takes the next of a pool of distinct copies of the weight, and a pool is at least --pool-mib
large (default 768 MiB, three times the 256 MiB Infinity Cache), so no call finds its weight in
a cache. Rounds are interleaved over the columns; a round times --reps calls between two device
events. Printed: the median microseconds per call, the spread over the rounds of (a) and (b),
(a)'s packed bytes per second, and the ratios (b)/(a), (c)/(a) and (d)/(a).

    python scripts/fp8_linear_bench.py [--rounds 7] [--reps 20] [--ms 1,8,16,64] [--blocks 128,32] [--out FILE]

--sweep prints, instead, (a) for every forced split_k and row_tiles at block 128 (the data behind
the launcher's choices in csrc/kernels/fp8_linear.hip).
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
BLOCKS = [128, 32]
CHUNK = 64 << 20
OFFSET = 8192  # a norm weight ahead of the parameter, as in a layer blob


def timed(cases, rounds, reps):
    """Interleaved rounds: {name: [us per call, one per round]}."""
    times = {c: [] for c in cases}
    for _ in range(rounds):
        for c, fn in cases.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[c].append(s.elapsed_time(e) * 1e3 / reps)
    return times


def spread(t):
    return (max(t) - min(t)) / statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pool-mib", type=int, default=768)
    ap.add_argument("--shapes", default="", help="comma-separated subset of " + ",".join(s[0] for s in SHAPES))
    ap.add_argument("--ms", default="", help="comma-separated rows of x instead of " + ",".join(map(str, MS)))
    ap.add_argument("--blocks", default="", help="comma-separated scale blocks instead of " + ",".join(map(str, BLOCKS)))
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_linear_bench needs a GPU")
    want = set(args.shapes.split(",")) if args.shapes else None
    ms = [int(v) for v in args.ms.split(",")] if args.ms else MS
    blocks = [int(v) for v in args.blocks.split(",")] if args.blocks else ([128] if args.sweep else BLOCKS)
    pool_bytes = args.pool_mib << 20
    rows, lines = [], []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    if args.sweep:
        emit(f"{'shape':10s} {'blk':>3s} {'M':>3s} {'tiles':>5s} {'split':>5s} {'us':>8s} {'sprd':>5s} {'GB/s':>7s}"
             "   (* = the launcher's choice of split at that number of row tiles)")
    else:
        emit(f"{'shape':10s} {'N':>6s} {'K':>6s} {'blk':>3s} {'M':>3s} {'split':>5s} {'(a) us':>8s} {'sprd':>5s} "
             f"{'(b) us':>8s} {'sprd':>5s} {'(c) us':>8s} {'(d) us':>8s} {'(a) GB/s':>9s} {'b/a':>6s} {'c/a':>6s} {'d/a':>6s}")
    for name, n, k in SHAPES:
        if want and name not in want:
            continue
        total = OFFSET + n * k
        src = 2 * total
        g = torch.Generator(device="cuda").manual_seed(n + k)
        layer = torch.empty(total, dtype=torch.bfloat16, device="cuda")
        layer[:OFFSET] = 1.0
        layer[OFFSET:] = (torch.randn(n * k, device="cuda", generator=g) / k ** 0.5).to(torch.bfloat16)
        xs = {m: torch.randn(m, k, device="cuda", generator=g).to(torch.bfloat16) for m in ms}
        p4 = ops.mxfp4_pack_layer(layer, CHUNK)
        n4 = max(2, -(-pool_bytes // p4.numel()))
        for block in blocks:
            packed0 = ops.fp8_pack_layer(layer, CHUNK, block)
            wbytes = n * k + n * k // block * 4  # the parameter's codes and scales
            np_, nb = max(2, -(-pool_bytes // packed0.numel())), max(2, -(-pool_bytes // (2 * n * k)))
            packed = [packed0] + [packed0.clone() for _ in range(np_ - 1)]
            kw = dict(src_bytes=src, chunk_bytes=CHUNK, block=block, elem_offset=OFFSET)
            if args.sweep:
                for m in ms:
                    x, cnt = xs[m], {"a": 0}

                    def run_a(sk, rt):
                        cnt["a"] += 1
                        return ops.fp8_linear(x, packed[cnt["a"] % np_], n, k, split_k=sk, row_tiles=rt, **kw)

                    chosen = _core.fp8_linear_slices(m, n, k)
                    cases = {(rt, sk): (lambda rt=rt, sk=sk: run_a(sk, rt)) for rt in (1, 2, 4) for sk in (1, 2, 4, 8, 16)
                             if not (rt == 4 and m > 32)}
                    for fn in cases.values():
                        fn()
                    torch.cuda.synchronize()
                    times = timed(cases, args.rounds, args.reps)
                    for (rt, sk), t in times.items():
                        med = statistics.median(t)
                        rows.append({"shape": name, "block": block, "M": m, "row_tiles": rt, "split_k": sk,
                                     "us": round(med, 2), "spread": round(spread(t), 3),
                                     "packed_GBps": round(wbytes / med / 1e3, 1), "auto_split_k": chosen})
                        emit(f"{name:10s} {block:3d} {m:3d} {rt:5d} {sk:5d} {med:8.2f} {spread(t):5.2f} "
                             f"{wbytes / med / 1e3:7.1f}{' *' if sk == chosen else ''}")
                del packed, packed0
                torch.cuda.empty_cache()
                continue
            dense0 = ops.fp8_unpack_range(packed0, src, CHUNK, OFFSET, n * k, block).view(n, k)
            dense = [dense0] + [dense0.clone() for _ in range(nb - 1)]
            pool4 = [p4] + [p4.clone() for _ in range(n4 - 1)]
            for m in ms:
                x = xs[m]
                cnt = {"a": 0, "b": 0, "c": 0, "d": 0}

                def run_a():
                    cnt["a"] += 1
                    return ops.fp8_linear(x, packed[cnt["a"] % np_], n, k, **kw)

                def run_b():
                    cnt["b"] += 1
                    w = ops.fp8_unpack_range(packed[cnt["b"] % np_], src, CHUNK, OFFSET, n * k, block).view(n, k)
                    return F.linear(x, w)

                def run_c():
                    cnt["c"] += 1
                    return F.linear(x, dense[cnt["c"] % nb])

                def run_d():
                    cnt["d"] += 1
                    return ops.mxfp4_linear(x, pool4[cnt["d"] % n4], n, k, src_bytes=src, chunk_bytes=CHUNK,
                                            elem_offset=OFFSET)

                cases = {"a": run_a, "b": run_b, "c": run_c, "d": run_d}
                ya, yc = run_a().float(), run_c().float()  # also the warm-up of every column
                run_b(), run_d()
                for fn in cases.values():
                    fn()
                torch.cuda.synchronize()
                rel = float((ya - yc).norm() / yc.norm())
                times = timed(cases, args.rounds, args.reps)
                med = {c: statistics.median(t) for c, t in times.items()}
                row = {"shape": name, "N": n, "K": k, "block": block, "M": m, "split_k": _core.fp8_linear_slices(m, n, k),
                       "a_us": round(med["a"], 2), "b_us": round(med["b"], 2), "c_us": round(med["c"], 2),
                       "d_us": round(med["d"], 2), "a_spread": round(spread(times["a"]), 3),
                       "b_spread": round(spread(times["b"]), 3), "a_packed_GBps": round(wbytes / med["a"] / 1e3, 1),
                       "b_over_a": round(med["b"] / med["a"], 2), "c_over_a": round(med["c"] / med["a"], 2),
                       "d_over_a": round(med["d"] / med["a"], 2), "a_vs_c_rel_err": rel,
                       "a_min_us": round(min(times["a"]), 2), "a_max_us": round(max(times["a"]), 2),
                       "b_min_us": round(min(times["b"]), 2), "b_max_us": round(max(times["b"]), 2),
                       "packed_copies": np_, "bf16_copies": nb, "mxfp4_copies": n4}
                rows.append(row)
                emit(f"{name:10s} {n:6d} {k:6d} {block:3d} {m:3d} {row['split_k']:5d} {row['a_us']:8.2f} "
                     f"{row['a_spread']:5.2f} {row['b_us']:8.2f} {row['b_spread']:5.2f} {row['c_us']:8.2f} "
                     f"{row['d_us']:8.2f} {row['a_packed_GBps']:9.1f} {row['b_over_a']:6.2f} {row['c_over_a']:6.2f} "
                     f"{row['d_over_a']:6.2f}")
            del packed, dense, packed0, dense0, pool4
            torch.cuda.empty_cache()
        del layer, p4
        torch.cuda.empty_cache()
    out = {"rounds": args.rounds, "reps": args.reps, "pool_MiB": args.pool_mib, "chunk_MiB": CHUNK >> 20,
           "sweep": args.sweep, "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
