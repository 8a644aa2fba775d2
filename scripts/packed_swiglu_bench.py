#!/usr/bin/env python3
"""The fused gated MLP of an fp8- or MXFP6-packed decoder layer against the per-projection route,
in one process and run (one MI355X).

gate/up of llama3-70b (28672 x 8192) and llama3-8b (14336 x 4096), M in {1, 8, 16, 64}, per format
(--fmt mxfp6,fp8; fp8 once per scale block of --block, default 128,32):

  (a) swiglu    ops.mxfp6_swiglu / ops.fp8_swiglu: one launch, x read once, g and u never leave the
                accumulators
  (b) 2 linear  two ops.mxfp6_linear / ops.fp8_linear (bf16) and F.silu(g) * u: two launches, two
                elementwise launches, g, u and the product through HBM

The parameters lie one behind the other at element 8192 of a packed layer (64 MiB chunks), as in
a layer blob. Every call takes the next of a pool of distinct copies of the layer, and a pool is
at least --pool-mib large (default 768 MiB, three times the 256 MiB Infinity Cache), so no call
finds its weights in a cache. Rounds are interleaved over the columns; a round times --reps calls
between two device events. Printed: the median microseconds per call, the spread of (a) and (b)
over the rounds ((max - min) / median), (a)'s packed bytes per second, (b)/(a), and whether the row
is a win: (b)/(a) exceeds 1 by more than the larger of the two spreads.

    python scripts/packed_swiglu_bench.py [--fmt mxfp6,fp8] [--block 128,32] [--rounds 7] [--reps 20]
                                          [--ms 1,8,16,64] [--out FILE]

--sweep prints, instead, (a) for every forced split_k and row_tiles (the data behind the
launchers' choices in csrc/kernels/mxfp6_swiglu.hip and fp8_swiglu.hip).
"""

import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from distributed_llm_dissemination_amd import _core, ops  # noqa: E402

MLP = [("70b gate/up", 28672, 8192), ("8b gate/up", 14336, 4096)]
MS = [1, 8, 16, 64]
CHUNK = 64 << 20
OFFSET = 8192  # a norm weight ahead of the parameters, as in a layer blob


class Format:
    """One packed format: its pack, linear, fused op and launcher rule behind one signature."""

    def __init__(self, name, block):
        self.name, self.block = name, block
        self.label = "mxfp6" if name == "mxfp6" else f"fp8 b{block}"
        self.kw = dict(block=block) if name == "fp8" else {}

    def pack_layer(self, layer):
        if self.name == "fp8":
            return ops.fp8_pack_layer(layer, CHUNK, self.block)
        return ops.mxfp6_pack_layer(layer, CHUNK)

    def packed_bytes(self, elems):
        return elems * 25 // 32 if self.name == "mxfp6" else elems + 4 * elems // self.block

    def swiglu(self, *a, **kw):
        return (ops.fp8_swiglu if self.name == "fp8" else ops.mxfp6_swiglu)(*a, **self.kw, **kw)

    def linear(self, *a, **kw):
        return (ops.fp8_linear if self.name == "fp8" else ops.mxfp6_linear)(*a, **self.kw, **kw)

    def slices(self, m, n, k):
        return (_core.fp8_swiglu_slices if self.name == "fp8" else _core.mxfp6_swiglu_slices)(m, n, k)


def packed_pool(fmt, rows, k, pool_bytes, seed):
    """(copies of the packed layer [norm weight, `rows` x k weights], its source bytes)."""
    total = OFFSET + rows * k
    g = torch.Generator(device="cuda").manual_seed(seed)
    layer = torch.empty(total, dtype=torch.bfloat16, device="cuda")
    layer[:OFFSET] = 1.0
    layer[OFFSET:] = (torch.randn(rows * k, device="cuda", generator=g) / k ** 0.5).to(torch.bfloat16)
    p0 = fmt.pack_layer(layer)
    del layer
    n = max(2, -(-pool_bytes // p0.numel()))
    return [p0] + [p0.clone() for _ in range(n - 1)], 2 * total


def timed(cases, rounds, reps):
    for fn in cases.values():  # warm-up of every column
        fn()
        fn()
    torch.cuda.synchronize()
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
    return {c: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for c, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fmt", default="mxfp6,fp8", help="comma-separated formats: mxfp6, fp8")
    ap.add_argument("--block", default="128,32", help="comma-separated fp8 scale blocks")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pool-mib", type=int, default=768)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--ms", default="", help="comma-separated rows of x instead of " + ",".join(map(str, MS)))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("packed_swiglu_bench needs a GPU")
    fmts = []
    for name in args.fmt.split(","):
        if name not in ("mxfp6", "fp8"):
            sys.exit(f"--fmt: 'mxfp6' or 'fp8', not {name!r}")
        fmts += [Format(name, int(b)) for b in args.block.split(",")] if name == "fp8" else [Format(name, 32)]
    pool_bytes = args.pool_mib << 20
    ms = [int(v) for v in args.ms.split(",")] if args.ms else MS
    rows, lines = [], []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    if args.sweep:
        emit(f"{'format':9s} {'shape':12s} {'M':>3s} {'tiles':>5s} {'split':>5s} {'us':>8s} {'sprd':>5s}   "
             "(* = the launcher's choice)")
    else:
        emit(f"{'format':9s} {'shape':12s} {'N':>6s} {'K':>6s} {'M':>3s} {'split':>5s} {'(a) us':>8s} {'sprd':>5s} "
             f"{'(b) us':>8s} {'sprd':>5s} {'(a) GB/s':>9s} {'b/a':>6s}  win")
    for fmt in fmts:
        for name, n, k in MLP:
            pool, src = packed_pool(fmt, 2 * n, k, pool_bytes, n + k)
            kw = dict(src_bytes=src, chunk_bytes=CHUNK)
            wbytes = fmt.packed_bytes(2 * n * k)  # both parameters' codes and scales
            for m in ms:
                x = torch.randn(m, k, device="cuda", generator=torch.Generator(device="cuda").manual_seed(m)).to(torch.bfloat16)
                cnt = {"a": 0, "b": 0}

                def run_a(split_k=0, row_tiles=0):
                    cnt["a"] += 1
                    return fmt.swiglu(x, pool[cnt["a"] % len(pool)], n, k, gate_offset=OFFSET, up_offset=OFFSET + n * k,
                                      split_k=split_k, row_tiles=row_tiles, **kw)

                def run_b():
                    cnt["b"] += 1
                    p = pool[cnt["b"] % len(pool)]
                    return F.silu(fmt.linear(x, p, n, k, elem_offset=OFFSET, **kw)) * fmt.linear(
                        x, p, n, k, elem_offset=OFFSET + n * k, **kw)

                if args.sweep:
                    chosen = fmt.slices(m, n, k)
                    cases = {(rt, sk): (lambda rt=rt, sk=sk: run_a(sk, rt)) for rt in (1, 2) for sk in (1, 2, 4, 8, 16)
                             if not (rt == 2 and m > 32) and sk <= (16 if m <= 16 and rt == 1 else 8)}
                    cases[(0, 0)] = run_a
                    for (rt, sk), (us, sp) in timed(cases, args.rounds, args.reps).items():
                        rows.append({"format": fmt.label, "shape": name, "M": m, "row_tiles": rt, "split_k": sk,
                                     "us": round(us, 2), "spread": round(sp, 3)})
                        emit(f"{fmt.label:9s} {name:12s} {m:3d} {rt:5d} {sk:5d} {us:8.2f} {sp:5.2f}"
                             + (f"   * split {chosen}" if sk == 0 else ""))
                    continue
                ya, yb = run_a().float(), run_b().float()
                rel = float((ya - yb).norm() / yb.norm())
                t = timed({"a": run_a, "b": run_b}, args.rounds, args.reps)
                ratio = t["b"][0] / t["a"][0]
                win = ratio - 1 > max(t["a"][1], t["b"][1])
                row = {"format": fmt.label, "shape": name, "N": n, "K": k, "M": m, "split_k": fmt.slices(m, n, k),
                       "a_us": round(t["a"][0], 2), "a_spread": round(t["a"][1], 3), "b_us": round(t["b"][0], 2),
                       "b_spread": round(t["b"][1], 3), "a_packed_GBps": round(wbytes / t["a"][0] / 1e3, 1),
                       "b_over_a": round(ratio, 2), "win": bool(win), "a_vs_b_rel_err": rel, "packed_copies": len(pool)}
                rows.append(row)
                emit(f"{fmt.label:9s} {name:12s} {n:6d} {k:6d} {m:3d} {row['split_k']:5d} {row['a_us']:8.2f} "
                     f"{row['a_spread']:5.2f} {row['b_us']:8.2f} {row['b_spread']:5.2f} {row['a_packed_GBps']:9.1f} "
                     f"{row['b_over_a']:6.2f}  {'yes' if win else 'no'}")
            del pool
            torch.cuda.empty_cache()
    out = {"rounds": args.rounds, "reps": args.reps, "pool_MiB": args.pool_mib, "chunk_MiB": CHUNK >> 20,
           "sweep": args.sweep, "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
