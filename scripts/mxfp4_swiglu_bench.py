#!/usr/bin/env python3
"""The fused routes of a packed decoder layer against the per-projection routes, in one process
and run (one MI355X).

Gated MLP, gate/up of llama3-70b (28672 x 8192) and llama3-8b (14336 x 4096), M in {1, 8, 16, 64}:

  (a) swiglu    ops.mxfp4_swiglu: one launch, x read once, g and u never leave the accumulators
  (b) 2 linear  two ops.mxfp4_linear (bf16) and F.silu(g) * u: two launches, two elementwise
                launches, g, u and the product through HBM

QKV of llama3-70b (q 8192, k and v 1024 rows, K = 8192), the same M:

  (a) one call  ops.mxfp4_linear over the contiguous [10240, 8192] weight
  (b) 3 calls   one ops.mxfp4_linear per projection

The parameters lie one behind the other at element 8192 of a packed layer (64 MiB chunks), as in
a layer blob. Every call takes the next of a pool of distinct copies of the layer, and a pool is
at least --pool-mib large (default 768 MiB, three times the 256 MiB Infinity Cache), so no call
finds its weights in a cache. Rounds are interleaved over the columns; a round times --reps calls
between two device events. Printed: the median microseconds per call, the spread of (a) and (b)
over the rounds ((max - min) / median), (a)'s packed bytes per second, and (b)/(a).

    python scripts/mxfp4_swiglu_bench.py [--rounds 7] [--reps 20] [--ms 1,8,16,64] [--out FILE]

--sweep prints, instead, (a) of the gated MLP for every forced split_k and row_tiles (the data
behind the launcher's choices in csrc/kernels/mxfp4_swiglu.hip).
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
QKV = [("70b qkv", (8192, 1024, 1024), 8192)]
MS = [1, 8, 16, 64]
CHUNK = 64 << 20
OFFSET = 8192  # a norm weight ahead of the parameters, as in a layer blob


def packed_pool(rows, k, pool_bytes, seed):
    """(copies of the packed layer [norm weight, `rows` x k weights], its source bytes)."""
    total = OFFSET + rows * k
    g = torch.Generator(device="cuda").manual_seed(seed)
    layer = torch.empty(total, dtype=torch.bfloat16, device="cuda")
    layer[:OFFSET] = 1.0
    layer[OFFSET:] = (torch.randn(rows * k, device="cuda", generator=g) / k ** 0.5).to(torch.bfloat16)
    p0 = ops.mxfp4_pack_layer(layer, CHUNK)
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pool-mib", type=int, default=768)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--ms", default="", help="comma-separated rows of x instead of " + ",".join(map(str, MS)))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mxfp4_swiglu_bench needs a GPU")
    pool_bytes = args.pool_mib << 20
    ms = [int(v) for v in args.ms.split(",")] if args.ms else MS
    rows, lines = [], []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    if args.sweep:
        emit(f"{'shape':12s} {'M':>3s} {'tiles':>5s} {'split':>5s} {'us':>8s} {'sprd':>5s}   (* = the launcher's choice)")
    else:
        emit(f"{'shape':12s} {'N':>6s} {'K':>6s} {'M':>3s} {'split':>5s} {'(a) us':>8s} {'sprd':>5s} {'(b) us':>8s} "
             f"{'sprd':>5s} {'(a) GB/s':>9s} {'b/a':>6s}")
    for name, n, k in MLP:
        pool, src = packed_pool(2 * n, k, pool_bytes, n + k)
        kw = dict(src_bytes=src, chunk_bytes=CHUNK)
        wbytes = 2 * n * k * 17 // 32  # both parameters' codes and scales
        for m in ms:
            x = torch.randn(m, k, device="cuda", generator=torch.Generator(device="cuda").manual_seed(m)).to(torch.bfloat16)
            cnt = {"a": 0, "b": 0}

            def run_a(split_k=0, row_tiles=0):
                cnt["a"] += 1
                return ops.mxfp4_swiglu(x, pool[cnt["a"] % len(pool)], n, k, gate_offset=OFFSET, up_offset=OFFSET + n * k,
                                        split_k=split_k, row_tiles=row_tiles, **kw)

            def run_b():
                cnt["b"] += 1
                p = pool[cnt["b"] % len(pool)]
                return F.silu(ops.mxfp4_linear(x, p, n, k, elem_offset=OFFSET, **kw)) * ops.mxfp4_linear(
                    x, p, n, k, elem_offset=OFFSET + n * k, **kw)

            if args.sweep:
                chosen = _core.mxfp4_swiglu_slices(m, n, k)
                cases = {(rt, sk): (lambda rt=rt, sk=sk: run_a(sk, rt)) for rt in (1, 2) for sk in (1, 2, 4, 8, 16)
                         if not (rt == 2 and m > 32) and sk <= (16 if m <= 16 and rt == 1 else 8)}
                cases[(0, 0)] = run_a
                for (rt, sk), (us, sp) in timed(cases, args.rounds, args.reps).items():
                    rows.append({"shape": name, "M": m, "row_tiles": rt, "split_k": sk, "us": round(us, 2)})
                    emit(f"{name:12s} {m:3d} {rt:5d} {sk:5d} {us:8.2f} {sp:5.2f}" + (f"   * split {chosen}" if sk == 0 else ""))
                continue
            ya, yb = run_a().float(), run_b().float()
            rel = float((ya - yb).norm() / yb.norm())
            t = timed({"a": run_a, "b": run_b}, args.rounds, args.reps)
            row = {"shape": name, "N": n, "K": k, "M": m, "split_k": _core.mxfp4_swiglu_slices(m, n, k),
                   "a_us": round(t["a"][0], 2), "a_spread": round(t["a"][1], 3), "b_us": round(t["b"][0], 2),
                   "b_spread": round(t["b"][1], 3), "a_packed_GBps": round(wbytes / t["a"][0] / 1e3, 1),
                   "b_over_a": round(t["b"][0] / t["a"][0], 2), "a_vs_b_rel_err": rel, "packed_copies": len(pool)}
            rows.append(row)
            emit(f"{name:12s} {n:6d} {k:6d} {m:3d} {row['split_k']:5d} {row['a_us']:8.2f} {row['a_spread']:5.2f} "
                 f"{row['b_us']:8.2f} {row['b_spread']:5.2f} {row['a_packed_GBps']:9.1f} {row['b_over_a']:6.2f}")
        del pool
        torch.cuda.empty_cache()
    for name, ns, k in ([] if args.sweep else QKV):
        n = sum(ns)
        pool, src = packed_pool(n, k, pool_bytes, n + k)
        kw = dict(src_bytes=src, chunk_bytes=CHUNK)
        wbytes = n * k * 17 // 32
        offs = [OFFSET + sum(ns[:i]) * k for i in range(len(ns))]
        for m in ms:
            x = torch.randn(m, k, device="cuda", generator=torch.Generator(device="cuda").manual_seed(m)).to(torch.bfloat16)
            cnt = {"a": 0, "b": 0}

            def one():
                cnt["a"] += 1
                y = ops.mxfp4_linear(x, pool[cnt["a"] % len(pool)], n, k, elem_offset=OFFSET, **kw)
                return y[:, :ns[0]], y[:, ns[0]:ns[0] + ns[1]], y[:, ns[0] + ns[1]:]

            def three():
                cnt["b"] += 1
                p = pool[cnt["b"] % len(pool)]
                return tuple(ops.mxfp4_linear(x, p, ni, k, elem_offset=o, **kw) for ni, o in zip(ns, offs))

            ya, yb = torch.cat(one(), 1).float(), torch.cat(three(), 1).float()
            rel = float((ya - yb).norm() / yb.norm())
            t = timed({"a": one, "b": three}, args.rounds, args.reps)
            row = {"shape": name, "N": n, "K": k, "M": m, "split_k": _core.mxfp4_linear_slices(m, n, k),
                   "a_us": round(t["a"][0], 2), "a_spread": round(t["a"][1], 3), "b_us": round(t["b"][0], 2),
                   "b_spread": round(t["b"][1], 3), "a_packed_GBps": round(wbytes / t["a"][0] / 1e3, 1),
                   "b_over_a": round(t["b"][0] / t["a"][0], 2), "a_vs_b_rel_err": rel, "packed_copies": len(pool)}
            rows.append(row)
            emit(f"{name:12s} {n:6d} {k:6d} {m:3d} {row['split_k']:5d} {row['a_us']:8.2f} {row['a_spread']:5.2f} "
                 f"{row['b_us']:8.2f} {row['b_spread']:5.2f} {row['a_packed_GBps']:9.1f} {row['b_over_a']:6.2f}")
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
