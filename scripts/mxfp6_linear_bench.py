#!/usr/bin/env python3
"""ops.mxfp6_linear (W6A16 from the MXFP6-packed layer in place) against the other ways to
multiply by that weight, in one process and run (one MI355X).

Per shape (llama3-70b projections) and M in {1, 8, 16, 64}:

  (a) linear    ops.mxfp6_linear: reads the packed weight (25/64 of the bf16 bytes) once
  (b) unpack+mm ops.mxfp6_unpack_range into a bf16 buffer, then F.linear: what decoder_forward did
                for an MXFP6 parameter before this kernel (reads the packed bytes, writes and reads
                the bf16 ones, two launches or more)
  (c) bf16 mm   F.linear on a bf16 weight unpacked beforehand: what --store bf16 buys, at 2.56
                times the HBM
  (d) the other packed formats on the same weight and shape: ops.mxfp4_linear (17/64 of the bf16
                bytes) and ops.fp8_linear at block 128 (33/64) and block 32 (36/64)

The weight is the [out, in] parameter at element 8192 of a packed layer (64 MiB chunks). Every
call takes the next of a pool of distinct copies of the weight, and a pool is at least --pool-mib
large (default 768 MiB, three times the 256 MiB Infinity Cache), so no call finds its weight in
a cache. Rounds are interleaved over the columns; a round times --reps calls between two device
events. Printed: the median microseconds per call of every column, the spread over the rounds,
max - min, of (a) and (b) in microseconds, (a)'s packed bytes per second, the ratios to (a), and
whether (a) beats (b) by more than the larger of the two spreads.

    python scripts/mxfp6_linear_bench.py [--rounds 7] [--reps 20] [--ms 1,8,16,64] [--out FILE] [--json FILE]

--sweep prints, instead, (a) for every forced split_k and row_tiles (the data behind the
launcher's choices in csrc/kernels/mxfp6_linear.hip).
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
COLUMNS = ["a", "b", "c", "mxfp4", "fp8_128", "fp8_32"]


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


def pool_of(t, pool_bytes):
    n = max(2, -(-pool_bytes // (t.numel() * t.element_size())))
    return [t] + [t.clone() for _ in range(n - 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pool-mib", type=int, default=768)
    ap.add_argument("--shapes", default="", help="comma-separated subset of " + ",".join(s[0] for s in SHAPES))
    ap.add_argument("--ms", default="", help="comma-separated rows of x instead of " + ",".join(map(str, MS)))
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default="", help="the printed table and the JSON line")
    ap.add_argument("--json", default="", help="the JSON result alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mxfp6_linear_bench needs a GPU")
    want = set(args.shapes.split(",")) if args.shapes else None
    ms = [int(v) for v in args.ms.split(",")] if args.ms else MS
    pool_bytes = args.pool_mib << 20
    rows, lines = [], []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    if args.sweep:
        emit(f"{'shape':10s} {'M':>3s} {'tiles':>5s} {'split':>5s} {'us':>8s} {'sprd':>5s} {'GB/s':>7s}"
             "   (* = the launcher's choice of split at that number of row tiles)")
    else:
        emit(f"{'shape':10s} {'N':>6s} {'K':>6s} {'M':>3s} {'split':>5s} {'(a) us':>8s} {'+-us':>6s} {'(b) us':>8s} "
             f"{'+-us':>6s} {'(c) us':>8s} {'mxfp4':>8s} {'fp8/128':>8s} {'fp8/32':>8s} {'(a) GB/s':>9s} {'b/a':>6s} "
             f"{'c/a':>6s} {'a>b':>4s}")
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
        p6 = pool_of(ops.mxfp6_pack_layer(layer, CHUNK), pool_bytes)
        wbytes = n * k // 32 * 25  # the parameter's codes and scale bytes
        kw = dict(src_bytes=src, chunk_bytes=CHUNK, elem_offset=OFFSET)
        if args.sweep:
            for m in ms:
                x, cnt = xs[m], {"a": 0}

                def run_a(sk, rt):
                    cnt["a"] += 1
                    return ops.mxfp6_linear(x, p6[cnt["a"] % len(p6)], n, k, split_k=sk, row_tiles=rt, **kw)

                chosen = _core.mxfp6_linear_slices(m, n, k)
                cases = {(rt, sk): (lambda rt=rt, sk=sk: run_a(sk, rt)) for rt in (1, 2, 4) for sk in (1, 2, 4, 8, 16)
                         if not (rt == 4 and m > 32)}
                for fn in cases.values():
                    fn()
                torch.cuda.synchronize()
                times = timed(cases, args.rounds, args.reps)
                for (rt, sk), t in times.items():
                    med = statistics.median(t)
                    sp = (max(t) - min(t)) / med
                    rows.append({"shape": name, "M": m, "row_tiles": rt, "split_k": sk, "us": round(med, 2),
                                 "spread": round(sp, 3), "packed_GBps": round(wbytes / med / 1e3, 1),
                                 "auto_split_k": chosen})
                    emit(f"{name:10s} {m:3d} {rt:5d} {sk:5d} {med:8.2f} {sp:5.2f} {wbytes / med / 1e3:7.1f}"
                         f"{' *' if sk == chosen else ''}")
            del p6, layer
            torch.cuda.empty_cache()
            continue
        dense = pool_of(ops.mxfp6_unpack_range(p6[0], src, CHUNK, OFFSET, n * k).view(n, k), pool_bytes)
        p4 = pool_of(ops.mxfp4_pack_layer(layer, CHUNK), pool_bytes)
        p8 = {b: pool_of(ops.fp8_pack_layer(layer, CHUNK, b), pool_bytes) for b in (128, 32)}
        for m in ms:
            x = xs[m]
            cnt = {c: 0 for c in COLUMNS}

            def nxt(c, pool):
                cnt[c] += 1
                return pool[cnt[c] % len(pool)]

            def run_a():
                return ops.mxfp6_linear(x, nxt("a", p6), n, k, **kw)

            def run_b():
                return F.linear(x, ops.mxfp6_unpack_range(nxt("b", p6), src, CHUNK, OFFSET, n * k).view(n, k))

            def run_c():
                return F.linear(x, nxt("c", dense))

            def run_4():
                return ops.mxfp4_linear(x, nxt("mxfp4", p4), n, k, **kw)

            def run_8(block):
                return ops.fp8_linear(x, nxt(f"fp8_{block}", p8[block]), n, k, block=block, **kw)

            cases = {"a": run_a, "b": run_b, "c": run_c, "mxfp4": run_4, "fp8_128": lambda: run_8(128),
                     "fp8_32": lambda: run_8(32)}
            ya, yc = run_a().float(), run_c().float()  # (c) multiplies by the very weights (a) dequantizes
            for _ in range(2):  # the warm-up of every column
                for fn in cases.values():
                    fn()
            torch.cuda.synchronize()
            rel = float((ya - yc).norm() / yc.norm())
            times = timed(cases, args.rounds, args.reps)
            med = {c: statistics.median(t) for c, t in times.items()}
            width = {c: max(t) - min(t) for c, t in times.items()}
            wins = med["b"] - med["a"] > max(width["a"], width["b"])
            row = {"shape": name, "N": n, "K": k, "M": m, "split_k": _core.mxfp6_linear_slices(m, n, k)}
            for c in COLUMNS:
                row[f"{c}_us"] = round(med[c], 2)
                row[f"{c}_min_us"], row[f"{c}_max_us"] = round(min(times[c]), 2), round(max(times[c]), 2)
            row.update({"a_packed_TBps": round(wbytes / med["a"] / 1e6, 3), "b_over_a": round(med["b"] / med["a"], 2),
                        "c_over_a": round(med["c"] / med["a"], 2), "mxfp4_over_a": round(med["mxfp4"] / med["a"], 2),
                        "fp8_128_over_a": round(med["fp8_128"] / med["a"], 2),
                        "fp8_32_over_a": round(med["fp8_32"] / med["a"], 2), "a_beats_b_beyond_spread": bool(wins),
                        "a_vs_c_rel_err": rel, "copies": {"mxfp6": len(p6), "bf16": len(dense), "mxfp4": len(p4),
                                                          "fp8_128": len(p8[128]), "fp8_32": len(p8[32])}})
            rows.append(row)
            emit(f"{name:10s} {n:6d} {k:6d} {m:3d} {row['split_k']:5d} {med['a']:8.2f} {width['a']:6.2f} {med['b']:8.2f} "
                 f"{width['b']:6.2f} {med['c']:8.2f} {med['mxfp4']:8.2f} {med['fp8_128']:8.2f} {med['fp8_32']:8.2f} "
                 f"{wbytes / med['a'] / 1e3:9.1f} {row['b_over_a']:6.2f} {row['c_over_a']:6.2f} {'yes' if wins else 'NO':>4s}")
        del p6, dense, p4, p8, layer
        torch.cuda.empty_cache()
    out = {"rounds": args.rounds, "reps": args.reps, "pool_MiB": args.pool_mib, "chunk_MiB": CHUNK >> 20,
           "sweep": args.sweep, "device": torch.cuda.get_device_name(0), "rows": rows}
    if not args.sweep:
        out["a_beats_b_beyond_spread_at_M_le_16"] = all(r["a_beats_b_beyond_spread"] for r in rows if r["M"] <= 16)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(out) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
