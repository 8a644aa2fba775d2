#!/usr/bin/env python3
"""MXFP6 kernels against their fp8 and MXFP4 counterparts, in one process and run (one MI355X).

Per 64 MiB bf16 source chunk, with 16 chunks back to back (pack, unpack) or 16 per launch
(verify + unpack, on all CUs and with the grid of the verify stream's 32 CUs):

  pack     reads 64 MiB, writes 25 MiB (mxfp6) / 17 MiB (mxfp4) / 36 MiB (fp8 at block 32)
  unpack   the reverse
  verify   CRC32C of the packed chunk and its 64 MiB of bf16: fp8 and mxfp4 read the packed
           chunk once (the fused kernel), mxfp6 twice (the CRC walk, then the unpack kernel)

The yardsticks are the fp8 and MXFP4 kernels measured in the same round: every round times
every kernel once, the rounds are interleaved, and the script prints the median, the extremes
and the spread (max - min over the median) over the rounds. The chunks cycle through a pool
larger than the 256 MiB Infinity Cache. The payload is bf16 weights (normal, sigma 0.02).

    python scripts/mxfp6_bench.py [--rounds 9] [--reps 4] [--pool 24] [--out FILE]
"""

import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from distributed_llm_dissemination_amd import _core  # noqa: E402

CHUNK = 64 << 20
N = CHUNK // 2
K = 16
NQ6 = N // 32 * 24  # bytes of MXFP6 codes of a chunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=4, help="timed repetitions of each 16-chunk pass per round")
    ap.add_argument("--pool", type=int, default=24, help="distinct 64 MiB chunks cycled through (>= 16)")
    ap.add_argument("--fp8-block", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pool, blk = max(K, args.pool), args.fp8_block
    assert _core.crc32c_batch_max() >= K

    def u8(n):
        return torch.empty(n, dtype=torch.uint8, device="cuda")

    p8, p4, p6 = (_core.fp8_packed_size(CHUNK, CHUNK, blk), _core.mxfp4_packed_size(CHUNK, CHUNK),
                  _core.mxfp6_packed_size(CHUNK, CHUNK))
    src, f8, m4, m6, outs = [], [], [], [], [u8(CHUNK) for _ in range(pool)]
    for i in range(pool):
        g = torch.Generator(device="cuda").manual_seed(900 + i)
        s = (torch.randn(N, device="cuda", generator=g) * 0.02).to(torch.bfloat16).view(torch.uint8)
        src.append(s)
        f8.append(u8(p8))
        m4.append(u8(p4))
        m6.append(u8(p6))
        _core.fp8_pack_chunks(s.data_ptr(), CHUNK, CHUNK, blk, f8[i].data_ptr())
        _core.mxfp4_pack_chunks(s.data_ptr(), CHUNK, CHUNK, m4[i].data_ptr())
        _core.mxfp6_pack_chunks(s.data_ptr(), CHUNK, CHUNK, m6[i].data_ptr())
    ws = torch.zeros(_core.crc32c_batch_workspace_bytes(), dtype=torch.uint8, device="cuda")
    res = torch.zeros(K, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    calls = [0]

    def ids():
        base = (calls[0] * K) % pool
        calls[0] += 1
        return [(base + j) % pool for j in range(K)]

    def pack_fp8():
        for i in ids():
            _core.fp8_pack(src[i].data_ptr(), N, f8[i].data_ptr(), f8[i].data_ptr() + N, blk)

    def pack_mx4():
        for i in ids():
            _core.mxfp4_pack(src[i].data_ptr(), N, m4[i].data_ptr(), m4[i].data_ptr() + N // 2)

    def pack_mx6():
        for i in ids():
            _core.mxfp6_pack(src[i].data_ptr(), N, m6[i].data_ptr(), m6[i].data_ptr() + NQ6)

    def unpack_fp8():
        for i in ids():
            _core.fp8_unpack(f8[i].data_ptr(), f8[i].data_ptr() + N, N, outs[i].data_ptr(), blk)

    def unpack_mx4():
        for i in ids():
            _core.mxfp4_unpack(m4[i].data_ptr(), m4[i].data_ptr() + N // 2, N, outs[i].data_ptr())

    def unpack_mx6():
        for i in ids():
            _core.mxfp6_unpack(m6[i].data_ptr(), m6[i].data_ptr() + NQ6, N, outs[i].data_ptr())

    def verify_fp8(cus):
        items = [(f8[i].data_ptr(), CHUNK, outs[i].data_ptr()) for i in ids()]
        _core.fp8_verify_unpack_batch_async(items, blk, res.data_ptr(), ws.data_ptr(), 0, cus)

    def verify_mx4(cus):
        items = [(m4[i].data_ptr(), CHUNK, outs[i].data_ptr()) for i in ids()]
        _core.mxfp4_verify_unpack_batch_async(items, res.data_ptr(), ws.data_ptr(), 0, cus)

    def verify_mx6(cus):
        items = [(m6[i].data_ptr(), CHUNK, outs[i].data_ptr()) for i in ids()]
        _core.mxfp6_verify_unpack_batch_async(items, res.data_ptr(), ws.data_ptr(), 0, cus)

    cases = {  # name -> (fn, bytes moved per chunk)
        "pack_fp8": (pack_fp8, CHUNK + p8), "pack_mxfp4": (pack_mx4, CHUNK + p4), "pack_mxfp6": (pack_mx6, CHUNK + p6),
        "unpack_fp8": (unpack_fp8, CHUNK + p8), "unpack_mxfp4": (unpack_mx4, CHUNK + p4),
        "unpack_mxfp6": (unpack_mx6, CHUNK + p6),
        "verify_fp8_all_cus": (lambda: verify_fp8(0), CHUNK + p8),
        "verify_mxfp4_all_cus": (lambda: verify_mx4(0), CHUNK + p4),
        "verify_mxfp6_all_cus": (lambda: verify_mx6(0), CHUNK + 2 * p6),
        "verify_fp8_32_cus": (lambda: verify_fp8(32), CHUNK + p8),
        "verify_mxfp4_32_cus": (lambda: verify_mx4(32), CHUNK + p4),
        "verify_mxfp6_32_cus": (lambda: verify_mx6(32), CHUNK + 2 * p6),
    }
    times = {k: [] for k in cases}
    for fn, _ in cases.values():  # warm up: code objects, CRC tables
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, (fn, _) in cases.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.reps / K)  # us per chunk

    # the kernels computed what the host codec computes (one chunk each)
    i = 0
    want = _core.mxfp6_pack_layer_host(src[i].cpu().numpy().tobytes(), CHUNK)
    _core.mxfp6_pack(src[i].data_ptr(), N, m6[i].data_ptr(), m6[i].data_ptr() + NQ6)
    res.zero_()
    outs[i].zero_()
    _core.mxfp6_verify_unpack_batch_async([(m6[i].data_ptr(), CHUNK, outs[i].data_ptr())], res.data_ptr(),
                                          ws.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    checks = {"pack_matches_host": m6[i].cpu().numpy().tobytes() == want,
              "verify_crc_matches_host": (res[0].item() & 0xFFFFFFFF) == _core.crc32c(want),
              "verify_bf16_matches_host": outs[i].cpu().numpy().tobytes() == _core.mxfp6_unpack_layer_host(want, CHUNK, CHUNK)}

    out = {"chunk_MiB": CHUNK >> 20, "chunks_per_pass": K, "rounds": args.rounds, "reps": args.reps,
           "fp8_block": blk, "payload": "weights", **checks, "cases": {}}
    lines = [f"{'case':22s} {'us/chunk':>9s} {'min':>7s} {'max':>7s} {'spread':>7s} {'MiB moved':>9s} {'GB/s':>8s}"]
    for name, (_, moved) in cases.items():
        t = times[name]
        med = statistics.median(t)
        out["cases"][name] = {"us_per_chunk": round(med, 2), "min": round(min(t), 2), "max": round(max(t), 2),
                              "spread": round((max(t) - min(t)) / med, 3), "MiB_moved": round(moved / (1 << 20), 1),
                              "GBps": round(moved / med / 1e3, 1)}
        c = out["cases"][name]
        lines.append(f"{name:22s} {c['us_per_chunk']:9.2f} {c['min']:7.2f} {c['max']:7.2f} {c['spread']:7.3f} "
                     f"{c['MiB_moved']:9.1f} {c['GBps']:8.1f}")
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if all(checks.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
