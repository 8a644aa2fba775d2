#!/usr/bin/env python3
"""What ops.attn_decode on an MXFP8 KV cache gives for the contract's non-finite clauses (one MI355X): a
scale byte of 255, a NaN code (0x7F / 0xFF) and - outside the contract - a scale byte of 0, each planted at
one place inside the valid prefix of sequence 1, KV head 0 of a [2, 2, 300, 128] cache with 4 query heads
per KV head. Printed per case: how many of that (sequence, KV head)'s 4 * 128 output elements are NaN or
inf, and whether every other row kept its bits. profiles/attn_decode_mxfp8/nonfinite_probe.txt is its output.

    python scripts/attn_decode_mxfp8_nonfinite.py
"""

import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from distributed_llm_dissemination_amd import ops  # noqa: E402

CASES = {  # name: (tensor index in (k codes, k scales, v codes, v scales), index, value)
    "k scale 255": (1, (1, 0, 270, 2), 255),
    "v scale 255": (3, (1, 0, 270, 2), 255),
    "k code 0x7F": (0, (1, 0, 17, 5), 0x7F),
    "v code 0xFF": (2, (1, 0, 17, 5), 0xFF),
    "k scale 255 at a zero code": (1, (1, 0, 270, 2), 255),
    "v scale 0": (3, (1, 0, 270, 2), 0),
    "k scale 0": (1, (1, 0, 270, 2), 0),
}


def main():
    if not torch.cuda.is_available():
        sys.exit("attn_decode_mxfp8_nonfinite needs a GPU")
    torch.manual_seed(0)
    b, kvh, g, n, d = 2, 2, 4, 300, 128
    k = torch.randn(b, kvh, n, d).to(torch.bfloat16).cuda()
    v = torch.randn(b, kvh, n, d).to(torch.bfloat16).cuda()
    q = torch.randn(b, kvh * g, d).to(torch.bfloat16).cuda()
    lens = torch.full((b,), n, dtype=torch.int32, device="cuda")
    clean = ops.mxfp8_quantize_rows(k) + ops.mxfp8_quantize_rows(v)

    def attend(t):
        return ops.attn_decode(q, t[0], t[2], lens, k_scale=t[1], v_scale=t[3], out_dtype=torch.float32).view(b, kvh, g, d)

    base = attend(clean)
    for name, (which, idx, value) in CASES.items():
        t = [x.clone() for x in clean]
        if name.endswith("zero code"):
            t[0][1, 0, 270, 64:96] = 0
        t[which][idx] = value
        y = attend(t)
        hit = y[1, 0]
        others = torch.equal(y[0].view(torch.int32), base[0].view(torch.int32)) and torch.equal(
            y[1, 1].view(torch.int32), base[1, 1].view(torch.int32))
        print(f"{name:28s} nan elements of the (b, kv head) {int(hit.isnan().sum())}/{hit.numel()}"
              f" inf {int(hit.isinf().sum())} other rows keep bits {others}", flush=True)


if __name__ == "__main__":
    main()
