"""The host-side sizing of ops.attn_decode (csrc/kernels/attn_decode_plan.h: the checks, the grid
and the workspace of a launch) under Address and UndefinedBehavior sanitizer: `make sanitize-attn`
builds csrc/tests/attn_decode_selftest.cc (a stand-alone program, no GPU) with
-fsanitize=address,undefined and runs it. The program walks an exact-size workspace with the two
kernels' own index arithmetic - an index past the plan's size ends it with a sanitizer report - and
takes the plan to the extremes of the contract, where a product that leaves int64 is reported."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attn_decode_selftest_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", ROOT, "sanitize-attn"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "attn_decode_selftest ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
