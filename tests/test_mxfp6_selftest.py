"""The MXFP6 host codec under Address and UndefinedBehavior sanitizer: `make sanitize-mxfp6`
builds csrc/tests/mxfp6_selftest.cc (a stand-alone program, exact-size heap buffers) with
-fsanitize=address,undefined and runs it: pack, unpack, layer and range over a layer with an
odd tail block count and offsets inside blocks, byte-straddling codes and chunk edges. A 6-bit
extraction that reads past a block or a chunk ends the program with a sanitizer report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mxfp6_selftest_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", ROOT, "sanitize-mxfp6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "mxfp6_selftest ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
