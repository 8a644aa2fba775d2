"""bench.py --dump-outputs / --full: the sampling plan (CPU) and one small run
whose dumped arrays are checked against the host's copy of the seeded layers."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


def test_flags_parse_and_default_off():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert a.steps == 3 and a.warmup == 2 and a.full is False and a.dump_outputs == ""
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_plan_is_fixed_bounded_and_covers_the_ends():
    sizes = [80 * MiB + 13] * 80
    plan = bench.dump_plan(sizes)
    assert plan == bench.dump_plan(sizes)  # seeded: the same ranges every run
    assert sum(n for _, _, n in plan) <= bench.DUMP_SAMPLE_BYTES
    # all outputs as float32 stay far below 64 MB
    assert 4 * sum(n for _, _, n in plan) + 8 * 3 * len(plan) < 64 * 10**6
    for layer, size in enumerate(sizes):
        mine = [(off, n) for l, off, n in plan if l == layer]
        assert mine[0][0] == 0 and mine[-1][0] + mine[-1][1] == size  # first and last bytes of every layer
        assert all(0 <= off and off + n <= size for off, n in mine)
        assert mine == sorted(set(mine))
    assert len({off for _, off, _ in plan}) > 80  # random blocks differ between layers


def test_dump_plan_takes_small_layers_whole():
    assert bench.dump_plan([5, 4096, 70000]) == [(0, 0, 5), (1, 0, 4096), (2, 0, 70000)]
    # a tight budget: two blocks of each layer at the least, the ends
    assert bench.dump_plan([3 * 4096 + 1], budget=4096) == [(0, 0, 4096), (0, 2 * 4096 + 1, 4096)]


@pytest.mark.gpu
def test_bench_dumps_the_layers_it_placed(core, tmp_path):
    """3 x 5 MiB on a 2 MiB grid (every layer ends in a 1 MiB chunk; larger than
    its sample share, so blocks are sampled): the dumped CRCs and bytes equal
    the host's generation of the same seeded layers, and the result line counts
    the steps it was asked for."""
    from distributed_llm_dissemination_amd.parallel.runtime import layer_seed

    layers, size, chunk = 3, 5 * MiB, 2 * MiB
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--layers", str(layers), "--layer-mib", "5", "--chunk-mib", "2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["unit"] == "GB/s" and res["value"] > 0
    want = [core.fill_random_host(size, layer_seed(0, l)) for l in range(layers)]
    crc = np.load(out / "layers_crc32c.npy")
    assert crc.dtype == np.float64
    assert [int(c) for c in crc] == [core.crc32c(w[o:o + chunk]) for w in want for o in range(0, size, chunk)]
    sample, index = np.load(out / "layers_sample.npy"), np.load(out / "layers_sample_index.npy")
    assert sample.dtype == np.float32 and index.dtype == np.float64
    plan = [(int(l), int(o), int(n)) for l, o, n in index]
    assert plan == bench.dump_plan([size] * layers)
    ref = np.concatenate([np.frombuffer(want[l][o:o + n], dtype=np.uint8) for l, o, n in plan])
    assert sample.shape == ref.shape and np.array_equal(sample, ref.astype(np.float32))
    assert sorted(os.listdir(out)) == ["layers_crc32c.npy", "layers_sample.npy", "layers_sample_index.npy"]
