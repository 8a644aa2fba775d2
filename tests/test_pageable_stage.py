"""Pageable host layers through the bounce ring, on the simulator (CPU).

A host layer the copy queues cannot DMA from (Backend::host_pinned says no:
the pinned pool was exhausted, or the memory was malloc'ed) is staged like a
disk-tier chunk without the read: a reader thread copies the chunk into a
pinned bounce buffer, and the buffer goes to HBM on a copy queue of its own.
Here the simulator is told which layers are pageable (_core.sim_set_pageable)
and the tests check the bytes, the counters, the ring's deadlock freedom, the
re-stage after a CRC mismatch, and - in model time - that the pageable chunks
cost the step nothing while the readers keep up, and a great deal when they
cannot (so the copy time is really charged).

Sizes: the packed formats need layer sizes of whole scale blocks (fp8's
smallest block is 32 bf16 values, 64 B), so the fp8 case has a 64-byte tail
where the unpacked case has 48 bytes.
"""

import contextlib
import itertools
import os
import threading
import time

import pytest

from distributed_llm_dissemination_amd import _core
from distributed_llm_dissemination_amd.models.catalog import make_workload
from distributed_llm_dissemination_amd.parallel import simclock
from distributed_llm_dissemination_amd.parallel.runtime import Runtime

KiB, MiB = 1 << 10, 1 << 20
_keys = itertools.count()


@contextlib.contextmanager
def pageable(rts, layers):
    """Register the host buffers of `layers` (on the ranks that hold them) as pageable."""
    marked = [r.layers[l] for r in rts for l in layers if l in r.layers and r.layers[l].has_host]
    for src in marked:
        _core.sim_set_pageable(src, True)
    try:
        yield
    finally:
        for src in marked:
            _core.sim_set_pageable(src, False)


def held_host_bytes(rt, layers):
    """Source bytes of the host-tier layers among `layers` that this rank holds."""
    return sum(rt.sizes[l] for l in layers if l in rt.layers and rt.layers[l].has_host)


def run(cfg, chunk, page, *, pack="none", opts=None):
    """One mode-1 session of `cfg` with the layers `page` pageable; returns (results, HBM images per rank)."""
    key = f"page{os.getpid()}_{next(_keys)}"
    n = len(cfg.nodes)
    kw = dict(pack=pack, pack_block=32) if pack != "none" else {}
    rts = [Runtime(cfg, i, engine="sim", registry={i: "127.0.0.1:0"}, chunk_bytes=chunk, sim_key=key,
                   engine_opts=opts or {}, **kw) for i in range(n)]
    reg = {i: r.transport.address() for i, r in enumerate(rts)}
    for r in rts:
        r.transport.set_registry(reg)
    try:
        with pageable(rts, page):
            for r in rts:
                r.prepare(1)
            res = [None] * n
            ths = [threading.Thread(target=lambda i=i: res.__setitem__(i, rts[i].execute(30))) for i in range(n)]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            assert all(x.ok for x in res), [x.error for x in res]
            images = [{l: r.layer_bytes(l) for l in sorted(cfg.layer_sizes())} for r in rts]
            bounced = [held_host_bytes(r, page) for r in rts]
        return res, images, bounced
    finally:
        for r in rts:
            r.close()


@pytest.mark.parametrize("pack", ["none", "fp8"])
@pytest.mark.parametrize("n", [1, 2])
def test_pageable_layers_land_the_same_bytes(n, pack):
    chunk = 64 * KiB
    size = 4 * chunk + (48 if pack == "none" else 64)
    cfg = make_workload(n, 6, size, tier="host", seeding="random", chunk_bytes=chunk)
    res0, img0, _ = run(cfg, chunk, [], pack=pack)
    res1, img1, bounced = run(cfg, chunk, [1, 4], pack=pack)
    assert img1 == img0
    assert sum(bounced) == 2 * size  # each pageable layer is held, and staged, by exactly one rank
    for r in range(n):
        s0, s1 = res0[r].engine_stats, res1[r].engine_stats
        print(f"rank {r}: host_bounce_bytes {s1['host_bounce_bytes']} (want {bounced[r]}), "
              f"verify_chunks {s1['verify_chunks']}, all-pinned run {s0['host_bounce_bytes']}")
        assert s1["host_bounce_bytes"] == bounced[r] and s0["host_bounce_bytes"] == 0
        assert s1["verify_failures"] == 0 and s1["unverified_pieces"] == 0
        assert s1["verify_chunks"] == s0["verify_chunks"] == 6 * 5  # every chunk of every layer checked, on every rank
        assert s1["bytes_staged"] == s0["bytes_staged"]
        for k in ("disk_direct_bytes", "disk_buffered_bytes"):
            assert s1[k] == 0 and s0[k] == 0


def test_ring_smaller_than_the_work():
    """One bounce buffer, three pageable layers, two ranks that each hold a
    pageable layer the other needs: a buffer returns to the ring when its H2D
    copy lands (not when the chunk's check does, which may wait on the peer),
    so the session completes."""
    chunk = 64 * KiB
    size = 4 * chunk + 48
    cfg = make_workload(2, 6, size, tier="host", seeding="random", chunk_bytes=chunk)
    owner = {l: r for r, nd in enumerate(cfg.nodes) for per in nd.initial_layers.values() for l in per}
    mine = [[l for l in range(6) if owner[l] == r] for r in range(2)]
    page = [mine[0][0], mine[1][0], mine[1][1]]
    _, img0, _ = run(cfg, chunk, [])
    res, img, bounced = run(cfg, chunk, page, opts={"disk_ring": 1})
    assert img == img0
    assert bounced == [size, 2 * size]
    assert [r.engine_stats["host_bounce_bytes"] for r in res] == bounced


def restage_failure(page):
    """Layer 1 of 3 with chunk 2's manifest CRC wrong: (engine error, engine stats) once the engine has failed."""
    chunk = 64 * KiB
    cfg = make_workload(1, 3, 4 * chunk + 48, tier="host", chunk_bytes=chunk)
    rt = Runtime(cfg, 0, engine="sim", registry={0: "127.0.0.1:0"}, chunk_bytes=chunk,
                 sim_key=f"page{os.getpid()}_{next(_keys)}")
    try:
        with pageable([rt], page):
            crc = list(rt.engine.manifest()[1].crc)
            crc[2] ^= 0x5A5A5A5A
            rt.engine.set_manifest(1, _core.CrcManifest(rt.grid, crc))
            rt.prepare(1)  # one rank: the leader plans and loads at once
            deadline = time.monotonic() + 30
            while not rt.engine.error() and time.monotonic() < deadline:
                time.sleep(0.002)
            return rt.engine.error(), rt.engine.stats()
    finally:
        rt.close()


def test_bad_manifest_restages_through_the_ring():
    """A pageable layer with one wrong manifest CRC is staged again through the
    ring, max_retries (4) times, and then fails as a pinned layer does."""
    chunk = 64 * KiB
    err, st = restage_failure([1])
    assert "CRC32C mismatch layer 1 chunk 2" in err and "retries exhausted" in err
    assert st.verify_failures == 5
    assert st.host_bounce_bytes == 4 * chunk + 48 + 4 * chunk  # the layer once, then chunk 2 four more times
    err0, st0 = restage_failure([])
    assert "retries exhausted" in err0 and st0.verify_failures == 5 and st0.host_bounce_bytes == 0


def timed(page, readers, host_copy_bps):
    """Model-time makespan of 20 layers x 16 chunks of 1 MiB on one rank."""
    key = f"pagetime{os.getpid()}_{next(_keys)}"
    t = _core.SimTiming()
    t.stage_bps = 57.5e9
    t.host_copy_bps = host_copy_bps
    _core.sim_set_timing(key, t)
    cfg = make_workload(1, 20, 16 * MiB, tier="host", chunk_bytes=MiB)
    with simclock.virtual_clock():
        rt = Runtime(cfg, 0, engine="sim", transport="inproc", registry={0: f"{key}/0"}, chunk_bytes=MiB,
                     sim_key=key, engine_opts={"disk_readers": readers})
        try:
            with pageable([rt], page):
                rt.prepare(1)
                (res,), dt = simclock.run_ranks([lambda: rt.execute(60)])
            assert res.ok, res.error
            assert res.engine_stats["host_bounce_bytes"] == len(page) * 16 * MiB
            return dt
        finally:
            rt.close()


def test_model_time_pageable_layers_cost_nothing_while_readers_keep_up():
    """20 % of the bytes pageable, four readers at 12 GB/s each: the bounce
    queue shares the rank's one PCIe with the pinned copies, the readers need
    11.5 GB/s in all, and the step stays within 3 % of bytes / PCIe rate - the
    margin tests/test_timing_sim.py gives every closed form. With one reader
    at 2 GB/s the pageable bytes alone take 5.75 x the bound."""
    bound = 20 * 16 * MiB / 57.5e9
    page = [16, 17, 18, 19]
    pinned = timed([], 4, 12e9)
    a = timed(page, 4, 12e9)
    b = timed(page, 4, 12e9)
    slow = timed(page, 1, 2e9)
    print(f"bound {bound * 1e3:.3f} ms: all pinned {pinned * 1e3:.3f}, pageable 16-19 {a * 1e3:.3f} and "
          f"{b * 1e3:.3f}, one reader at 2 GB/s {slow * 1e3:.3f}")
    assert bound <= pinned <= 1.03 * bound
    assert bound <= a <= 1.03 * bound
    # identical to the microsecond: the resolution tests/test_timing_sim.py::test_model_time_is_deterministic holds
    # model time to (absolute clock values differ between runs, so the last float bits of a span do too)
    assert round(a * 1e3, 3) == round(b * 1e3, 3), (a, b)
    assert slow > 1.5 * 1.03 * bound
