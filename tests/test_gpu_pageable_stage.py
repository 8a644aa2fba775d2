"""Pageable host layers through the bounce ring on the GPU.

DISSEM_PINNED_LIMIT_BYTES makes HostBuffer.pinned hand out pageable memory past
a cap, which is what a pinned pool smaller than the model does. The engine
then finds those layers pageable (hipPointerGetAttributes) and stages their
chunks through its pinned bounce ring on a copy stream of its own. 5 layers of
3 chunks and a tail, the last 3 layers pageable: 12 pageable chunks, more than
the ring's 8 buffers. The HBM images must be byte for byte those of a run with
every layer pinned.

Sizes: the packed formats need layer sizes of whole scale blocks (64 B: 32
bf16 values), so their tail is 64 bytes where the unpacked case has 48.
"""

import os

import pytest

from distributed_llm_dissemination_amd.models.catalog import make_workload
from distributed_llm_dissemination_amd.parallel.runtime import Runtime

MiB = 1 << 20
LAYERS = 5

pytestmark = pytest.mark.gpu


def session(gpu, size, pack):
    """One mode-1 session; returns (stats, HBM image per layer, chunk CRCs per layer, is_pinned per layer)."""
    cfg = make_workload(1, LAYERS, size, tier="host", chunk_bytes=MiB)
    kw = dict(pack=pack, pack_block=32) if pack != "none" else {}
    rt = Runtime(cfg, 0, engine="rccl", chunk_bytes=MiB, registry={0: "127.0.0.1:0"}, verify=True, **kw)
    try:
        res = rt.run(1, timeout=60)
        assert res.ok, res.error
        images = [rt.layer_tensor(l).cpu() for l in range(LAYERS)]
        crcs = [gpu.crc32c_chunks(rt.engine.device_ptr(l), rt.slot_sizes[l], rt.grid) for l in range(LAYERS)]
        return res.engine_stats, images, crcs
    finally:
        rt.close()


@pytest.mark.parametrize("pack", ["none", "fp8", "mxfp4", "mxfp6"])
def test_pageable_layers_stage_through_the_ring(gpu, pack, monkeypatch):
    size = 3 * MiB + (48 if pack == "none" else 64)
    monkeypatch.delenv("DISSEM_PINNED_LIMIT_BYTES", raising=False)
    stats0, images0, crcs0 = session(gpu, size, pack)
    assert stats0["host_bounce_bytes"] == 0
    # room for two more layers: layers 0 and 1 are pinned, 2, 3 and 4 pageable
    monkeypatch.setenv("DISSEM_PINNED_LIMIT_BYTES", str(gpu.HostBuffer.pinned_live_bytes() + 2 * size + size // 2))
    stats, images, crcs = session(gpu, size, pack)
    print(f"{pack}: host_bounce_bytes {stats['host_bounce_bytes']} (want {3 * size}), bytes_staged "
          f"{stats['bytes_staged']}, verify_chunks {stats['verify_chunks']}")
    assert stats["host_bounce_bytes"] == 3 * size
    assert stats["bytes_staged"] == stats0["bytes_staged"] == LAYERS * size
    assert stats["verify_failures"] == 0 and stats["verify_chunks"] == stats0["verify_chunks"] == LAYERS * 4
    assert stats["disk_direct_bytes"] == 0 and stats["disk_buffered_bytes"] == 0
    for l in range(LAYERS):
        assert bytes(images[l].numpy()) == bytes(images0[l].numpy()), l
    assert crcs == crcs0


def test_pointer_query_tells_pinned_from_pageable(gpu, monkeypatch):
    monkeypatch.delenv("DISSEM_PINNED_LIMIT_BYTES", raising=False)
    assert gpu.HostBuffer.pinned(MiB).is_pinned
    assert not gpu.HostBuffer.malloc(MiB).is_pinned
    live = gpu.HostBuffer.pinned_live_bytes()
    monkeypatch.setenv("DISSEM_PINNED_LIMIT_BYTES", str(live + MiB))
    under, over = gpu.HostBuffer.pinned(MiB), gpu.HostBuffer.pinned(MiB)
    assert under.is_pinned and not over.is_pinned
    assert gpu.HostBuffer.pinned_live_bytes() == live + MiB
    del under, over
    assert gpu.HostBuffer.pinned_live_bytes() == live
    monkeypatch.delenv("DISSEM_PINNED_LIMIT_BYTES")
    # A shared-memory segment registered with HIP is DMA-able, the same mapping
    # unregistered is not. Some machines (virtual ones) refuse to register
    # memory a process already has: there only the refusal itself, which must
    # leave no error behind for the next launch, and the unregistered answer
    # can be checked.
    name = f"dld_pagetest_{os.getpid()}"
    try:
        seg = gpu.HostBuffer.shared(name, MiB, True, True)
    except RuntimeError as e:
        assert "hipHostRegister" in str(e)
        seg = None
        print(f"hipHostRegister refused here: {e}")
    if seg is not None:
        assert seg.is_pinned
        del seg
    plain = gpu.HostBuffer.shared(name + "_u", MiB, True, False)
    assert not plain.is_pinned
    del plain
    dev = gpu.device_malloc(4096)
    try:
        gpu.fill_random(dev, 4096, 1)  # a launch right after: reports any error left behind
        gpu.device_synchronize()
    finally:
        gpu.device_free(dev)
