"""tiled_depth_grid.py on a machine without a GPU: the table, the proofs and the discrimination checks
behind test_gpu_tiled_depth_grid.py, all on the reference alone.

The table is what it claims: from BM, BN (the bindings) and 256 CUs every case's mblocks, nblocks, nwg,
q8, r8, nsteps and tail are computed the way the launcher and the kernel compute them, and the step
totals 2 (no tail), 4, 5, 32, 33, 64, 224, 416, the remainders r8 = 0, 1, 7, a grid of exactly 2 CUs
and one beyond 8 CUs all occur - a retune of the tile fails here first. Every exact case is exact:
Built.prove, a condition on the inputs and no measurement. The inputs discriminate: removing the
products of any one K step, the tail included, changes an element of every workgroup tile of the
expectation; any two workgroup tiles of it differ; a Python model of the XCD remap is a bijection on
range(nwg) for every nwg of the table (the device code itself is held by the GPU file's exact values
and guard buffer). And every case runs through the ops' CPU route against the same float64
expectation: equality (gated: check_exact_regimes) on the exact cases, K 2^-23 sum |x w| on the random
ones, as the older host files have it."""
import numpy as np
import pytest
import torch

import tiled_depth_grid as tdg
from test_gpu_mxfp4_swiglu import check_exact_regimes

F32 = dict(out_dtype=torch.float32)
ALL_CASES = [(v, g, c) for v in tdg.VARIANTS for g in (False, True) for c in tdg.cases(v, g)]


def test_the_table_is_what_it_claims():
    assert tdg.CUS == 256 and len(tdg.EXACT) == len(ALL_CASES) == 4 * (12 + 6) + 6 + 3
    geo = [tdg.geometry(v, c) for v, _, c in ALL_CASES]
    assert {g["total_steps"] for g in geo} >= {2, 4, 5, 32, 33, 64, 224, 416}
    assert any(g["nsteps"] == 2 and g["tail"] == 0 for g in geo)  # the first even total without a tail step
    assert any(g["nsteps"] % 2 == 1 and g["tail"] for g in geo) and any(g["nsteps"] % 2 == 0 and g["tail"] for g in geo)
    assert {g["r8"] for g in geo} >= {0, 1, 7}
    assert any(g["nwg"] == 2 * tdg.CUS for g in geo) and any(g["nwg"] > 8 * tdg.CUS for g in geo)
    for v in tdg.VARIANTS:
        bm, bn = tdg.tile(v)
        for gated in (False, True):
            by = {c.name: (c, tdg.geometry(v, c)) for c in tdg.cases(v, gated)}
            for name, (c, g) in by.items():
                assert c.gated == gated and c.k % 32 == 0 and c.n % 16 == 0
                assert g["cols"] == (bn // 2 if gated else bn) and g["nwg"] == g["mblocks"] * g["nblocks"]
                if c.tag == "depth":
                    assert (c.m, g["mblocks"], g["nblocks"], g["nwg"]) == (bm + 1, 2, 2, 4) and name == f"K={c.k}"
                if c.tag == "grid":
                    assert (c.k, g["nsteps"], g["tail"]) == (416, 3, 1)
            if v == "w4a8":
                want_k = [448, 8160] if gated else [448, 4192, 28672]
            else:
                want_k = [448, 8160, 28672] if gated else tdg.DEPTH_K
            assert [c.k for c, _ in by.values() if c.tag == "depth"] == want_k
            steps = {k: (k >> 7, (k >> 5) & 3) for k in tdg.DEPTH_K}
            assert steps == {256: (2, 0), 448: (3, 2), 640: (5, 0), 4096: (32, 0), 4192: (32, 3), 8160: (63, 3),
                             28672: (224, 0), 53248: (416, 0)}
            if v == "w4a8":
                want_grids = ["G2"] if gated else ["G1", "G2"]
            else:
                want_grids = ["G1", "G2"] if gated else ["G1", "G2", "G3"]
            assert [n for n in ("G1", "G2", "G3") if n in by] == want_grids
            if "G1" in by:
                c, g = by["G1"]
                assert (g["mblocks"], g["nblocks"], g["nwg"], g["r8"]) == (2, 256, 2 * tdg.CUS, 0)
                assert c.m % bm == 0 and c.n % g["cols"] == 0  # no partial tile anywhere
            c, g = by["G2"]
            assert (g["mblocks"], g["nblocks"], g["nwg"], g["q8"], g["r8"]) == (3, 683, 8 * tdg.CUS + 1, 256, 1)
            assert c.m == 2 * bm + 5 and g["nwg"] > 4 * tdg.CUS
            if "G3" in by:
                c, g = by["G3"]
                assert (g["mblocks"], g["nblocks"], g["nwg"], g["r8"]) == (5, 51, 255, 7) and c.m == 4 * bm + 7
            if "both" in by:
                c, g = by["both"]
                assert g["nsteps"] >= 32 and g["nwg"] >= 33 and c.m % bm and c.n % g["cols"]
            assert ("both" in by) == (not (gated and v == "w4a8"))
    assert max(c.n * c.k * (2 if c.gated else 1) for _, _, c in ALL_CASES) < 70e6  # elements of the largest layer


def test_the_remap_model_is_a_bijection():
    counts = sorted({tdg.geometry(v, c)["nwg"] for v, _, c in ALL_CASES})
    assert {4, 255, 512, 2049} <= set(counts)
    for nwg in counts + list(range(1, 70)):
        lids = [tdg.remap(b, nwg) for b in range(nwg)]
        assert sorted(lids) == list(range(nwg)), nwg
        # ids b, b + 8, ... (one XCD) become consecutive
        for xcd in range(min(8, nwg)):
            mine = [tdg.remap(b, nwg) for b in range(xcd, nwg, 8)]
            assert mine == list(range(mine[0], mine[0] + len(mine)))


def _every_step_shows_in_every_tile(b):
    bm, cols = b.geo["bm"], b.geo["cols"]
    steps = tdg.steps_of(b.k)
    assert len(steps) == b.geo["total_steps"]
    for w in b.ws:
        for k0, k1 in steps:
            part = b.xf[:, k0:k1] @ w[:, k0:k1].T  # what the expectation loses without this step
            seen = tdg.tiles_any(part != 0, bm, cols)
            assert seen.shape == (b.geo["mblocks"], b.geo["nblocks"]) and seen.all(), (k0, np.argwhere(~seen)[:4])


def _any_two_tiles_differ(b):
    for want in b.wants():
        d = tdg.tile_digests(want, b.geo["bm"], b.geo["cols"])
        assert len(d) == b.geo["nwg"] == len(set(d))


@pytest.mark.parametrize("variant,case", tdg.EXACT, ids=[tdg.exact_id(p) for p in tdg.EXACT])
def test_exact_case_is_exact_discriminates_and_agrees_with_the_cpu_route(variant, case):
    b = tdg.Built(variant, case)
    assert b.offs[0] > 0 and all(o % 32 == 0 for o in b.offs) and b.total >= b.offs[-1] + b.n * b.k + 64
    b.prove()
    _every_step_shows_in_every_tile(b)
    _any_two_tiles_differ(b)
    y = b.run("cpu", **F32)
    assert y.dtype == torch.float32 and tuple(y.shape) == (b.m, b.n)
    if b.gated:
        check_exact_regimes(y, *b.wants())
    else:
        assert np.array_equal(y.numpy().astype(np.float64), b.wants()[0])


def test_the_deepest_cases_need_the_narrowed_images():
    """At K = 53248 the closed form holds for MXFP6 and fp8 only on the narrowed image, for MXFP4 on
    the ordinary one with x in [-2, 2]; up to K = 4096 every format keeps x in [-8, 8] and its
    ordinary image."""
    for f in tdg.FORMATS:
        hi, wmax, extra = tdg.level(f, 53248)
        assert hi == 2 and (wmax, bool(extra)) == ((12.0, False) if f.name == "mxfp4" else (7.5, True))
        assert hi * wmax * 53248 < 2.0 ** 24 * f.uw
        assert tdg.level(f, 4096)[0] == 8 and not tdg.level(f, 4096)[2]
        for k in tdg.DEPTH_K + [416, 8192]:
            assert tdg.level(f, k)  # none is out of reach


RANDOM = [(v, s, False) for v in tdg.VARIANTS for s in range(2)] + [("w4a8", 1, True)]


@pytest.mark.parametrize("variant,shape,outliers", RANDOM, ids=[f"{v}-{s}" + ("-outliers" if o else "") for v, s, o in RANDOM])
def test_random_case_on_the_cpu_route(variant, shape, outliers):
    m, n, k = tdg.random_shapes(variant)[shape]
    assert (m, k) == (tdg.tile(variant)[0] + 1, (8160, 28672)[shape]) and tdg.geometry(
        variant, tdg.Case("r", "depth", False, m, n, k))["nwg"] == 4
    c = tdg.Random(variant, m, n, k, "cpu", outliers)
    if outliers:  # products 2^14 and more apart inside groups of 8 consecutive k
        e = np.frexp(np.abs(c.x.float().numpy()).reshape(m, -1, 8))[1]
        assert ((e.max(-1) - e.min(-1)) >= 14).mean() > 0.1
    err = np.abs(c.run("cpu", **F32).numpy().astype(np.float64) - c.want)
    print(variant, (m, n, k), "max err / bound", float((err / c.bound).max()))
    assert (err <= c.bound).all()
