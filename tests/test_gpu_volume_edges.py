"""Scene.query_volumes on the MI355X where csrc/volume.hip's plan and addressing have edges: batches of more than 65 536 records (each
thread of volume_scan owns several workgroups), whole workgroups of records without a work item in front of, between and behind the
others, batches of 1, 255, 256, 257, 65 536 and 65 537 records, boxes and spheres that start and end at every residue around a run
boundary, and worlds that are not cubes (384 x 384 x 128 and 128 x 128 x 384), preloaded and streaming.  The records come from
tests/_box_cases.py, the expected results from test_gpu_volume.py's numpy model.  Every number is an integer, every comparison exact."""
import time

import numpy as np
import pytest

from _box_cases import (BIG_RECORDS, BIG_RUNS, BOX, HOLES, WORLDS, base_batch, big_batch, items_of, mixed_records, model_sweep, run_records, streaming_scene,
                        tall_sweeps, tiled, world_voxels, zero_item_records)
from _edit_model import all_device_words
from test_gpu_volume import assert_results, model_results, resident_cells

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def preloaded(bm, torch_cuda):
    """world -> a scene of it with every brick resident, built on first use"""
    scenes = {}

    def get(world):
        if world not in scenes:
            scenes[world] = bm.Scene.from_voxels(world_voxels(world))
        return scenes[world]

    yield get
    for s in scenes.values():
        s.close()


@pytest.fixture(scope="module")
def base(bm):
    """the base batch of 4099 records in the cubic world, its model, the zero-item records and theirs: computed once, left unchanged"""
    vox = world_voxels("cube")
    recs, zero = base_batch(bm), zero_item_records(bm, WORLDS["cube"])
    want, zero_want = model_results(bm, vox, recs), model_results(bm, vox, zero)
    assert (items_of(zero, WORLDS["cube"]) == 0).all() and (zero_want["solid"] == 0).all() and (zero_want["status"] == 1).sum() == 4
    assert (want["solid"] > 0).sum() > 1000 and (want["status"] == 1).sum() > 50 and ((recs["shape"] != BOX) & (want["solid"] > 0)).sum() > 100
    return recs, want, zero, zero_want


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_volume_edges.py took {time.time() - t0:.1f} s")


def query_both(scene, recs, want, what):
    assert_results(scene.query_volumes(recs).packed, want, what=what + " ")
    assert_results(scene.query_volumes(recs, any=True).packed, want, any_mode=True, what=what + " BM_VOLUME_ANY ")


@pytest.mark.parametrize("empty_tail", [False, True])
def test_more_than_65536_records(empty_tail, bm, torch_cuda, preloaded, base):
    t0 = time.time()
    recs, want = big_batch(bm, *base, empty_tail)
    n = len(recs)
    nblocks = (n + 255) // 256
    assert n == BIG_RECORDS >= 3 * 65536 + 77 and (nblocks + 255) // 256 == 4 and 4 * 255 >= nblocks, "volume_scan: 4 workgroups per thread, none for the last thread"
    per_block = np.add.reduceat(items_of(recs, WORLDS["cube"]), np.arange(0, n, 256))
    assert len(per_block) == nblocks
    for first, count in BIG_RUNS:
        assert (per_block[first:first + count] == 0).all() and (first == 0 or per_block[first - 1] > 0)
        assert per_block[first + count] > 0 or (empty_tail and first + count == nblocks - 1)
    assert per_block[0] == 0 and (per_block[300:303] == 0).all() and per_block[nblocks - 2] == 0, "workgroup 0, three in a row and the last full one are empty"
    assert (per_block[-1] == 0) == empty_tail and (per_block > 0).sum() >= nblocks - 7
    query_both(preloaded("cube"), recs, want, f"{n} records")
    print(f"{n} records, empty tail {empty_tail}: {time.time() - t0:.1f} s", flush=True)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536, 65537])
def test_small_batches(n, bm, torch_cuda, preloaded, base):
    recs, want = tiled(base[0], base[1], n)
    assert len(recs) == n and items_of(recs[:1], WORLDS["cube"])[0] > 0, "the first record has work items: a batch of one is not empty"
    query_both(preloaded("cube"), recs, want, f"{n} records")


@pytest.mark.parametrize("world", ["cube", "flat"])
def test_runs_and_shared_records(world, bm, torch_cuda, preloaded):
    t0 = time.time()
    dims = WORLDS[world]
    recs = run_records(bm, dims)
    items = items_of(recs, dims)
    lo, hi = recs["lo"][0::2, 0], recs["hi"][0::2, 0]
    for B in range(128, dims[0], 128):
        near = (lo >= B - 8) & (lo <= B + 8)
        assert set((lo[near] % 8).tolist()) == set(range(8)) and set((hi[near] % 8).tolist()) == set(range(8)), "every residue mod 8 around the run boundary"
    assert {0, 127} <= set((lo % 128).tolist()) and {0, 127} <= set((hi % 128).tolist()) and (hi % 128 == 0).sum() > 50
    assert {1, 2, 4, 5} <= set(items.tolist()), "records of 1, 2, 4 and 5 work items"
    want = model_results(bm, world_voxels(world), recs)
    assert (want["solid"][1::2] > 0).sum() > len(recs) // 4
    query_both(preloaded(world), recs, want, f"runs in the {world} world")
    print(f"runs {world}: {len(recs)} records, {time.time() - t0:.1f} s", flush=True)


@pytest.mark.parametrize("world", ["flat", "tall"])
def test_mixed_batch_in_a_world_that_is_no_cube(world, bm, torch_cuda, preloaded):
    t0 = time.time()
    dims, vox = WORLDS[world], world_voxels(world)
    recs = mixed_records(bm, np.random.default_rng(82 + len(world)), dims)
    want = model_results(bm, vox, recs)
    assert (want["status"] == 1).sum() >= 100 and (want["solid"] > 0).sum() > 1000
    scene = preloaded(world)
    got = scene.query_volumes(recs)
    assert_results(got.packed, want, what=f"{world} ")
    assert (got.unresolved == 0).all()
    whole = len(recs) - 1
    assert tuple(recs["lo"][whole]) == (0, 0, 0) and tuple(recs["hi"][whole]) == dims and recs["shape"][whole] == BOX
    zs, ys, xs = np.nonzero(vox)
    assert int(got.solid[whole]) == int(vox.sum(dtype=np.int64))
    assert tuple(got.lo[whole]) == (xs.min(), ys.min(), zs.min()) and tuple(got.hi[whole]) == (xs.max() + 1, ys.max() + 1, zs.max() + 1)
    assert_results(scene.query_volumes(recs, any=True).packed, want, any_mode=True, what=f"{world} BM_VOLUME_ANY ")
    print(f"mixed {world}: {len(recs)} records, {time.time() - t0:.1f} s", flush=True)


def test_streaming_flat_world_counts_what_is_resident(bm, torch_cuda):
    torch = torch_cuda
    t0 = time.time()
    dims, vox = WORLDS["flat"], world_voxels("flat")
    scene = streaming_scene(bm, torch, "flat")
    words = all_device_words(scene)
    resident = resident_cells(scene)
    assert resident.shape == (dims[2] // 8, dims[1] // 8, dims[0] // 8)
    rng = np.random.default_rng(83)
    (x0, x1), (y0, y1), (z0, z1) = HOLES["flat"]  # and boxes around the hole, whose walls are resident
    p = np.stack([rng.integers(x0 - 24, x1 + 12, 600), rng.integers(y0 - 24, y1 + 12, 600), rng.integers(z0 - 24, z1 + 12, 600)], 1)
    recs = np.concatenate([bm.volume_box(p, p + rng.integers(1, 25, p.shape)), mixed_records(bm, rng, dims)])
    want = model_results(bm, vox, recs, resident)
    print(f"streaming flat: {len(recs)} records, {(want['unresolved'] > 0).sum()} with unresolved cells, {(want['solid'] > 0).sum()} with resident solid voxels", flush=True)
    assert (want["unresolved"] > 0).sum() > 100 and (want["solid"] > 0).sum() > 100
    loads = scene.info()["stream_batches"]
    query_both(scene, recs, want, "streaming flat")
    assert np.array_equal(all_device_words(scene), words), "a volume query wrote an index word"
    assert scene.process_load_queue() == 0 and scene.info()["stream_batches"] == loads, "a volume query filed a brick request"
    scene.close()
    print(f"streaming flat: {time.time() - t0:.1f} s", flush=True)


def test_sweep_box_in_the_tall_world(bm, torch_cuda, preloaded):
    t0 = time.time()
    vox, Z = world_voxels("tall"), WORLDS["tall"][2]
    lo, hi, sign, dist = tall_sweeps()
    n = len(lo)
    axis = np.full(n, 2)
    d, unresolved = preloaded("tall").sweep_box(lo, hi, axis, sign, dist)
    assert (unresolved == 0).all()
    want = model_sweep(vox, lo, hi, axis, sign, dist)
    bad = np.nonzero(d != want)[0]
    assert len(bad) == 0, f"{len(bad)} sweeps differ, first {bad[0]}: {lo[bad[0]]} ... {hi[bad[0]]} sign {sign[bad[0]]} dist {dist[bad[0]]}: got {d[bad[0]]}, want {want[bad[0]]}"
    # what the moved boxes passed through, on z
    a, b = np.where(sign > 0, lo[:, 2], lo[:, 2] - want), np.where(sign > 0, hi[:, 2] + want, hi[:, 2])
    moved = want > 0
    for plane in (128, 256):
        assert (moved & (a < plane) & (b > plane)).sum() >= 20, f"too few sweeps pass z = {plane}"
    assert (moved & (b > Z)).sum() >= 20, "too few sweeps leave the world through its top"
    assert ((want < dist) & moved).sum() >= 20 and (want == dist).sum() >= 20 and (sign < 0).sum() >= 100
    print(f"sweep_box tall: {n} sweeps, {time.time() - t0:.1f} s", flush=True)
