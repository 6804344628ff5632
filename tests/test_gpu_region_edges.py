"""Scene.write_region / Scene.read_region on the MI355X at every edge of csrc/region.hip's arithmetic: every pair of 16-byte chunk
residues of lo.x and hi.x, every pair of cell residues on y and z, boxes inside one chunk, onto and across the run boundary at x = 128,
across every supercell boundary, clipped by each face, outside and around the world -- in a flat world (3 x 3 x 1 supercells), a tall
one (1 x 1 x 3) and a cube (2 x 2 x 2), through the aligned and the general instantiation, and in streaming scenes (region_patch).
The cases come from tests/_box_cases.py (tests/test_box_cases_host.py checks what they cover).  Every comparison is exact."""
import time

import numpy as np
import pytest

from _box_cases import (LOADED, ROUTES, SWEEPS, WORLDS, Slab, assert_route, box_cells, cell_grid, model_read, region_cases, streaming_scene,
                        volume_for, world_voxels)
from _edit_model import all_device_words, assert_device_world
from test_region_host import model_write

pytestmark = pytest.mark.gpu
CANARY = 0xC9


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def preloaded(bm, torch_cuda):
    """world -> a scene of it with every brick resident, built on first use; the read tests share them and leave them as they are"""
    scenes = {}

    def get(world):
        if world not in scenes:
            scenes[world] = bm.Scene.from_voxels(world_voxels(world))
        return scenes[world]

    yield get
    for s in scenes.values():
        s.close()


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_region_edges.py took {time.time() - t0:.1f} s")


def shape_of(lo, hi):
    return (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])


def whole_world(scene, route, torch):
    """the whole world read on the device through one instantiation: the general one gets an odd row pitch"""
    X, Z = scene.grid_size, scene.grid_height
    if route == "aligned":
        out = torch.empty((Z, X, X), dtype=torch.uint8, device="cuda:0")
    else:
        out = torch.empty((Z, X, X + 1), dtype=torch.uint8, device="cuda:0")[:, :, 1:]
    return scene.read_region((0, 0, 0), (X, X, Z), out=out).cpu().numpy()


@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("world", list(WORLDS))
def test_writes(world, route, sweep, bm, torch_cuda):
    torch = torch_cuda
    t0 = time.time()
    model = world_voxels(world).copy()
    scene = bm.Scene.from_voxels(model)
    slab = Slab(torch, route, 0xEE)  # non-zero all round the slice: a load outside the box would show as solid voxels
    rng = np.random.default_rng(len(world) + 10 * len(route) + 100 * len(sweep))
    cases = region_cases(world, route, sweep)
    writes = 0
    for i, (lo, hi) in enumerate(cases):
        shape = shape_of(lo, hi)
        for op in ("replace", "set", "clear") if sweep == "x" and i % 4 == 0 else ("replace",):
            V = volume_for(rng, shape, 0.3 if max(shape) > 100 else 0.5)
            big, view, _ = slab.view(shape, i)
            view.copy_(torch.from_numpy(V))
            assert_route(bm, route, lo, view)
            scene.write_region(lo, view, op)
            model = model_write(model, lo, V, op)
            view.fill_(0xEE)
            glo, ghi = tuple(v - 16 for v in lo), tuple(v + 16 for v in hi)  # the box grown by 16 voxels, clipped by the library
            got = scene.read_region(glo, ghi, device=True).cpu().numpy()
            want = model_read(model, glo, ghi)
            assert np.array_equal(got, want), f"case {i} {op} {lo} ... {hi}: {np.count_nonzero(got != want)} voxels around the box differ from the model"
            writes += 1
    assert_device_world(scene, model)
    dev, host = scene.device_cube_field(), scene.host_cube_field()
    assert np.array_equal(dev, host), f"{np.count_nonzero(dev != host)} field bytes differ from the host build"
    for r in ROUTES:
        assert np.array_equal(whole_world(scene, r, torch), model), f"the whole world read through the {r} instantiation"
    assert np.array_equal(scene.voxels().view(np.uint8), model)
    scene.close()
    print(f"writes {world} {route} {sweep}: {len(cases)} boxes, {writes} writes, {time.time() - t0:.1f} s", flush=True)


@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("world", list(WORLDS))
def test_reads(world, route, sweep, bm, torch_cuda, preloaded):
    torch = torch_cuda
    t0 = time.time()
    scene, model = preloaded(world), world_voxels(world)
    slab = Slab(torch, route, CANARY)
    cases = region_cases(world, route, sweep)
    for i, (lo, hi) in enumerate(cases):
        big, view, sl = slab.view(shape_of(lo, hi), i)
        assert_route(bm, route, lo, view)
        assert scene.read_region(lo, hi, out=view) is view
        got = big.cpu().numpy()
        view.fill_(CANARY)
        want = np.full(tuple(big.shape), CANARY, np.uint8)
        want[sl] = model_read(model, lo, hi)
        bad = got != want
        assert not bad.any(), f"case {i} {lo} ... {hi}: {np.count_nonzero(bad[sl])} voxels of the box differ from the model, {np.count_nonzero(bad) - np.count_nonzero(bad[sl])} bytes outside it were written"
        host = np.full(tuple(big.shape), CANARY, np.uint8)
        assert scene.read_region(lo, hi, out=host[sl]) is not None
        assert np.array_equal(host, got), f"case {i} {lo} ... {hi}: the host read into a slice differs from the device read"
    print(f"reads {world} {route} {sweep}: {len(cases)} boxes, {time.time() - t0:.1f} s", flush=True)


@pytest.mark.parametrize("world", ["cube", "flat"])
def test_streaming_reads(world, bm, torch_cuda):
    """region_patch: device reads of a scene that holds some of the bricks give the model whatever is resident"""
    torch = torch_cuda
    t0 = time.time()
    scene, model = streaming_scene(bm, torch, world), world_voxels(world)
    info = scene.info()
    words = all_device_words(scene)
    loaded = cell_grid((words & np.uint32(LOADED)) != 0, info)
    missing = cell_grid(words != 0, info) & ~loaded  # non-empty, not resident
    loads = info["stream_batches"]
    boxes = patched = unpacked = 0
    for route in ROUTES:
        for sweep in ("x", "y", "z"):
            for i, (lo, hi) in enumerate(region_cases(world, route, sweep)):
                got = scene.read_region(lo, hi, device=True).cpu().numpy()
                want = model_read(model, lo, hi)
                assert np.array_equal(got, want), f"{route} {sweep} case {i} {lo} ... {hi}: {np.count_nonzero(got != want)} voxels differ from the model"
                boxes += 1
                patched += bool(box_cells(missing, lo, hi).any())
                unpacked += bool(box_cells(loaded, lo, hi).any())
    print(f"streaming reads {world}: {boxes} boxes, {patched} over a non-resident brick, {unpacked} over a resident one, "
          f"{info['resident_bricks']} of {info['total_bricks']} bricks resident, {time.time() - t0:.1f} s", flush=True)
    assert 4 * patched >= boxes, "too few boxes overlap a brick that is not resident: the case shows little of region_patch"
    assert 4 * unpacked >= boxes, "too few boxes overlap a resident brick: the case shows little of region_unpack next to region_patch"
    assert np.array_equal(all_device_words(scene), words), "a read wrote an index word"
    assert scene.process_load_queue() == 0 and scene.info()["stream_batches"] == loads, "a read filed a brick request"
    scene.close()
