"""A scene from the caller's own voxels on the MI355X (bm_scene_load_voxels): the device route (csrc/load.hip) builds exactly what the
generator and the host route build, for terrain and for content that is not terrain; the loaded scene renders like the oracle's, streams,
takes edits and answers ray queries like a generated one; and a load is ordered behind the stream that produced the volume.

Every comparison covers every supercell, every brick, every field byte and every ray.  Pool bases are not readable through the API as
numbers; they are compared through what they address: bm_scene_device_brick(sc, slot) reads arena[pool_base[sc] + slot]."""
import ctypes as C
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from _load_model import canonical_supercell
from test_gpu_edit import CAM, G, R_HI, R_LO, assert_radiance, assert_same, oracle_clear, orender, render

pytestmark = pytest.mark.gpu

BM_EINVAL = 10001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def terrain(bm, torch_cuda):
    """the generated 256^3 scene (preloaded) and its voxels"""
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    return scene, scene.voxels()


def supercells_of(scene):
    return range(scene.info()["supercells"])


def assert_same_world(a, b, device_bricks=True):
    """host words and bricks, device words and (through the pool bases) every device brick of two preloaded scenes"""
    assert a.info()["supercells"] == b.info()["supercells"]
    for sc in supercells_of(a):
        (wa, ba), (wb, bb) = a.host_supercell(sc), b.host_supercell(sc)
        assert np.array_equal(wa, wb), f"supercell {sc}: host words differ"
        assert np.array_equal(ba, bb), f"supercell {sc}: host bricks differ"
        da, db = a.device_indices(sc), b.device_indices(sc)
        assert np.array_equal(da, wa) and np.array_equal(db, wb), f"supercell {sc}: device words differ from the host words"
        if device_bricks:
            for slot in range(len(ba)):
                assert np.array_equal(a.device_brick(sc, slot), ba[slot]), f"supercell {sc} slot {slot}: device brick (first scene)"
                assert np.array_equal(b.device_brick(sc, slot), bb[slot]), f"supercell {sc} slot {slot}: device brick (second scene)"
    ia, ib = a.info(), b.info()
    for key in ("total_bricks", "resident_bricks", "pool_bytes", "index_bytes", "cube_field_bytes", "generated", "on_device"):
        assert ia[key] == ib[key], key
    assert ia["resident_bricks"] == ia["total_bricks"]


def assert_is_canonical(scene, volume):
    """words and bricks of every supercell equal the numpy model; device words equal them; every device brick equals its host brick"""
    sg = scene.info()["supergrid_xy"]
    total = 0
    for sc in supercells_of(scene):
        want_words, want_bricks = canonical_supercell(volume, sc % sg, (sc // sg) % sg, sc // (sg * sg))
        words, bricks = scene.host_supercell(sc)
        assert np.array_equal(words, want_words), f"supercell {sc}: words differ from the model"
        assert np.array_equal(bricks, want_bricks), f"supercell {sc}: bricks differ from the model"
        assert np.array_equal(scene.device_indices(sc), want_words)
        for slot in range(len(bricks)):
            assert np.array_equal(scene.device_brick(sc, slot), want_bricks[slot]), f"supercell {sc} slot {slot}"
        total += len(bricks)
    info = scene.info()
    assert info["total_bricks"] == total and info["resident_bricks"] == total and info["pool_bytes"] == 64 * total


def assert_field_is_exact(scene):
    dev, host = scene.device_cube_field(), scene.host_cube_field()
    assert np.array_equal(dev, host), f"{np.count_nonzero(dev != host)} field bytes differ"
    return dev


def hits_bits(hits):
    return np.ascontiguousarray(hits.packed).view(np.uint32)


def assert_distances(got, geometric):
    """Hit distances of axis-parallel rays between voxel centres and voxel faces.  The geometric distance is a multiple of 0.5 below 256,
    exact in fp32.  The walk (the reference's intersect_voxel, csrc/traverse.h process_candidate) measures the part inside the hit brick
    from the brick's entry point pushed kEpsilon = 0.001 voxels along the ray (o8 = entry * 8 - n * kEpsilon), so it reports the geometric
    distance less kEpsilon -- or the geometric distance itself when the hit voxel lies on the brick's entry face, where the pushed
    point is inside it.  Rounding: a handful of fp32 operations on coordinates below 256 (ulp 2^-15), allowed 4 ulps = 1.25e-4."""
    k_epsilon, tol = 0.001, 4 * 2.0 ** -15
    err = got.astype(np.float64) - geometric
    assert (err <= tol).all() and (err >= -k_epsilon - tol).all(), f"distance errors {err.min():.6f} ... {err.max():.6f}"


def other_content(size=G):
    """a volume that is not terrain: floating blobs, an all-solid supercell, overhangs, a single voxel in the far corner"""
    v = np.zeros((size, size, size), np.uint8)
    z, y, x = np.ogrid[:size, :size, :size]
    for (cx, cy, cz), r in (((60, 70, 200), 23), ((130, 40, 90), 17), ((126, 126, 126), 9), ((30, 200, 30), 30)):
        v[(x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r] = 200
    v[128:, 128:, 128:] = 1                 # supercell (1, 1, 1): 4096 bricks
    v[150:154, 20:120, 140:250] = 7         # a roof ...
    v[100:150, 20:24, 140:144] = 7          # ... on one leg: an overhang
    v[40:44, 150:230, 10:100] = 3           # a shelf with a hole in it
    v[40:44, 180:200, 40:60] = 0
    v[size - 1, size - 1, size - 1] = 255
    v[0, 0, 0] = 1
    return v


# ---------------------------------------------------------------- 1
def test_round_trip_equals_the_generated_scene(bm, orc, torch_cuda, terrain):
    torch = torch_cuda
    a, vox = terrain
    b = bm.Scene.from_voxels(torch.from_numpy(vox).to("cuda:0"))
    assert_same_world(a, b)
    field = assert_field_is_exact(b)
    assert np.array_equal(field, a.device_cube_field())
    assert np.array_equal(b.voxels(), vox)
    cam = bm.Camera(**CAM).update()
    fa, fb = render(bm, torch, a, cam), render(bm, torch, b, cam)
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and fa[2] == fb[2], "the loaded scene's frame differs from the generated scene's"
    w = orc.World(G, G)
    w.reset_device(True)
    want = orender(orc, w, cam)
    assert_same(fa, want)
    assert_same(fb, want)
    pack_ms, field_ms, mirror_ms = b.last_load_ms()
    assert pack_ms > 0 and field_ms > 0 and mirror_ms > 0
    b.close()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("content", ["terrain", "noise", "other"])
def test_host_route_equals_device_route(content, bm, torch_cuda, terrain):
    torch = torch_cuda
    if content == "terrain":
        vol = terrain[1]
    elif content == "noise":
        rng = np.random.default_rng(3)
        vol = np.where(rng.random((128, G, G)) < 0.004, rng.integers(1, 256, (128, G, G)), 0).astype(np.uint8)  # a world lower than it is wide
    else:
        vol = other_content()
    h = bm.Scene.from_voxels(vol)
    d = bm.Scene.from_voxels(torch.from_numpy(vol).to("cuda:0"))
    assert_same_world(h, d)
    assert np.array_equal(assert_field_is_exact(h), assert_field_is_exact(d))
    with pytest.raises(bm.BrickmapError):
        h.last_load_ms()  # device time exists for loads from device memory only
    h.close()
    d.close()


def test_volume_that_does_not_start_on_16_bytes(bm, torch_cuda):
    torch = torch_cuda
    vol = other_content()
    big = torch.zeros(vol.size + 64, dtype=torch.uint8, device="cuda:0")
    view = big[3:3 + vol.size].view(G, G, G)
    view.copy_(torch.from_numpy(vol))
    assert view.data_ptr() % 16 != 0
    scene = bm.Scene.from_voxels(view)
    assert_is_canonical(scene, vol)
    assert_field_is_exact(scene)
    scene.close()


# ---------------------------------------------------------------- 3
def test_content_that_is_not_terrain(bm, torch_cuda):
    torch = torch_cuda
    vol = other_content()
    scene = bm.Scene.from_voxels(torch.from_numpy(vol).to("cuda:0"))
    assert_is_canonical(scene, vol)
    assert len(scene.host_supercell(7)[1]) == 4096  # supercell (1, 1, 1)
    assert_field_is_exact(scene)
    assert np.array_equal(scene.voxels(), vol != 0)
    solid = vol != 0

    # axis-parallel rays from voxel centres of the top layer straight down, and of the x = 0 face along +x, wherever the start voxel is empty
    ys, xs = np.nonzero(~solid[G - 1])
    origins = np.stack([xs + 0.5, ys + 0.5, np.full(len(xs), G - 0.5)], 1).astype(np.float32)
    hits = scene.cast_rays(origins, np.tile(np.float32([0, 0, -1]), (len(xs), 1)))
    column = solid[:, ys, xs]                                  # [z, ray]
    any_solid = column.any(0)
    top = G - 1 - np.argmax(column[::-1], axis=0)              # highest solid z of the column
    assert np.array_equal(hits.level >= 0, any_solid)
    assert np.array_equal(hits.level[any_solid], np.full(any_solid.sum(), 2))
    assert np.array_equal(hits.voxel[any_solid], np.stack([xs, ys, top], 1)[any_solid])
    assert_distances(hits.distance[any_solid], (G - 0.5 - (top + 1))[any_solid])
    down = (origins, hits)
    assert np.isinf(hits.distance[~any_solid]).all()
    zs, ys = np.nonzero(~solid[:, :, 0])
    origins = np.stack([np.full(len(ys), 0.5), ys + 0.5, zs + 0.5], 1).astype(np.float32)
    hits = scene.cast_rays(origins, np.tile(np.float32([1, 0, 0]), (len(ys), 1)))
    row = solid[zs, ys, :]                                     # [ray, x]
    any_solid = row.any(1)
    first = np.argmax(row, axis=1)
    assert np.array_equal(hits.level >= 0, any_solid)
    assert np.array_equal(hits.voxel[any_solid], np.stack([first, ys, zs], 1)[any_solid])
    assert_distances(hits.distance[any_solid], (first - 0.5)[any_solid])

    # the same content the old way: generate, clear everything, set every voxel -- other slots, the same voxels, so the same walk
    old = bm.Scene(G, G, device=0).generate().preload_all()
    old.clear_box((0, 0, 0), (G, G, G))
    assert old.info()["total_bricks"] == 0
    z, y, x = np.nonzero(solid)
    coords = np.stack([x, y, z], 1).astype(np.int32)
    for k in range(0, len(coords), 1 << 18):
        old.set_voxels(coords[k:k + (1 << 18)], 1)
    assert np.array_equal(old.voxels(), solid)
    assert old.info()["total_bricks"] == scene.info()["total_bricks"]
    assert np.array_equal(old.device_cube_field(), scene.device_cube_field())
    rng = np.random.default_rng(11)
    n = 6000
    origins = rng.uniform(0, G, (n, 3)).astype(np.float32)
    directions = rng.normal(size=(n, 3)).astype(np.float32)
    got, want = scene.cast_rays(origins, directions), old.cast_rays(origins, directions)
    assert (want.level >= 0).sum() > n // 4
    assert np.array_equal(hits_bits(got), hits_bits(want)), f"{np.count_nonzero((hits_bits(got) != hits_bits(want)).any(-1))} rays differ"
    again = old.cast_rays(down[0], np.tile(np.float32([0, 0, -1]), (len(down[0]), 1)))
    assert np.array_equal(hits_bits(again), hits_bits(down[1])), "the axis-parallel rays differ between the two scenes"
    old.close()
    scene.close()


def test_the_empty_volume(bm, torch_cuda):
    torch = torch_cuda
    scene = bm.Scene.from_voxels(torch.zeros((G, G, G), dtype=torch.bool, device="cuda:0"))
    assert_is_canonical(scene, np.zeros((G, G, G), np.uint8))
    assert scene.info()["total_bricks"] == 0
    assert_field_is_exact(scene)
    assert not scene.voxels().any()
    rng = np.random.default_rng(5)
    hits = scene.cast_rays(rng.uniform(0, G, (2000, 3)).astype(np.float32), rng.normal(size=(2000, 3)).astype(np.float32))
    assert (hits.level == -1).all()
    acc, dbg, _ = render(bm, torch, scene, bm.Camera(**CAM).update())
    assert not ((dbg[..., 1] >> 8) & 1).any(), "a frame of the empty world hits something"
    scene.fill_box((10, 10, 10), (20, 20, 20))  # and it is live
    assert_field_is_exact(scene)
    assert scene.voxels().sum() == 1000
    scene.close()


# ---------------------------------------------------------------- 4
def carved_terrain(vox):
    """terrain minus a few boxes and spheres in what the camera sees: (the volume, what was removed)"""
    carve = np.zeros_like(vox)
    carve[R_LO[2]:R_HI[2], R_LO[1]:R_LO[1] + 30, R_LO[0]:R_HI[0]] = True
    carve[0:G, 120:136, 120:140] = True  # a shaft across the supercell border, down to the floor of the world
    z, y, x = np.ogrid[:G, :G, :G]
    for (cx, cy, cz), r in (((180, 120, 120), 28), ((128, 128, 100), 21), ((90, 150, 110), 13)):
        carve |= (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r
    removed = carve & vox
    assert removed.any()
    return vox & ~carve, removed


def test_loaded_scene_matches_the_edited_oracle_preloaded(bm, orc, torch_cuda, terrain):
    torch = torch_cuda
    vol, removed = carved_terrain(terrain[1])
    scene = bm.Scene.from_voxels(torch.from_numpy(vol).to("cuda:0"))
    w = orc.World(G, G)
    oracle_clear(w, removed)
    w.reset_device(True)
    cam = bm.Camera(**CAM).update()
    for primary in (True, False):
        assert_same(render(bm, torch, scene, cam, primary=primary), orender(orc, w, cam, primary=primary))
    pristine = orc.World(G, G)
    pristine.reset_device(True)
    assert not np.array_equal(orender(orc, w, cam)[1], orender(orc, pristine, cam)[1]), "the carving is not visible"
    scene.close()


@pytest.mark.parametrize("overlapped", [0, 1], ids=["blocking", "overlapped"])
def test_loaded_scene_matches_the_edited_oracle_streaming(overlapped, bm, orc, torch_cuda, terrain):
    torch = torch_cuda
    vol, removed = carved_terrain(terrain[1])
    scene = bm.Scene(G, G, device=0)
    scene.set_queue_capacity(1 << 16)
    scene.load_voxels(torch.from_numpy(vol).to("cuda:0"))
    scene.reset_residency().set_streaming_mode(overlapped)
    assert scene.info()["resident_bricks"] == 0
    w = orc.World(G, G)
    w.set_queue_cap(1 << 16)
    oracle_clear(w, removed)
    w.reset_device(False)
    cam = bm.Camera(**CAM).update()
    assert_same(render(bm, torch, scene, cam), orender(orc, w, cam))  # nothing resident: every brick requested the same way
    for _ in range(64):
        render(bm, torch, scene, cam)
        if scene.process_load_queue() == 0 and scene.process_load_queue() == 0:
            break
    else:
        pytest.fail("streaming did not reach a steady state")
    w.reset_device(True)
    assert_same(render(bm, torch, scene, cam), orender(orc, w, cam), counters=False)
    assert not scene.info()["failed"]
    scene.preload_all()  # and back: the host world is authoritative
    assert_same(render(bm, torch, scene, cam), orender(orc, w, cam))
    scene.close()


# ---------------------------------------------------------------- 5
def test_a_loaded_scene_is_live(bm, torch_cuda, terrain):
    torch = torch_cuda
    vol = other_content()
    scene = bm.Scene.from_voxels(torch.from_numpy(vol).to("cuda:0"))
    want = vol != 0
    z, y, x = np.ogrid[:G, :G, :G]
    scene.carve_sphere((160, 160, 160), 40)  # into the all-solid supercell, across its faces
    want &= ~((x - 160) ** 2 + (y - 160) ** 2 + (z - 160) ** 2 <= 40 * 40)
    assert_field_is_exact(scene)
    assert np.array_equal(scene.voxels(), want)
    scene.fill_box((5, 100, 60), (120, 140, 75))
    want[60:75, 100:140, 5:120] = True
    assert_field_is_exact(scene)
    assert np.array_equal(scene.voxels(), want)
    info = scene.info()
    assert info["resident_bricks"] == info["total_bricks"] and not info["failed"]
    cam = bm.Camera(**CAM).update()
    edited = bm.Scene.from_voxels(want)  # the edited content, loaded: other slots, the same voxels
    fa, fb = render(bm, torch, scene, cam), render(bm, torch, edited, cam)
    assert np.array_equal(fa[1], fb[1])
    assert_radiance(fa[0], fb[0])
    edited.close()

    # a second load replaces the world: nothing of the first one is left in the accounts, and frames see only the new one
    gen, tvox = terrain
    scene.load_voxels(torch.from_numpy(tvox).to("cuda:0"))
    assert_same_world(gen, scene)
    assert scene.info()["brick_bytes"] == gen.info()["brick_bytes"], "the arena still holds the first world's bricks"
    assert_field_is_exact(scene)
    fa, fb = render(bm, torch, scene, cam), render(bm, torch, gen, cam)
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and fa[2] == fb[2]
    scene.load_voxels(vol)  # ... and once more through the host route
    assert_is_canonical(scene, vol)
    assert_field_is_exact(scene)
    scene.close()


# ---------------------------------------------------------------- 6
def test_load_is_ordered_behind_the_stream_that_made_the_volume(bm, torch_cuda):
    torch = torch_cuda
    vol = other_content()
    src = torch.from_numpy(vol).to("cuda:0")
    dst = torch.zeros_like(src)
    busy = torch.randn((4096, 4096), device="cuda:0")
    scene = bm.Scene(G, G, device=0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        for _ in range(20):  # work that keeps the side stream busy while the host runs ahead
            busy = busy @ busy * 1e-3
        torch.where(src != 0, src, torch.zeros_like(src), out=dst)
        scene.load_voxels(dst)  # on the side stream, no synchronisation in between
    host = bm.Scene.from_voxels(vol)
    assert_same_world(host, scene)
    assert np.array_equal(scene.device_cube_field(), host.device_cube_field())
    # ... and with the stream given by handle while another stream is current
    dst.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            busy = busy @ busy * 1e-3
        torch.where(src != 0, src, torch.zeros_like(src), out=dst)
    scene.load_voxels(dst, stream=side.cuda_stream)
    assert_same_world(host, scene)
    host.close()
    scene.close()


# ---------------------------------------------------------------- 7
def wide_volume(torch, size, height):
    """slabs, pillars and blobs with long empty runs between them, made on the device"""
    v = torch.zeros((height, size, size), dtype=torch.uint8, device="cuda:0")
    v[:8, :, :1024] = 1                                   # a ground slab along the x = 0 side
    v[64:72, size - 1100:size - 1000, 1200:1300] = 9    # a hanging slab
    x = torch.arange(size, device="cuda:0")
    pillar = (x % 256 < 16) & (x >= size - 600)
    v[:, pillar[:, None] & pillar[None, :]] = 2           # pillars in the far corner, floor to ceiling
    z, y, xx = torch.arange(height, device="cuda:0")[:, None, None], torch.arange(128, device="cuda:0")[None, :, None], torch.arange(128, device="cuda:0")[None, None, :]
    for (cx, cy), r in (((1500, 300), 40), ((size // 2, size // 2), 55), ((300, size - 200), 25), ((size - 64, 64), 60)):
        blob = ((xx - 64) ** 2 + (y - 64) ** 2 + (z - height // 2) ** 2 <= r * r).to(torch.uint8) * 5
        v[:, cy - 64:cy + 64, cx - 64:cx + 64] |= blob
    v[height - 1, size - 1, size - 1] = 1
    return v


def test_grid_wider_than_one_field_pass_reaches(bm, torch_cuda):
    torch = torch_cuda
    size, height = 4096, 128
    free, _ = torch.cuda.mem_get_info(0)
    if free < 12 << 30:  # the volume, the temporaries that build it, two scenes
        size = 2176     # 272 brick cells across: still wider than the 254 cells a pass reaches
        warnings.warn(f"only {free >> 20} MiB of device memory free: the wide-grid load test runs on {size} x {size} x {height} instead of 4096 x 4096 x 128")
    dev = wide_volume(torch, size, height)
    assert size // 8 > 254
    d = bm.Scene.from_voxels(dev)
    vol = dev.cpu().numpy()
    del dev
    h = bm.Scene.from_voxels(vol)
    assert d.info()["total_bricks"] > 0
    # words and bricks: the device route's host world is the read-back of its index grid and arena
    assert_same_world(h, d, device_bricks=False)
    field = d.device_cube_field()
    assert np.array_equal(field, d.host_cube_field()), f"{np.count_nonzero(field != d.host_cube_field())} field bytes differ"
    assert np.array_equal(field, h.device_cube_field())
    # the volume is what the case asks for: empty runs longer than the 254 cells a pass reaches, along x and along y (the x and y passes
    # cap their runs there; the cubes themselves cannot be larger than the grid is high)
    occupied = vol.reshape(height // 8, 8, size // 8, 8, size // 8, 8).any(axis=(1, 3, 5))
    assert not occupied[8, 100, :].any() and not occupied[8, :size // 8 - 80, 200].any() and size // 8 - 80 > 254
    assert field[:, 1:-1, 1:-1, 1:-1].max() == height // 8
    sg = d.info()["supergrid_xy"]
    for sc in (0, sg - 1, sg * sg - 1, (sg // 2) * sg + sg // 2):  # spot checks against the model (every supercell is compared with the host route above)
        want_words, want_bricks = canonical_supercell(vol, sc % sg, (sc // sg) % sg, sc // (sg * sg))
        words, bricks = d.host_supercell(sc)
        assert np.array_equal(words, want_words) and np.array_equal(bricks, want_bricks)
        for slot in range(len(bricks)):
            assert np.array_equal(d.device_brick(sc, slot), want_bricks[slot])
    h.close()
    d.close()


# ---------------------------------------------------------------- 8
def test_refusals_leave_the_scene_as_it_was(bm, torch_cuda, terrain):
    torch = torch_cuda
    from brickmap_amd import _lib
    L = _lib.load()
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    cam = bm.Camera(**CAM).update()
    before, info = render(bm, torch, scene, cam), scene.info()
    host = np.ones((G, G, G), np.uint8)
    dev = torch.ones((G, G, G), dtype=torch.uint8, device="cuda:0")
    n = host.size
    calls = [
        (host.ctypes.data, n - 1, _lib.BM_VOXELS_HOST),      # wrong byte counts
        (host.ctypes.data, n + 1, _lib.BM_VOXELS_HOST),
        (dev.data_ptr(), n // 2, _lib.BM_VOXELS_DEVICE),
        (host.ctypes.data, 0, _lib.BM_VOXELS_HOST),
        (None, n, _lib.BM_VOXELS_HOST),                      # null
        (None, n, _lib.BM_VOXELS_DEVICE),
        (host.ctypes.data, n, 2),                            # unknown `where`
        (dev.data_ptr(), n, -1),
        (host.ctypes.data, n, _lib.BM_VOXELS_DEVICE),        # host memory offered as device memory
    ]
    for ptr, size, where in calls:
        assert L.bm_scene_load_voxels(scene.gpuScene, C.c_void_p(ptr), size, where, None) == BM_EINVAL, (size, where)
        assert L.bm_last_error_string()
    for bad in (np.ones((G, G, 2 * G), np.uint8)[:, :, ::2], np.ones((G, G, G), np.float32), np.ones((128, G, G), np.uint8), dev[:, :, :128]):
        with pytest.raises(ValueError):
            scene.load_voxels(bad)
    assert scene.info() == info
    assert_same_world(terrain[0], scene)
    assert np.array_equal(scene.device_cube_field(), terrain[0].device_cube_field())
    after = render(bm, torch, scene, cam)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    # a scene that holds no world yet refuses the same way and can still be loaded
    fresh = bm.Scene(G, G, device=0)
    assert L.bm_scene_load_voxels(fresh.gpuScene, C.c_void_p(host.ctypes.data), n - 1, _lib.BM_VOXELS_HOST, None) == BM_EINVAL
    assert L.bm_scene_load_voxels(None, C.c_void_p(host.ctypes.data), n, _lib.BM_VOXELS_HOST, None) == BM_EINVAL
    assert not fresh.info()["generated"]
    fresh.load_voxels(dev)
    assert fresh.info()["total_bricks"] == (G // 8) ** 3
    fresh.close()
    scene.close()


def test_headless_main_renders_a_volume_file(bm, torch_cuda, tmp_path):
    exe = os.path.join(ROOT, "examples", "headless_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    vol = other_content()
    path = tmp_path / "volume.raw"
    vol.tofile(path)
    out = tmp_path / "frame.ppm"
    r = subprocess.run([exe, "--voxels", str(path), "256", "256", "160", "96", "2", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    total = sum(len(canonical_supercell(vol, sc & 1, (sc >> 1) & 1, sc >> 2)[1]) for sc in range(8))
    m = re.search(r"(\d+) of (\d+) bricks resident", r.stdout)
    assert m and int(m.group(1)) == total and int(m.group(2)) == total, r.stdout
    assert out.stat().st_size == len(b"P6\n160 96\n255\n") + 160 * 96 * 3
    (tmp_path / "short.raw").write_bytes(b"\x01" * 1000)
    r = subprocess.run([exe, "--voxels", str(tmp_path / "short.raw"), "256", "256", "160", "96", "2", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "does not hold" in r.stderr
