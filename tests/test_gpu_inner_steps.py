"""The walk's two innermost bodies on the MI355X (brickmap_amd/csrc/steps.h: the Amanatides-Woo move and the packed cell of the brick
walk with its one-word occupancy test), against the CPU oracle, on the smallest worlds the builder accepts: a 128^3 world (one
supercell) and a tall 128 x 128 x 256 one, whose cube field has another slice pitch.

Frames: the ordered instrumented frame (hit records bit for bit, all eight traversal counters), the production helper-lane frame
(ray digest), and (chunk, sample) items at 2 spp.  Ray queries: axis-aligned and diagonal directions from origins on voxel faces,
cell faces and brick corners and from outside the box -- the rays on which tmax ties, -0.0 start values and first-cell hits occur;
a random frame almost never produces them.
"""
import itertools

import numpy as np
import pytest

from test_gpu_parity import assert_radiance, assert_ray_digest, cameras, gpu_render, oracle_sample_digest
from test_gpu_query import INT_MAX, assert_same_hits, oracle_hits

pytestmark = pytest.mark.gpu

W = H = 64
DIMS = [(128, 128), (128, 256)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module", params=DIMS, ids=["cube128", "tall128x256"])
def small_world(request, bm, orc, torch_cuda):
    G, GH = request.param
    scene = bm.Scene(G, GH, device=0).generate().preload_all()
    world = orc.World(G, GH)
    world.reset_device(True)
    cam, ocam = cameras(bm, orc, G, pos=(G / 2, G / 8, 0.8 * GH))
    yield G, GH, scene, world, cam, ocam
    scene.close()


def test_frames_match_the_oracle(bm, orc, torch_cuda, small_world):
    G, GH, scene, world, cam, ocam = small_world
    world.reset_device(True)
    p = bm.FrameParams(W, H, spp=1, max_bounces=3, flags=bm.BM_FLAG_COUNTERS)
    scene.counters_reset()
    acc, dbg = gpu_render(bm, torch_cuda, scene, cam, p)  # ordered instrumented frame; the production frames are compared inside
    oacc, odbg, ocnt, _ = world.render(ocam, orc.make_frame(W, H, spp=1, max_bounces=3))
    assert ocnt["brick_tests"] > 1000 and ocnt["voxel_steps"] > 5 * ocnt["brick_tests"] and ocnt["index_loads"] > 10000  # both bodies run
    assert np.array_equal(dbg, odbg), f"{np.count_nonzero((dbg != odbg).any(-1))} pixels with different hit records"
    assert scene.counters() == ocnt
    assert_ray_digest(world)  # the helper-lane frame (the timed instantiation family), ray by ray
    assert_radiance(acc, oacc)
    assert np.all(acc[..., 3] == 1)


def test_sample_items_match_the_oracle(bm, orc, torch_cuda, small_world):
    G, GH, scene, world, cam, ocam = small_world
    torch = torch_cuda
    world.reset_device(True)
    p = bm.FrameParams(W, H, spp=2, max_bounces=3, flags=bm.BM_FLAG_SAMPLE_ITEMS)
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    dbg = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda:0")
    scene.render(cam, p, acc, debug=dbg)
    plain = torch.zeros_like(acc)
    scene.render(cam, p, plain)  # the production instantiation in the same mode
    torch.cuda.synchronize()
    want = oracle_sample_digest(orc, world, ocam, W, H, 2)
    assert np.array_equal(dbg.cpu().numpy().view(np.uint32), want), "sample-item digest differs from the oracle"
    oacc, _, _, _ = world.render(ocam, orc.make_frame(W, H, spp=2, max_bounces=3))
    a, b = acc.cpu().numpy(), plain.cpu().numpy()
    assert np.array_equal(a[..., 3], b[..., 3]) and np.array_equal(a[..., 3], oacc[..., 3])
    assert_radiance(a, oacc)
    assert_radiance(b, oacc)


def special_rays(bm, G, GH):
    """26 directions (axes, face diagonals, space diagonals, every sign) from origins on voxel faces, cell faces, brick corners, voxel
    centres (three-way ties along the diagonals) and outside the box."""
    dirs = []
    for d in itertools.product((-1.0, 0.0, 1.0), repeat=3):
        n = sum(abs(c) for c in d)
        if n:
            dirs.append(np.array(d, np.float32) * (np.float32(1.0) / np.sqrt(np.float32(n))))  # equal components stay equal: exact ties
    top = 0.75 * GH
    origins = [
        (40.0, 33.5, top), (41.25, 64.0, top - 3.0), (50.5, 20.25, float(int(top))),      # on an integer voxel face (x / y / z)
        (64.0, 40.5, top), (30.25, 48.0, top), (70.5, 21.75, float(8 * int(top / 8))),    # on a brick-cell face
        (64.0, 64.0, float(8 * int(top / 8))), (32.0, 96.0, top), (8.0, 8.0, 8.0),        # brick corners (two and three faces at once)
        (60.5, 60.5, top + 0.5), (20.5, 100.5, 0.5 * GH + 0.5),                           # voxel centres
        (-20.0, 64.5, 0.5 * GH), (64.5, G + 30.0, 0.6 * GH), (70.25, 60.0, GH + 40.0),    # outside the box
        (-16.0, -16.0, -16.0), (G + 16.0, G + 16.0, GH + 16.0),                           # outside, on the long diagonal through corners
    ]
    o = np.repeat(np.array(origins, np.float32), len(dirs), axis=0)
    d = np.tile(np.array(dirs, np.float32), (len(origins), 1))
    return bm.pack_rays(o, d)


def test_ray_queries_on_faces_corners_and_diagonals(bm, orc, torch_cuda, small_world):
    G, GH, scene, _, _, _ = small_world
    world = orc.World(G, GH)  # a world of its own: exact mode moves the oracle's LoD distances out of reach
    world.reset_device(True)
    world.set_lod(INT_MAX, INT_MAX)
    rays = special_rays(bm, G, GH)
    assert 300 <= len(rays) <= 1000
    got = scene.cast_rays(rays).packed
    want = oracle_hits(world, rays)
    assert (want["level"] == 2).sum() > len(rays) // 5 and (want["level"] == -1).sum() > 20  # hits and misses are both exercised
    assert_same_hits(got, want, f"special rays {G}x{G}x{GH}")
