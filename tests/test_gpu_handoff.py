"""The stream hand-off (brickmap_amd/_handoff.py) in the calls that had no side-stream case of their own: Quads.triangles,
DistanceField.mask, TravelField.paths and Scene.pixel_rays.  The producing call is queued on the current stream, the call under test runs
on a side stream from probe_streams with no host synchronisation in between, and its result must equal, bit for bit, that of the same call
on the current stream.  The volume is 9 x 10 x 17 [z, y, x] -- it crosses an 8^3 cell along every axis --, the frame 5 x 3: milliseconds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def scene(bm, torch_cuda):
    s = bm.Scene(128, 128, device=0).generate().preload_all()
    yield s
    s.close()


@pytest.fixture(scope="module")
def side(bm, torch_cuda):
    """the raw handle of one stream that is not torch's current one"""
    handles = bm.probe_streams(1, device=0)
    assert handles[0] != torch_cuda.cuda.current_stream().cuda_stream
    yield handles[0]
    torch_cuda.cuda.synchronize()
    bm.release_streams(handles)


@pytest.fixture()
def volume(torch_cuda):
    """a few solid voxels on both sides of the cell borders at 8 (z, y, x) and 16 (x), made on the current stream just before the call"""
    vol = np.zeros((9, 10, 17), np.uint8)
    for z, y, x in ((0, 0, 0), (7, 7, 7), (8, 8, 8), (8, 9, 16), (3, 8, 15), (4, 4, 16), (7, 2, 8)):
        vol[z, y, x] = 1
    return torch_cuda.from_numpy(vol).cuda()


def same_bytes(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_triangles_on_a_side_stream(torch_cuda, scene, side, volume):
    quads = scene.mesh_quads(volume, capacity=64)       # with a capacity the host does not wait for the quads
    got = quads.triangles(stream=side)                  # (reads the count first, which does)
    want = quads.triangles()
    torch_cuda.cuda.synchronize()
    assert quads.count == 7 * 6 and tuple(got.shape) == (2 * quads.count, 3, 3) and same_bytes(got, want)


def test_distance_mask_on_a_side_stream(torch_cuda, scene, side, volume):
    field = scene.distance_field(volume)                 # queued on the current stream; nobody waits for it
    got = field.mask(5, stream=side)
    out = torch_cuda.full((9, 10, 17), 77, dtype=torch_cuda.uint8, device="cuda")
    assert field.mask(5, above=True, out=out, stream=side) is out
    want, want_above = field.mask(5), field.mask(5, above=True)
    torch_cuda.cuda.synchronize()
    assert same_bytes(got, want) and same_bytes(out, want_above)
    assert 0 < int(want.sum()) < want.numel() and int(want.sum()) + int(want_above.sum()) == want.numel()


def test_travel_paths_on_a_side_stream(torch_cuda, scene, side, volume):
    field = scene.travel_field(volume, [(1, 1, 1)])
    starts = [(16, 9, 7), (0, 9, 8), (8, 8, 8), (15, 0, 0), (40, 0, 0)]      # far corners, a blocked voxel, one outside
    d_starts = torch_cuda.tensor(starts, dtype=torch_cuda.int32, device="cuda")   # made on the current stream, read on the side stream
    got = field.paths(d_starts, 40, stream=side)
    got_list = field.paths(starts, 40, stream=side)
    want = field.paths(starts, 40)
    torch_cuda.cuda.synchronize()
    for g in (got, got_list):
        assert same_bytes(g[0], want[0]) and same_bytes(g[1], want[1])
    lengths = want[1].cpu().numpy()
    assert lengths[0] == 15 + 8 + 6 + 1 and lengths[2] == 0 and lengths[4] == 0 and (lengths[[0, 1, 3]] > 8).all()


def test_pixel_rays_on_a_side_stream(bm, torch_cuda, scene, side):
    cam = bm.Camera(position=(64.0, 16.0, 100.0), horizontal_angle=0.8, vertical_angle=-0.5).update()
    got = scene.pixel_rays(cam, 5, 3, stream=side)
    want = scene.pixel_rays(cam, 5, 3)
    torch_cuda.cuda.synchronize()
    assert tuple(got.shape) == (15, 8) and same_bytes(got, want)
    ys, xs = np.divmod(np.arange(15), 5)
    host = bm.camera_pixel_rays(cam, 5, 3, xs + 0.5, ys + 0.5)
    assert got.cpu().numpy().tobytes() == host.tobytes()
    hits = scene.cast_rays(got, stream=side)             # and the rays feed a query on the same stream, as pixel_hits does
    torch_cuda.cuda.synchronize()
    assert same_bytes(hits.packed, scene.cast_rays(want).packed)
