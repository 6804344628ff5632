"""The walk fields as one piece on the MI355X (csrc/walk_fields.h, csrc/field_book.h): changes that cross what the cube field, the escape
table, the sun plane with its shadow heights and the view plane each keep -- a carved voxel, a new brick, a residency rebuild, another
volume loaded into the same scene -- each followed by the build counters, the readbacks and a frame, against a scene built from the
changed volume from scratch.

The world is 256 x 256 x 128 voxels (32 x 32 x 16 cells, two supercells along x and y): a floor one cell thick, a block of full bricks
standing on it (one cell along x, three along y, two high) and an overhang.  The block is three bricks wide because no single column can
make a cell dark: the rule of csrc/shadowheight.h takes the least full top of the columns w and w + 1 a ray can reach, so the carved
brick has full neighbours on both sides.  Frames are 64 x 64, 1 spp, 4 segments, under the x-dominant sun of test_gpu_sunfield.py."""
import numpy as np
import pytest

from test_gpu_escape import RGB_TOL
from test_gpu_shadowheights import assert_slice
from test_gpu_sunfield import SUN_X

pytestmark = pytest.mark.gpu

G, GH = 256, 128
W = H = 64
BLOCK = (slice(8, 24), slice(112, 136), slice(128, 136))  # [z, y, x]: cells x 16, y 14 ... 16, z 1 ... 2
CARVED = (131, 123, 11)                                    # (x, y, z): a voxel of the block's middle column, bottom brick
NEW_BRICK = ((200, 200, 64), (208, 208, 72))               # empty space, in another supercell than the block


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def volume():
    vox = np.zeros((GH, G, G), np.uint8)
    vox[:8] = 1
    vox[BLOCK] = 1
    vox[48:56, 150:200, 100:180] = 1  # the overhang: a slab one cell thick, in the air
    return vox  # (shared: the tests copy before they change it)


def cameras(bm):
    """two resting places that see the block and the overhang"""
    return (bm.Camera(position=(G / 2, G / 8, 0.8 * GH), horizontal_angle=0.8, vertical_angle=-0.5).update(),
            bm.Camera(position=(G / 2 + 20, G / 8 + 4, 0.7 * GH), horizontal_angle=0.8, vertical_angle=-0.5).update())


def frame(bm, torch, scene, cam, flags=0):
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    scene.render(cam, bm.FrameParams(W, H, spp=1, max_bounces=3, flags=flags, sun_position=SUN_X), acc)
    torch.cuda.synchronize()
    return acc.cpu().numpy()


def rest(bm, torch, scene, cam):
    """two production launches from `cam`: by the second the camera has rested; returns the second frame"""
    frame(bm, torch, scene, cam)
    return frame(bm, torch, scene, cam)


def counters(scene):
    return scene.sun_plane_stats()[0], scene.view_plane_stats()[0]


def readbacks(scene):
    return dict(field=scene.device_cube_field(), escape=scene.escape_table(), sun=scene.sun_plane()[0], sun_plan=scene.sun_plane()[1],
                shadow=scene.shadow_heights()[0], shadow_plan=scene.shadow_heights()[1], view=scene.view_plane()[0], view_origin=scene.view_plane()[1])


def assert_same_readbacks(got, want, what):
    for name, w in want.items():
        g = got[name]
        assert g is not None and w is not None, f"{what}: no {name}"
        assert g == w if isinstance(w, dict) else np.array_equal(g, w), f"{what}: {name} differs from the fresh scene's"


def assert_same_frame(got, want, what):
    assert np.array_equal(got[..., 3], want[..., 3]), f"{what}: terminated counts differ"
    err, bound = float(np.abs(got[..., :3] - want[..., :3]).max()), RGB_TOL * float(np.abs(want[..., :3]).max())
    print(f"{what}: max |rgb difference| {err:.3e}, bound {bound:.3e}")
    assert float(want[..., :3].max()) > 0 and err <= bound, f"{what}: radiance differs: {err:.3e} > {bound:.3e}"


def test_carved_voxel_rebuilds_the_slice_alone(bm, torch_cuda, volume):
    torch = torch_cuda
    cam, _ = cameras(bm)
    s = bm.Scene.from_voxels(torch.from_numpy(volume).to("cuda:0"))
    rest(bm, torch, s, cam)
    before, builds = assert_slice(s, "as loaded"), counters(s)
    assert builds == (1, 1) and (before > 0).any()
    s.set_voxels([CARVED], 0)
    frame(bm, torch, s, cam)
    got = frame(bm, torch, s, cam)
    assert counters(s) == builds, "no cell's occupancy changed: both planes stand"
    after = assert_slice(s, "carved")
    assert (after <= before).all() and (after < before).any(), "the block's middle column no longer shadows what it did"
    edited = volume.copy()
    edited[CARVED[2], CARVED[1], CARVED[0]] = 0
    assert np.array_equal(s.voxels(), edited.astype(bool))
    fresh = bm.Scene.from_voxels(edited)
    want = rest(bm, torch, fresh, cam)
    assert np.array_equal(fresh.shadow_heights()[0], s.shadow_heights()[0])
    assert_same_frame(got, want, "carved voxel")
    s.close()
    fresh.close()


def test_new_brick_rebuilds_both_planes_once(bm, torch_cuda, volume):
    torch = torch_cuda
    cam, _ = cameras(bm)
    s = bm.Scene.from_voxels(torch.from_numpy(volume).to("cuda:0"))
    rest(bm, torch, s, cam)
    builds = counters(s)
    s.fill_box(*NEW_BRICK)
    assert counters(s) == builds, "an edit alone builds nothing"
    assert s.view_plane()[0] is None and s.sun_plane()[0] is not None, "the stale view plane reads as none, the sun plane as last built"
    got = rest(bm, torch, s, cam)
    assert counters(s) == (builds[0] + 1, builds[1] + 1)
    edited = volume.copy()
    (x0, y0, z0), (x1, y1, z1) = NEW_BRICK
    edited[z0:z1, y0:y1, x0:x1] = 1
    fresh = bm.Scene.from_voxels(edited)
    want = rest(bm, torch, fresh, cam)
    assert_same_readbacks(readbacks(s), readbacks(fresh), "new brick")
    assert_same_frame(got, want, "new brick")
    s.close()
    fresh.close()


def test_residency_rebuild_keeps_the_planes(bm, torch_cuda, volume):
    torch = torch_cuda
    cam, _ = cameras(bm)
    s = bm.Scene.from_voxels(torch.from_numpy(volume).to("cuda:0"))
    frame(bm, torch, s, cam, bm.BM_FLAG_ORDERED)
    want = frame(bm, torch, s, cam, bm.BM_FLAG_ORDERED)
    builds, heights = counters(s), s.shadow_heights()[0]
    assert heights.any()
    s.reset_residency()
    s.preload_all()
    got = frame(bm, torch, s, cam, bm.BM_FLAG_ORDERED)
    assert counters(s) == builds, "residency changes no cell's occupancy: both planes stand"
    assert np.array_equal(s.shadow_heights()[0], heights)
    assert_slice(s, "preloaded again")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the ordered frame differs after reset_residency + preload_all"
    s.close()


def test_another_volume_in_the_same_scene(bm, torch_cuda, volume):
    torch = torch_cuda
    cam, cam2 = cameras(bm)
    s = bm.Scene.from_voxels(torch.from_numpy(volume).to("cuda:0"))
    rest(bm, torch, s, cam)
    other = np.ascontiguousarray(volume[:, ::-1, :])  # the same pieces, mirrored in y: other columns, other shadows
    s.load_voxels(torch.from_numpy(other).to("cuda:0"))
    assert s.view_plane()[0] is None and s.sun_plane()[0] is None and s.shadow_heights()[0] is None, "a new world: nothing is built yet"
    frame(bm, torch, s, cam2)
    assert s.view_plane()[0] is None, "one launch from a new place: the camera has not rested"
    assert s.sun_plane()[0] is not None
    got = frame(bm, torch, s, cam2)
    assert s.view_plane()[0] is not None
    fresh = bm.Scene.from_voxels(other)
    want = rest(bm, torch, fresh, cam2)
    assert_same_readbacks(readbacks(s), readbacks(fresh), "loaded volume")
    assert (assert_slice(fresh, "loaded volume, from scratch") > 0).any()  # (... and those heights are the rule's, for the mirrored block)
    assert_same_frame(got, want, "loaded volume")
    s.close()
    fresh.close()
