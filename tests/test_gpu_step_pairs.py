"""Frames whose rays run into the borders of the cube field's planes, where the pair move of the single-move passes (csrc/steps.h
step_pair_ahead, csrc/trace.hip BM_STEP_AHEAD) looks one cell further than it commits: the byte beyond a border cell lies in the row padding,
in the neighbouring plane or in the guard bytes round the planes (csrc/field_layout.h), and is dropped -- so every frame must be the oracle's,
and nothing a reader of the fields sees may change.

Shapes: 128^3 worlds (16 cells per side, generated, resident), a flat one (256 x 256 x 128) and a tall one (128 x 128 x 256); 16 x 16 pixels
(a few waves that are mostly tail) and 64 x 48; no bounces and three.  Cameras:
  inside        the benchmark's pose scaled to the world
  in_*          outside the world, looking in through each of its six faces
  out_*         inside and above the terrain, looking out through each face; the terrain closes the bottom, so out_bottom looks down a
                shaft cut through the world (both the product's and the oracle's) -- its rays are of octant 7 and leave through the bottom
                of that plane, and up_shaft looks up the same shaft from below the world: rays of octant 0 that enter at the bottom slice of
                plane 0, the lowest offsets there are, and leave through the top
  top_*         out through the top under the default sun and under one that has no sun plane: with the camera at rest the production
                frames of a case walk the view plane, the last plane of the allocation, and the first of them, before the camera has
                rested, the octant planes

Every frame is compared with the oracle as tests/test_gpu_jump_room.py does (tests/test_gpu_parity.py gpu_render): the ordered instrumented
frame bit for bit (hit records, index_loads in word 7 included), the ordered production frame bit for bit with that, the helper-lane
production frame on terminated-path counts exactly and radiance within the suite's bar, and its rays through the order-independent ray
digest, bit for bit; the traversal counters of a counted frame equal the oracle's."""
import numpy as np
import pytest

from test_gpu_edit import oracle_clear
from test_gpu_parity import assert_radiance, assert_ray_digest, cameras, gpu_render
from test_gpu_sunfield import SUN_ACROSS, SUN_X

pytestmark = pytest.mark.gpu

G = 128
SHAPES = ((16, 16), (64, 48))
WORLDS = {"cube": (G, G), "shaft": (G, G), "flat": (256, 128), "tall": (128, 256)}
SHAFT = ((56, 56, 0), (72, 72, G))  # two cells by two, from the bottom to the top


def _unit(*d):
    v = np.float32(d)
    return tuple(float(x) for x in v / np.linalg.norm(v))


# name: (world, position, direction or None for the benchmark's angles, sun)
POSES = {
    "inside": ("cube", None, None, SUN_X),
    "in_x0": ("cube", (-40.0, 60.0, 90.0), _unit(1, 0.1, -0.3), SUN_X),
    "in_x1": ("cube", (170.0, 60.0, 90.0), _unit(-1, 0.1, -0.3), SUN_X),
    "in_y0": ("cube", (60.0, -40.0, 90.0), _unit(0.1, 1, -0.3), SUN_X),
    "in_y1": ("cube", (60.0, 170.0, 90.0), _unit(0.1, -1, -0.3), SUN_X),
    "in_top": ("cube", (60.0, 70.0, 200.0), _unit(0.1, -0.2, -1), SUN_X),
    "in_bottom": ("cube", (60.0, 70.0, -40.0), _unit(0.1, 0.2, 1), SUN_X),
    "out_x0": ("cube", (64.0, 64.0, 120.0), _unit(-1, 0.05, 0.1), SUN_X),
    "out_x1": ("cube", (64.0, 64.0, 120.0), _unit(1, -0.05, 0.1), SUN_X),
    "out_y0": ("cube", (64.0, 64.0, 120.0), _unit(0.05, -1, 0.1), SUN_X),
    "out_y1": ("cube", (64.0, 64.0, 120.0), _unit(-0.05, 1, 0.1), SUN_X),
    "top_sun": ("cube", (64.0, 64.0, 100.0), _unit(0.1, 0.15, 1), SUN_X),
    "top_no_sun_plane": ("cube", (64.0, 64.0, 100.0), _unit(-0.1, 0.15, 1), SUN_ACROSS),
    "out_bottom": ("shaft", (64.5, 64.5, 120.0), _unit(-0.02, -0.03, -1), SUN_X),
    "up_shaft": ("shaft", (63.5, 63.5, -30.0), _unit(0.02, 0.03, 1), SUN_X),
    "flat": ("flat", None, None, SUN_X),
    "flat_out_top": ("flat", (200.0, 60.0, 120.0), _unit(0.3, 0.2, 1), SUN_X),
    "tall": ("tall", None, None, SUN_X),
    "tall_out_x1": ("tall", (64.0, 64.0, 250.0), _unit(1, 0.05, 0.02), SUN_X),
}
LEAVES = [p for p in POSES if p.startswith(("out_", "top_", "up_", "flat_out", "tall_out"))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def worlds(bm, orc, torch_cuda):
    """name -> (scene, oracle world), made on first use; the shaft is cut into both"""
    made = {}

    def get(name):
        if name not in made:
            g, gh = WORLDS[name]
            s = bm.Scene(g, gh, device=0).generate().preload_all()
            w = orc.World(g, gh)
            if name == "shaft":
                (x0, y0, z0), (x1, y1, z1) = SHAFT
                removed = np.zeros((gh, g, g), bool)
                removed[z0:z1, y0:y1, x0:x1] = s.voxels()[z0:z1, y0:y1, x0:x1] != 0
                assert removed[:8].any(), "the shaft opens the bottom"
                s.clear_box(*SHAFT)
                oracle_clear(w, removed)
                assert not s.voxels()[z0:z1, y0:y1, x0:x1].any()
            w.reset_device(True)
            made[name] = (s, w)
        return made[name]

    yield get
    for s, _ in made.values():
        s.close()


def pose_cameras(bm, orc, pose):
    world, pos, direction, sun = POSES[pose]
    g, gh = WORLDS[world]
    if pos is None:
        pos = (g / 2, g / 8, 0.8 * gh)
    return cameras(bm, orc, g, pos=pos, direction=direction), sun


_oracle_frames = {}


def oracle_frame(orc, world, ocam, pose, W, H, mb, sun):
    """The oracle's frame, counters and ray digest, rendered once per case."""
    key = (pose, W, H, mb)
    if key not in _oracle_frames:
        world.reset_device(True)
        oacc, odbg, ocnt, _ = world.render(ocam, orc.make_frame(W, H, spp=1, max_bounces=mb, sun=sun))
        _oracle_frames[key] = (oacc, odbg, ocnt, world.last_ray_digest.copy())
    return _oracle_frames[key]


@pytest.mark.parametrize("mb", (0, 3))
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("pose", list(POSES))
def test_frames_match_the_oracle(pose, W, H, mb, bm, orc, torch_cuda, worlds):
    scene, world = worlds(POSES[pose][0])
    (cam, ocam), sun = pose_cameras(bm, orc, pose)
    p = bm.FrameParams(W, H, spp=1, max_bounces=mb, sun_position=sun)
    plan = bm.frame_plan(p)
    assert plan["helpers"] and not plan["ordered"]
    oacc, odbg, _, odigest = oracle_frame(orc, world, ocam, pose, W, H, mb, sun)
    acc, dbg = gpu_render(bm, torch_cuda, scene, cam, p)
    if pose in LEAVES:
        assert np.count_nonzero(odbg[..., 1] == 0) > 0, "some primary ray leaves the world"
    else:
        assert np.count_nonzero(odbg[..., 1]) > 0, "the world is in view"
    assert np.array_equal(dbg, odbg), f"{np.count_nonzero((dbg != odbg).any(-1))} pixels with different hit records"
    assert np.array_equal(acc[..., 3], oacc[..., 3]) and np.all(acc[..., 3] == 1), "terminated-path counts differ from the oracle's"
    assert_radiance(acc, oacc)
    world.last_ray_digest = odigest
    assert_ray_digest(world)


@pytest.mark.parametrize("pose", list(POSES))
def test_counters_match_the_oracle(pose, bm, orc, torch_cuda, worlds):
    """index_loads counts committed cells only: a counted frame's traversal counters are the oracle's, with helper lanes as well (gpu_render (c))"""
    W, H, mb = 64, 48, 3
    scene, world = worlds(POSES[pose][0])
    (cam, ocam), sun = pose_cameras(bm, orc, pose)
    _, odbg, ocnt, _ = oracle_frame(orc, world, ocam, pose, W, H, mb, sun)
    scene.counters_reset()
    _, dbg = gpu_render(bm, torch_cuda, scene, cam, bm.FrameParams(W, H, spp=1, max_bounces=mb, flags=bm.BM_FLAG_COUNTERS, sun_position=sun))
    assert np.array_equal(dbg, odbg)
    assert scene.counters() == ocnt and ocnt["index_loads"] > 0
    scene.counters_reset()


def test_the_fields_read_back_unchanged(bm, orc, torch_cuda, worlds):
    """The guard bytes change nothing a reader sees: the cube field is the host's before and after frames, the sun plane and the view plane read
    back after further frames as they did once built."""
    torch = torch_cuda
    scene, _ = worlds("cube")
    (cam, _), sun = pose_cameras(bm, orc, "top_sun")
    field = scene.device_cube_field()
    assert np.array_equal(field, scene.host_cube_field()) and field.shape == (8, G // 8 + 2, G // 8 + 2, G // 8 + 2)

    def frames(n):
        for k in range(n):
            acc = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
            scene.render(cam, bm.FrameParams(64, 48, spp=1, sample_base=k, max_bounces=3, sun_position=sun), acc)
        torch.cuda.synchronize()

    frames(2)  # by the second launch the camera has rested: both planes stand
    sun_plane, view_plane = scene.sun_plane()[0], scene.view_plane()[0]
    assert sun_plane is not None and view_plane is not None
    frames(3)
    assert np.array_equal(scene.device_cube_field(), field)
    assert np.array_equal(scene.sun_plane()[0], sun_plane) and np.array_equal(scene.view_plane()[0], view_plane)
