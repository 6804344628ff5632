"""Frames whose rays spend their walk where the rule "is a jump worth it here" (csrc/steps.h jump_worth) decides: below
t = 2^BM_JUMP_WORTH_EXP cells a lane with a jump-sized cube ahead is ST_OUTER and takes single moves, or rides in the jump pass of
other lanes; above it it asks for jump passes as before.  Single moves and jumps land on the same tmax bits, so every frame must be
the oracle's: what can go wrong is a lane that never becomes eligible again (the frame would not end, or end with paths missing) or
one that jumps where jump.h is not valid (other hits).

Shapes: one superchunk (128^3, generated, resident); 16 x 16 pixels (a few waves that are mostly tail) and 64 x 48; 1 spp and 4 spp
(the library's (chunk, sample) items in the production plan); no bounces (primary rays only: every lane climbs the low binades at the
same time) and three (bounce and shadow rays start theirs next to lanes far along their walk).  Cameras:
  bench     the benchmark's pose scaled to G = 128
  skim      a quarter of a cell above the terrain looking along it and slightly down: long runs of cells in the low binades with small
            cubes (the surface is right below), then larger cubes while t is still small
  along_x   looking along +x, direction (1, 0, 0): two zero components in the camera's direction

Every frame is compared with the oracle as tests/test_gpu_shade_routes.py does (tests/test_gpu_parity.py gpu_render): the ordered
instrumented frame bit for bit (hit records, index_loads in word 7 included), the ordered production frame bit for bit with that
(inside gpu_render), the helper-lane production frame on terminated-path counts exactly and radiance within the suite's bar, and its
rays through the order-independent ray digest, bit for bit."""
import numpy as np
import pytest

from test_gpu_parity import assert_radiance, assert_ray_digest, cameras, gpu_render

pytestmark = pytest.mark.gpu

G = 128
SHAPES = ((16, 16), (64, 48))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def scene(bm, torch_cuda):
    s = bm.Scene(G, G, device=0).generate()
    s.preload_all()
    yield s
    s.close()


@pytest.fixture(scope="module")
def world(orc):
    w = orc.World(G, G)
    w.reset_device(True)
    return w


@pytest.fixture(scope="module")
def poses(bm, orc, scene):
    vox = scene.voxels()  # [z, y, x]
    x0, y0 = 2, G // 2
    column = np.nonzero(vox[:, y0, x0])[0]
    assert column.size, "the terrain has a column under the skimming camera"
    top = float(column.max() + 1)  # the terrain's upper face in that column
    skim = np.float32([1.0, 0.03, -0.08])
    skim /= np.linalg.norm(skim)
    return {
        "bench": cameras(bm, orc, G),
        "skim": cameras(bm, orc, G, pos=(x0 + 0.5, y0 + 0.5, top + 2.0), direction=skim),  # 2 voxels = a quarter of a cell
        "along_x": cameras(bm, orc, G, pos=(5.5, 50.5, 0.55 * G + 0.5), direction=(1.0, 0.0, 0.0)),
    }


_oracle_frames = {}


def oracle_frame(orc, world, ocam, pose, W, H, spp, mb):
    """The oracle's frame and ray digest, rendered once per case."""
    key = (pose, W, H, spp, mb)
    if key not in _oracle_frames:
        world.reset_device(True)
        oacc, odbg, _, _ = world.render(ocam, orc.make_frame(W, H, spp=spp, max_bounces=mb))
        _oracle_frames[key] = (oacc, odbg, world.last_ray_digest.copy())
    return _oracle_frames[key]


@pytest.mark.parametrize("mb", (0, 3))
@pytest.mark.parametrize("spp", (1, 4))
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("pose", ("bench", "skim", "along_x"))
def test_frames_match_the_oracle(pose, W, H, spp, mb, bm, orc, torch_cuda, scene, world, poses):
    cam, ocam = poses[pose]
    p = bm.FrameParams(W, H, spp=spp, max_bounces=mb)
    plan = bm.frame_plan(p)
    assert plan["helpers"] and not plan["ordered"] and bool(plan["sample_items"]) == (spp > 1)
    oacc, odbg, odigest = oracle_frame(orc, world, ocam, pose, W, H, spp, mb)
    acc, dbg = gpu_render(bm, torch_cuda, scene, cam, p)
    if pose != "along_x":
        assert np.count_nonzero(odbg[..., 1]) > 0, "the terrain is in view"
    assert np.array_equal(dbg, odbg), f"{np.count_nonzero((dbg != odbg).any(-1))} pixels with different hit records"
    assert np.array_equal(acc[..., 3], oacc[..., 3]) and np.all(acc[..., 3] == spp), "terminated-path counts differ from the oracle's"
    assert_radiance(acc, oacc)
    world.last_ray_digest = odigest
    assert_ray_digest(world)
