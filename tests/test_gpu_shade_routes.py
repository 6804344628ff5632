"""Every way into the ray set-up of the shade pass (csrc/trace.hip, phase C), on frames small enough that they all meet in a few waves.

The shade pass names the next ray's inputs instead of copying them: a block that decides which ray a lane traces next only sets the
lane's path state (P_SETUP_*), and the set-up block at the end of the pass reads origin, direction and normal from their one home each
(`hitp`; `bdir` or `r.d`; `pn` or zero).  The routes that end there:

  connect -> bounce                      a shadow ray came back, the path goes on                       (P_SHD_DONE -> P_SETUP_EXT)
  connect -> next primary ray            a shadow ray came back, the path had reached the bounce limit  (P_SHD_LAST -> P_GEN -> P_SETUP_EXT)
  hit, shadow ray drawn                  kept by the lane or handed to an idle lane (helper-lane frames: given, taken, and the owner
                                         going on with its bounce ray or its next path in the same pass)  (P_SETUP_SHD / _LAST / _HELP)
  hit, no shadow ray, path goes on       the surface faces away from the sun                              (P_SETUP_EXT)
  hit, no shadow ray, path ends          the same at the bounce limit                                     (P_GEN)
  miss, primary-only hit                 the path ends, the next primary ray follows                      (P_GEN -> P_SETUP_EXT)

Which of them a frame takes is read off the ORACLE's hit records, not assumed: per pixel the first-hit record (word 1), the number of
extend rays (word 6, low half) and of shadow rays (high half) of one-sample frames with and without bounces -- the first segment of a
path is the same ray whatever the bounce limit.  Every frame is then compared with the oracle as the parity suite does (tests/
test_gpu_parity.py gpu_render): the ordered instrumented frame bit for bit, the ordered production frame bit for bit with that, the
helper-lane production frame on terminated-path counts exactly and radiance within the bar, and the helper-lane frame's own hits through
the order-independent ray digest, bit for bit.

Shapes: one superchunk (128^3, generated, resident); 16 x 16 pixels -- 256 items for four waves and more, so most of a wave's life is
its tail, with idle lanes next to lanes that draw shadow rays -- and 64 x 48."""
import numpy as np
import pytest

from test_gpu_parity import assert_radiance, assert_ray_digest, gpu_render

pytestmark = pytest.mark.gpu

G = 128
SHAPES = ((16, 16), (64, 48))
SUN_LOW = (0.31, 0.22)  # a sun under which part of what the camera sees faces away from it (asserted below)


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
def cams(bm, orc):
    cam = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
    return cam, orc.make_camera(cam.position, cam.direction)


_routes = {}


def routes(orc, world, ocam, W, H, sun):
    """What the paths of sample 0 do, from the oracle's hit records of two one-sample frames (computed once per shape and sun):
    no bounces -- one extend ray per pixel, so `hit` and `cast` are those of the first segment -- and three bounces."""
    key = (W, H, sun)
    if key not in _routes:
        _, d0, _, _ = world.render(ocam, orc.make_frame(W, H, spp=1, max_bounces=0, sun=sun))
        _, d3, _, _ = world.render(ocam, orc.make_frame(W, H, spp=1, max_bounces=3, sun=sun))
        hit = d0[..., 1] != 0
        cast = (d0[..., 6] >> 16) == 1
        assert np.array_equal(d0[..., 6] & 0xFFFF, np.ones((H, W), np.uint32)) and not np.any(cast & ~hit)
        n_ext, n_shd = d3[..., 6] & 0xFFFF, d3[..., 6] >> 16
        assert np.all(n_ext[hit] >= 2) and np.all(n_ext[~hit] == 1)  # a first hit below the bounce limit is followed by a bounce ray
        _routes[key] = dict(
            miss=int(np.count_nonzero(~hit)),
            cast=int(np.count_nonzero(cast)),              # a shadow ray at the first segment: at the limit with no bounces, bounced on with three
            dark=int(np.count_nonzero(hit & ~cast)),       # a first hit that faces away from the sun: no shadow ray
            cast_at_limit=int(np.count_nonzero((n_ext == 4) & (n_shd == 4))),  # three bounces: the fourth segment hit and drew a shadow ray
            bounced_after_shadow=int(np.count_nonzero((n_shd >= 1) & (n_ext >= 2) & cast)))
    return _routes[key]


def check(bm, orc, torch, scene, world, cams, params, oframe, want_digest=True):
    cam, ocam = cams
    world.reset_device(True)
    acc, dbg = gpu_render(bm, torch, scene, cam, params)
    oacc, odbg, _, _ = world.render(ocam, oframe)
    assert np.array_equal(dbg, odbg), f"{np.count_nonzero((dbg != odbg).any(-1))} pixels with different hit records"
    assert np.array_equal(acc[..., 3], oacc[..., 3]), "terminated-path counts differ from the oracle's"
    assert_radiance(acc, oacc)
    if want_digest:
        assert_ray_digest(world)
    return acc


@pytest.mark.parametrize("mb", (0, 3))
@pytest.mark.parametrize("W,H", SHAPES)
def test_helper_lane_frames_hand_shadow_rays_over(W, H, mb, bm, orc, torch_cuda, scene, world, cams):
    """(a) Production frames with helper lanes, and their instrumented sibling (BM_FLAG_RAY_DIGEST): shadow rays are given and taken; with
    no bounces every owner is at the limit and goes on with its next path (or idles), with three the owner sets its bounce ray up in
    the pass in which it gave the shadow ray away."""
    r = routes(orc, world, cams[1], W, H, (0.05, 0.1))
    assert r["cast"] > 0 and r["miss"] > 0
    if mb == 3:
        assert r["bounced_after_shadow"] > 0 and r["cast_at_limit"] > 0
    p = bm.FrameParams(W, H, spp=1, max_bounces=mb)
    plan = bm.frame_plan(p)
    assert plan["helpers"] and not plan["ordered"]
    check(bm, orc, torch_cuda, scene, world, cams, p, orc.make_frame(W, H, spp=1, max_bounces=mb))


@pytest.mark.parametrize("mb", (0, 3))
@pytest.mark.parametrize("W,H", SHAPES)
def test_ordered_pixel_items_connect_into_bounce_and_next_sample(W, H, mb, bm, orc, torch_cuda, scene, world, cams):
    """(b) BM_FLAG_ORDERED, two samples per pixel traced by one lane one after the other: connect -> bounce (three bounces) and connect
    -> the next sample's primary ray in the same pass (a shadow ray drawn at the bounce limit: every shadow ray with no bounces)."""
    r = routes(orc, world, cams[1], W, H, (0.05, 0.1))
    assert r["cast"] > 0
    if mb == 3:
        assert r["bounced_after_shadow"] > 0 and r["cast_at_limit"] > 0
    p = bm.FrameParams(W, H, spp=2, max_bounces=mb, flags=bm.BM_FLAG_ORDERED)
    plan = bm.frame_plan(p)
    assert plan["ordered"] and not plan["helpers"] and not plan["sample_items"]
    acc = check(bm, orc, torch_cuda, scene, world, cams, p, orc.make_frame(W, H, spp=2, max_bounces=mb), want_digest=False)
    assert np.all(acc[..., 3] == 2)


@pytest.mark.parametrize("mb", (0, 3))
@pytest.mark.parametrize("W,H", SHAPES)
def test_surfaces_that_face_away_draw_no_shadow_ray(W, H, mb, bm, orc, torch_cuda, scene, world, cams):
    """(c) A sun under which some first hits face away: no shadow ray -- the path ends in the shade pass (no bounces) or its bounce ray
    is set up there (three) -- next to hits that do draw one."""
    r = routes(orc, world, cams[1], W, H, SUN_LOW)
    assert r["dark"] > 0 and r["cast"] > 0
    p = bm.FrameParams(W, H, spp=1, max_bounces=mb, sun_position=SUN_LOW)
    check(bm, orc, torch_cuda, scene, world, cams, p, orc.make_frame(W, H, spp=1, max_bounces=mb, sun=SUN_LOW))


@pytest.mark.parametrize("W,H", SHAPES)
def test_primary_only_frames(W, H, bm, orc, torch_cuda, scene, world, cams):
    """(d) BM_FLAG_PRIMARY_ONLY: every path ends at its first ray, hit or miss, and the next primary ray follows in the same pass."""
    r = routes(orc, world, cams[1], W, H, (0.05, 0.1))
    assert r["miss"] > 0 and r["cast"] + r["dark"] > 0
    p = bm.FrameParams(W, H, spp=2, max_bounces=3, flags=bm.BM_FLAG_PRIMARY_ONLY)
    acc = check(bm, orc, torch_cuda, scene, world, cams, p, orc.make_frame(W, H, spp=2, max_bounces=3, primary_only=1), want_digest=False)
    assert np.all(acc[..., 3] == 2)


@pytest.mark.parametrize("W,H", SHAPES)
def test_uniform_ring_of_three_frames_in_one_buffer(W, H, bm, orc, torch_cuda, scene, world, cams):
    """(e) Three frames of the view as one uniform launch with frame groups on, into one buffer: the oracle's three-sample frame --
    terminated-path counts exactly, radiance within the bar, and (instrumented sibling, one shared record buffer) its ray digest."""
    torch = torch_cuda
    cam, ocam = cams
    assert bm.frame_plan(bm.FrameParams(W, H, spp=1, max_bounces=3))["ring_group"] > 1 and not bm.tuning_overrides()
    world.reset_device(True)
    oacc, _, _, _ = world.render(ocam, orc.make_frame(W, H, spp=3, max_bounces=3))
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    scene.render_frames(cam, [bm.FrameParams(W, H, spp=1, sample_base=k, max_bounces=3) for k in range(3)], acc)
    acc_d, dig = torch.zeros_like(acc), torch.zeros((H, W, 8), dtype=torch.int32, device="cuda:0")
    scene.render_frames(cam, [bm.FrameParams(W, H, spp=1, sample_base=k, max_bounces=3, flags=bm.BM_FLAG_RAY_DIGEST) for k in range(3)], acc_d, debugs=[dig] * 3)
    torch.cuda.synchronize()
    assert np.array_equal(dig.cpu().numpy().view(np.uint32), world.last_ray_digest), "frame ring: ray digest differs from the oracle's"
    for got in (acc.cpu().numpy(), acc_d.cpu().numpy()):
        assert np.array_equal(got[..., 3], oacc[..., 3]) and np.all(got[..., 3] == 3)
        assert_radiance(got, oacc)
