"""Shadow rays that the shadow heights decide are never drawn (csrc/trace.hip shade block, csrc/shadowheight.h shadow_origin), on the MI355X.

The production instantiations test the shadow ray's origin in the shade pass and let a dark lane take the transition of a surface that
faces away from the sun; the instrumented kernel never reads the table.  So every case compares production frames with instrumented ones
the way tests/test_gpu_shadowheights.py does (check_frames: ordered production bit for bit, helper-lane alpha exact and radiance within
RGB_TOL x max), in that file's scenes, and asserts from its numpy model that shadow rays of cells the camera sees start in dark cells --
no case passes without the rule firing.  The cases are the places where the new transition can go wrong: paths that end in the shade pass
itself (max_bounces 0), sample items with helper lanes and atomic sums, a uniform launch of three frames, a ring whose second frame has
no plane, suns without a plan, origins outside the box (top faces of a world that reaches its top layer, seen from outside), a streaming
scene (zero slice, the same brick requests), and an edit that opens dark cells to the sun.  Frames are 64 x 48; the world is 128^3 voxels.
The rule's CPU test is tests/test_shadow_origin_rule.py."""
import numpy as np
import pytest

import test_gpu_shadowheights as sh
from test_gpu_escape import camera
from test_gpu_shadowheights import H, RGB_TOL, SCENES, W, assert_slice, check_frames, render_once, scene_voxels, scenes, seen_dark_cells, terrain, torch_cuda  # noqa: F401 (fixtures)
from test_gpu_sunfield import SUN_ACROSS, SUN_X, SUN_Y, SUN_Z, WORLDS, camera_over

pytestmark = pytest.mark.gpu

G, GH = WORLDS["cube"]


def assert_rule_fires(scene, cam, what):
    """the condition of test_gpu_shadowheights: shadow rays of surface cells the camera sees start in dark cells; returns Zd"""
    zd = assert_slice(scene, what)
    dark, seen = seen_dark_cells(scene, cam, zd)
    print(f"{what}: {dark} of {seen} primary hits start their shadow ray in a dark cell")
    assert dark > seen // 50 and dark > 10, f"{what}: the rule ends too few of the view's shadow rays to be tested ({dark} of {seen})"
    return zd


def with_params(monkeypatch, bm, **kw):
    """check_frames and render_once of test_gpu_shadowheights with other frame parameters (its own: 1 spp, 3 bounces)"""
    def params(bm_, sun, flags=0, sample_base=0):
        return bm.FrameParams(W, H, sample_base=sample_base, flags=flags, sun_position=sun, **kw)
    monkeypatch.setattr(sh, "params", params)


def fresh_scene(bm, torch, terrain, kind, change=None):
    vox = scene_voxels(kind, terrain["cube"])
    if change is not None:
        change(vox)
    return bm.Scene.from_voxels(torch.from_numpy(vox.astype(np.uint8)).to("cuda:0"))


def zeros(torch, *shape, dtype=None):
    return torch.zeros(shape, dtype=dtype or torch.float32, device="cuda:0")


# ---------------------------------------------------------------- paths that end, or go on, inside the shade pass
@pytest.mark.parametrize("max_bounces", [0, 3])
@pytest.mark.parametrize("kind", SCENES)
def test_dark_lanes_end_or_bounce_in_the_shade_pass(kind, max_bounces, bm, torch_cuda, scenes, monkeypatch):
    """max_bounces 0: every dark ray's path is `terminated` -- the lane goes to the generate block of the same pass; 3: it sets its bounce ray up"""
    with_params(monkeypatch, bm, spp=1, max_bounces=max_bounces)
    scene, cam = scenes(kind), camera_over(bm, G, GH)
    inst = check_frames(bm, torch_cuda, scene, cam, SUN_X, f"{kind}, {max_bounces} bounces")
    assert np.array_equal(inst[..., 3], np.ones((H, W), np.float32)), "one path per pixel"
    assert_rule_fires(scene, cam, f"{kind}, {max_bounces} bounces")


@pytest.mark.parametrize("max_bounces", [0, 3])
def test_sample_items_with_helper_lanes(max_bounces, bm, torch_cuda, scenes):
    """4 spp dealt as (chunk, sample) items: helper lanes and atomic sums; alpha is 4 in every pixel exactly"""
    torch = torch_cuda
    scene, cam = scenes("notch"), camera_over(bm, G, GH)
    inst, dbg, got = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32), zeros(torch, H, W, 4)
    scene.render(cam, bm.FrameParams(W, H, spp=4, max_bounces=max_bounces, flags=bm.BM_FLAG_ORDERED, sun_position=SUN_X), inst, debug=dbg)
    scene.render(cam, bm.FrameParams(W, H, spp=4, max_bounces=max_bounces, flags=bm.BM_FLAG_SAMPLE_ITEMS, sun_position=SUN_X), got)
    torch.cuda.synchronize()
    a, b = got.cpu().numpy(), inst.cpu().numpy()
    assert np.array_equal(a[..., 3], np.full((H, W), 4.0, np.float32)) and np.array_equal(b[..., 3], a[..., 3])
    err, bound = float(np.abs(a[..., :3] - b[..., :3]).max()), RGB_TOL * float(np.abs(b[..., :3]).max())
    print(f"sample items, {max_bounces} bounces: max |rgb difference| {err:.3e}, bound {bound:.3e}")
    assert err <= bound and bound > 0
    assert_rule_fires(scene, cam, "sample items")


def test_uniform_launch_of_three_frames(bm, torch_cuda, scenes):
    """three frames of one view as one uniform launch into one buffer (what the benchmark issues) = the sum of three instrumented launches"""
    torch = torch_cuda
    scene, cam = scenes("hollow"), camera_over(bm, G, GH)
    inst, dbg, got = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32), zeros(torch, H, W, 4)
    for k in range(3):
        scene.render(cam, bm.FrameParams(W, H, spp=1, sample_base=k, max_bounces=3, flags=bm.BM_FLAG_ORDERED, sun_position=SUN_X), inst, debug=dbg)
    scene.render_frames(cam, [bm.FrameParams(W, H, spp=1, sample_base=k, max_bounces=3, sun_position=SUN_X) for k in range(3)], got)
    torch.cuda.synchronize()
    a, b = got.cpu().numpy(), inst.cpu().numpy()
    assert np.array_equal(a[..., 3], b[..., 3]) and np.array_equal(b[..., 3], np.full((H, W), 3.0, np.float32))
    err, bound = float(np.abs(a[..., :3] - b[..., :3]).max()), RGB_TOL * float(np.abs(b[..., :3]).max())
    print(f"uniform launch of three: max |rgb difference| {err:.3e}, bound {bound:.3e}")
    assert err <= bound and bound > 0
    assert_rule_fires(scene, cam, "uniform launch of three")


@pytest.mark.parametrize("max_bounces", [0, 3])
def test_ring_of_two_suns(max_bounces, bm, torch_cuda, scenes):
    """two frames with different suns as one launch: the plane and the table are the first frame's; the second has no plane and must not test"""
    torch = torch_cuda
    scene, cam = scenes("notch"), camera_over(bm, G, GH)

    def params(sun, flags, k):
        return bm.FrameParams(W, H, spp=1, sample_base=k, max_bounces=max_bounces, flags=flags, sun_position=sun)
    for flags in (bm.BM_FLAG_ORDERED, 0):
        want = []
        for k, sun in enumerate((SUN_X, SUN_Y)):
            inst, dbg = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32)
            scene.render(cam, params(sun, bm.BM_FLAG_ORDERED, k), inst, debug=dbg)
            want.append(inst)
        got = [zeros(torch, H, W, 4) for _ in range(2)]
        scene.render_frames(cam, [params(sun, flags, k) for k, sun in enumerate((SUN_X, SUN_Y))], got)
        torch.cuda.synchronize()
        assert scene.sun_plane()[1]["dom"] == 0, "the plane is the first frame's"
        for k in range(2):
            a, b = got[k].cpu().numpy(), want[k].cpu().numpy()
            assert np.array_equal(a[..., 3], b[..., 3])
            if flags:
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"ordered ring, frame {k}"
            else:
                assert float(np.abs(a[..., :3] - b[..., :3]).max()) <= RGB_TOL * float(np.abs(b[..., :3]).max()), f"helper-lane ring, frame {k}"
    assert_rule_fires(scene, cam, "ring of two suns")


def test_suns_without_a_plan(bm, torch_cuda, scenes):
    """a cone across an octant boundary has no plane (nothing is built, the table of the sun before stays and is not read); a z-dominant sun has a
    plane and no shadow heights (the slice is zero)"""
    scene, cam = scenes("overhang"), camera_over(bm, G, GH)
    render_once(bm, torch_cuda, scene, cam, SUN_X)
    assert_rule_fires(scene, cam, "the sun before")
    builds = scene.sun_plane_stats()[0]
    check_frames(bm, torch_cuda, scene, cam, SUN_ACROSS, "cone across an octant boundary")
    assert scene.sun_plane_stats()[0] == builds, "nothing is built for a sun without a plan"
    check_frames(bm, torch_cuda, scene, cam, SUN_Z, "z dominant")
    entries, splan, _ = scene.shadow_heights()
    assert splan["valid"] == 0 and not entries.any()


# ---------------------------------------------------------------- origins the rule leaves undecided
def test_origins_outside_the_box_are_traced(bm, torch_cuda, terrain):
    """a tower that reaches the world's topmost voxel layer, seen from outside and above: hit points on its top face lie outside the box
    (z = height + 2 epsilon), the rule is undecided and the ray is traced as it always was"""
    def tower(vox):
        vox[:, 56:72, 80:96] = True
    scene = fresh_scene(bm, torch_cuda, terrain, "notch", tower)
    cam = camera(bm, (G / 2, 40.0, GH + 32.0), (0.5, 0.5, -0.7))  # above the world's top; the middle of the view meets the tower's top face
    assert cam.position[2] > GH
    hits = scene.pixel_hits(cam, W, H)
    voxel, normal, level = hits.voxel.cpu().numpy(), hits.normal.cpu().numpy(), hits.level.cpu().numpy()
    on_top = int(np.count_nonzero((level >= 0) & (voxel[:, 2] == GH - 1) & (np.rint(normal[:, 2]) == 1)))
    print(f"origins outside the box: {on_top} primary hits on the tower's top face")
    assert on_top > 10, "the view does not see the top face"
    check_frames(bm, torch_cuda, scene, cam, SUN_X, "origins outside the box")
    assert_rule_fires(scene, cam, "origins outside the box")
    scene.close()


# ---------------------------------------------------------------- a streaming scene
def test_streaming_scene_requests_what_it_did(bm, torch_cuda, terrain):
    """after reset_residency the slice is zero: the ordered production frame is the instrumented one and both request the same bricks"""
    torch = torch_cuda
    scene, cam = fresh_scene(bm, torch, terrain, "notch"), camera_over(bm, G, GH)
    render_once(bm, torch, scene, cam, SUN_X)
    assert_rule_fires(scene, cam, "preloaded")
    p = bm.FrameParams(W, H, spp=1, max_bounces=3, flags=bm.BM_FLAG_ORDERED, sun_position=SUN_X)
    scene.reset_residency()
    inst, dbg = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32)
    scene.render(cam, p, inst, debug=dbg)
    torch.cuda.synchronize()
    requested_inst = scene.process_load_queue()
    scene.reset_residency()
    prod = zeros(torch, H, W, 4)
    scene.render(cam, p, prod)
    torch.cuda.synchronize()
    entries, splan, _ = scene.shadow_heights()  # (rebuilt, as zeros, by the production frame: the instrumented one never reads it)
    assert splan["valid"] == 0 and not entries.any(), "no shadow heights while bricks are streamed in"
    requested_prod = scene.process_load_queue()
    assert requested_inst == requested_prod > 0, f"bricks requested: instrumented {requested_inst}, production {requested_prod}"
    assert np.array_equal(prod.cpu().numpy().view(np.uint32), inst.cpu().numpy().view(np.uint32))
    scene.close()


# ---------------------------------------------------------------- an edit that lets the sun in
def test_edit_opens_dark_cells_to_the_sun(bm, torch_cuda, terrain):
    """part of the wall that shadows the view is removed: cells behind it are dark no longer, and the next frame is the instrumented frame of the edited scene"""
    torch = torch_cuda
    scene, cam = fresh_scene(bm, torch, terrain, "partial top"), camera_over(bm, G, GH)
    render_once(bm, torch, scene, cam, SUN_X)
    before = assert_rule_fires(scene, cam, "before the edit")
    scene.clear_box((24, 56, 8), (32, 104, 104))  # the wall along y, between the view and the sun
    check_frames(bm, torch, scene, cam, SUN_X, "after the edit")
    after = assert_rule_fires(scene, cam, "after the edit")
    assert (after <= before).all() and (after < before).any(), "the wall no longer shadows what it did"
    scene.close()
