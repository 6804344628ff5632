"""The sun plane on the MI355X (csrc/sunfield.h, sunfield.hip; the rules' CPU replay is tests/test_sunfield_rule.py).

5.1  The plane the device holds (bm_scene_sun_plane) equals the rules written in numpy (numpy_sun_plane below, on the device's own index
     words and the plan the device reports): after generate, after load_voxels, after an edit that puts a brick where the plane said
     "nothing can be hit from here on", after a region write, and after the sun has changed -- in a cube, a flat and a tall world.
5.2  Frames of the production instantiations -- whose shadow rays walk the plane -- against the instrumented one's, which never reads
     it: ordered frames bit for bit, helper-lane frames (what bench.py times) with alpha exact and radiance within the parity tolerance
     of test_gpu_escape -- under an overhang between the surface and the sun, with a very low sun, a sun with z dominant, a sun whose
     cone lies across an octant boundary (no plane: the octant planes as before) and a ring of two frames with different suns.
5.3  The build counter stands still across renders with the same sun and world and moves once after one edit batch.
Frames are 64 x 64, 1 spp, 4 segments; worlds of 128^3 to 256 x 256 x 128 voxels."""
import math

import numpy as np
import pytest

from test_gpu_escape import RGB_TOL, device_occupancy, numpy_table

pytestmark = pytest.mark.gpu

WORLDS = {"cube": (128, 128), "tall": (128, 256), "flat": (256, 128)}
W = H = 64
MB = 3
SUN_X = (0.05, 0.1)    # the default: (-0.904, -0.294, 0.309), x dominant
SUN_Y = (0.2, 0.1)     # (-0.294, -0.904, 0.309), y dominant
SUN_Z = (0.3, 0.4)     # (0.095, -0.294, 0.951), z dominant
SUN_LOW = (0.05, 0.02)  # 3.6 degrees above the horizon
SUN_ACROSS = (0.0, 0.1)  # y = 0: the cone lies across an octant boundary


def sun_direction(sun):
    px, py = sun[0] * 6.28, (sun[1] - 0.5) * 3.14
    return np.array([math.cos(px) * math.sin(py), math.sin(px) * math.sin(py), math.cos(py)])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def terrain(bm, torch_cuda):
    """per world: the generated terrain's voxels [z, y, x] (bool), computed once"""
    out = {}
    for name, (g, h) in WORLDS.items():
        s = bm.Scene(g, h, device=0).generate()
        out[name] = s.voxels().astype(bool)
        s.close()
    return out


# ---------------------------------------------------------------- the rules in numpy
def numpy_sun_plane(occ, plan):
    """uint8 [z, y, x] over brick cells: the bytes of include/brickmap.h bm_scene_sun_plane for the occupancy `occ` and the plan `plan`"""
    B, dom, m1, m2, octant = plan["bins"], plan["dom"], plan["m1"], plan["m2"], plan["octant"]
    lo, hi = (plan["lo1"], plan["lo2"]), (plan["hi1"], plan["hi2"])
    nz = occ.shape[0]
    zs = np.arange(nz).reshape(-1, 1, 1)
    top = np.where(occ, zs, -1).max(axis=0)   # [y, x]
    quad = numpy_table(occ)[octant]           # [y, x]: the quadrant rule's threshold of the cone's octant

    def directed3(a):  # [z, y, x] -> [ud, u2, u1]
        for axis in range(3):
            if octant >> axis & 1:
                a = np.flip(a, 2 - axis)
        return np.transpose(a, (2 - dom, 2 - m2, 2 - m1))

    def directed2(a):  # [y, x] -> [ud, u1] (D and m1 horizontal)
        for axis in range(2):
            if octant >> axis & 1:
                a = np.flip(a, 1 - axis)
        return np.transpose(a, (1 - dom, 1 - m1))

    A = directed3(occ)
    nd, n2, n1 = A.shape
    # ---- the first stamped z of every column, in directed coordinates
    if plan["clear"]:
        top_d, quad_d = directed2(top), directed2(quad)
        stamped = np.zeros((nd, n1), np.int64)
        cn = np.zeros((n1 + 2, B), np.int64)
        for ud in range(nd - 1, -1, -1):
            height = np.zeros(n1 + 1, np.int64)
            height[:n1] = (top_d[ud] + 1) * 256
            w = np.arange(n1)
            c = np.maximum(height[:n1], height[1:])  # hi1 >= 1: a ray anywhere in the cell can reach the next column
            for g in range(0, B + hi[0]):
                c = np.maximum(c, cn[w + g // B, g % B])
            stamped[ud] = np.minimum(np.where(c > 0, (c + 4 + 255) // 256, 0), quad_d[ud] + 1)
            cc = np.zeros_like(cn)
            for b in range(B):
                f = height[:n1].copy()
                if (b + hi[0]) // B:
                    f = np.maximum(f, height[1:])
                for g in range(b + lo[0], b + hi[0] + 1):
                    f = np.maximum(f, cn[w + g // B, g % B] - plan["rise"])
                cc[:n1, b] = f
            cn = cc
        z_of = np.arange(n2).reshape(1, -1, 1)            # m2 = z, never flipped
        is_stamped = z_of >= stamped[:, None, :]          # [ud, u2, u1]
    else:
        first = quad + 1  # D = z: (u2, u1) are (y, x), flipped where the cone's direction is negative
        for axis in range(2):
            if octant >> axis & 1:
                first = np.flip(first, 1 - axis)
        is_stamped = np.arange(nd).reshape(-1, 1, 1) >= first[None, :, :]
    # ---- face values slab by slab, and the bytes
    out = np.zeros(A.shape, np.uint8)
    fn = np.zeros((n2 + 2, n1 + 2, B, B), np.int64)
    i2, i1 = np.meshgrid(np.arange(n2), np.arange(n1), indexing="ij")

    def least(g1s, g2s):
        m = np.full((n2, n1), 253, np.int64)
        for g2 in g2s:
            for g1 in g1s:
                m = np.minimum(m, fn[i2 + g2 // B, i1 + g1 // B, g2 % B, g1 % B])
        return m

    for ud in range(nd - 1, -1, -1):
        blocked = np.ones((n2 + 1, n1 + 1), bool)
        blocked[:n2, :n1] = A[ud]

        def rect(o1, o2):
            r = np.zeros((n2, n1), bool)
            for j in range(o2 + 1):
                for i in range(o1 + 1):
                    r |= blocked[j:j + n2, i:i + n1]
            return r

        byte = np.where(rect((B - 1 + hi[0]) // B, (B - 1 + hi[1]) // B), 0, 1 + least(range(0, B + hi[0]), range(0, B + hi[1])))
        byte = np.maximum(byte, 1)
        byte = np.where(is_stamped[ud], 255, byte)
        out[ud] = np.where(A[ud], 0, byte)
        fc = np.zeros_like(fn)
        for b2 in range(B):
            for b1 in range(B):
                f = 1 + least(range(b1 + lo[0], b1 + hi[0] + 1), range(b2 + lo[1], b2 + hi[1] + 1))
                fc[:n2, :n1, b2, b1] = np.where(rect((b1 + hi[0]) // B, (b2 + hi[1]) // B), 0, f)
        fn = fc
    # ---- back to [z, y, x]
    inv = np.argsort((2 - dom, 2 - m2, 2 - m1))
    out = np.transpose(out, inv)
    for axis in range(3):
        if octant >> axis & 1:
            out = np.flip(out, 2 - axis)
    return np.ascontiguousarray(out)


def test_numpy_plane_on_a_hand_made_world():
    """(no GPU work) the model above on a world small enough to reason about: one brick, sun along +x with small +y and +z slopes"""
    occ = np.zeros((6, 6, 8), bool)
    occ[2, 3, 6] = True
    plan = dict(valid=1, octant=0, dom=0, m1=1, m2=2, lo1=0, hi1=1, lo2=0, hi2=1, clear=1, rise=20, bins=4)
    p = numpy_sun_plane(occ, plan)
    assert p[2, 3, 6] == 0 and p[2, 3, 5] == 1 and p[2, 2, 5] == 1 and p[1, 2, 5] == 1, "cells from which the brick is one move away"
    assert p[2, 3, 4] == 2 and p[2, 3, 0] >= 3, "nothing before the brick's slab"
    assert p[3, 3, 0] == 255 and (p[3:] == 255).all() and (p[:, 4:, :] == 255).all() and (p[:, :, 7] == 255).all(), "above, beside and behind the brick nothing can be hit"
    assert p[2, 3, 0] != 255 and p[0, 2, 0] != 255 and p[0, 0, 0] == 255, "(0, 0) cannot reach the brick's column: at most 3 + 6 bins along y"


# ---------------------------------------------------------------- helpers
def params(bm, sun, flags=0, sample_base=0):
    return bm.FrameParams(W, H, spp=1, sample_base=sample_base, max_bounces=MB, flags=flags, sun_position=sun)


def camera_over(bm, g, h):
    return bm.Camera(position=(g / 2, g / 8, 0.8 * h), horizontal_angle=0.8, vertical_angle=-0.5).update()


def render_once(bm, torch, scene, cam, sun):
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    scene.render(cam, params(bm, sun), acc)
    torch.cuda.synchronize()
    return acc.cpu().numpy()


def assert_plane(scene, sun, what):
    plane, plan = scene.sun_plane()
    assert plane is not None and plan["valid"] == 1, f"{what}: no sun plane was built"
    d = np.abs(sun_direction(sun))
    assert plan["dom"] == int(d.argmax()) and plan["octant"] == sum(1 << k for k in range(3) if sun_direction(sun)[k] < 0)
    others = [k for k in range(3) if k != plan["dom"]]
    for k, (lo, hi) in zip(others, ((plan["lo1"], plan["hi1"]), (plan["lo2"], plan["hi2"]))):
        slope = d[k] / d[plan["dom"]] * plan["bins"]
        assert lo <= slope <= hi and hi - lo <= 2, f"{what}: bins {lo}..{hi} per slab for a slope of {slope:.2f} bins"
    assert (plane[0] == 255).all() and (plane[-1] == 255).all() and (plane[:, 0] == 255).all() and (plane[:, :, -1] == 255).all(), f"{what}: border"
    got, want = plane[1:-1, 1:-1, 1:-1], numpy_sun_plane(device_occupancy(scene), plan)
    assert np.array_equal(got, want), f"{what}: {np.count_nonzero(got != want)} of {want.size} bytes differ from the rules"
    return got


# ---------------------------------------------------------------- 5.1 the plane
@pytest.mark.parametrize("world", list(WORLDS))
def test_plane_equals_the_rules(world, bm, torch_cuda, terrain):
    torch = torch_cuda
    g, h = WORLDS[world]
    cam = camera_over(bm, g, h)
    s = bm.Scene(g, h, device=0).generate().preload_all()
    assert s.sun_plane()[0] is None and s.sun_plane_stats()[0] == 0, "built by the first frame that reads it"
    render_once(bm, torch, s, cam, SUN_X)
    first = assert_plane(s, SUN_X, "generate")
    assert (first == 255).any() and ((first >= 4) & (first < 255)).any() and (first == 0).any()
    s.close()
    s = bm.Scene.from_voxels(torch.from_numpy(terrain[world].astype(np.uint8)).to("cuda:0"))
    render_once(bm, torch, s, cam, SUN_X)
    assert np.array_equal(assert_plane(s, SUN_X, "load_voxels"), first)
    # a brick in a cell that read 255, with stamped cells between it and where the sun's rays come from: they are no longer clear
    zs, ys, xs = np.nonzero(first[:, 2:-2, 2:-2] == 255)
    k = int(np.argmin(zs * 4096 + np.abs(ys - len(first[0]) // 2) + np.abs(xs - len(first[0]) // 2)))  # the lowest such cell, near the middle
    cz, cy, cx = int(zs[k]), int(ys[k]) + 2, int(xs[k]) + 2
    s.fill_box((cx * 8, cy * 8, cz * 8), (cx * 8 + 8, cy * 8 + 8, cz * 8 + 8))
    render_once(bm, torch, s, cam, SUN_X)
    edited = assert_plane(s, SUN_X, "edit")
    assert edited[cz, cy, cx] == 0 and ((first == 255) & (edited != 255) & (edited != 0)).any(), "the brick shadows cells that were clear"
    s.clear_box((cx * 8, cy * 8, cz * 8), (cx * 8 + 8, cy * 8 + 8, cz * 8 + 8))
    render_once(bm, torch, s, cam, SUN_X)
    assert np.array_equal(assert_plane(s, SUN_X, "edit undone"), first)
    # a region write: a floating slab over a corner of the world
    slab = np.ones((8, 40, 48), np.uint8)
    s.write_region((g // 2 - 20, g // 2 - 30, h - 24), slab)
    render_once(bm, torch, s, cam, SUN_X)
    assert not np.array_equal(assert_plane(s, SUN_X, "region write"), first)
    # the sun moves: another plan, another plane
    for sun in (SUN_Y, SUN_Z, SUN_LOW):
        render_once(bm, torch, s, cam, sun)
        assert_plane(s, sun, f"sun {sun}")
    s.close()


# ---------------------------------------------------------------- 5.2 frames
def frames(bm, torch, scene, cam, sun):
    """the frame four ways: instrumented (ordered, with hit records), production ordered, production with helper lanes, and the hit records"""
    def zeros(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device="cuda:0")
    inst, dbg, prod, helped = zeros(H, W, 4), zeros(H, W, 8, dtype=torch.int32), zeros(H, W, 4), zeros(H, W, 4)
    scene.render(cam, params(bm, sun, bm.BM_FLAG_ORDERED), inst, debug=dbg)
    scene.render(cam, params(bm, sun, bm.BM_FLAG_ORDERED), prod)
    scene.render(cam, params(bm, sun), helped)
    torch.cuda.synchronize()
    return inst.cpu().numpy(), prod.cpu().numpy(), helped.cpu().numpy(), dbg.cpu().numpy().view(np.uint32)


def check_frames(bm, torch, scene, cam, sun, what):
    inst, prod, helped, dbg = frames(bm, torch, scene, cam, sun)
    assert np.array_equal(prod.view(np.uint32), inst.view(np.uint32)), f"{what}: {np.count_nonzero((prod != inst).any(-1))} pixels of the ordered production frame differ from the instrumented one"
    assert np.array_equal(helped[..., 3], inst[..., 3]), f"{what}: alpha of the helper-lane frame differs"
    err, bound = float(np.abs(helped[..., :3] - inst[..., :3]).max()), RGB_TOL * float(np.abs(inst[..., :3]).max())
    print(f"{what}: helper-lane frame max |rgb difference| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: radiance of the helper-lane frame differs: {err:.3e} > {bound:.3e}"
    hit = dbg[..., 1] != 0
    assert hit.sum() > W * H // 4, f"{what}: the view shows too little terrain for its shadow rays to mean anything"
    return inst


@pytest.fixture(scope="module")
def overhang_scene(bm, torch_cuda, terrain):
    """the cube terrain with a slab floating between the surface and the sun, over the part of the world the camera looks at"""
    g, h = WORLDS["cube"]
    vox = terrain["cube"].copy()
    vox[h - 24:h - 16, g // 8:g // 2, g // 4:g // 4 * 3] = True
    scene = bm.Scene.from_voxels(torch_cuda.from_numpy(vox.astype(np.uint8)).to("cuda:0"))
    yield scene
    scene.close()


@pytest.mark.parametrize("sun,name,valid", [(SUN_X, "default sun", True), (SUN_LOW, "very low sun", True), (SUN_Z, "z dominant", True), (SUN_Y, "y dominant", True),
                                            (SUN_ACROSS, "cone across an octant boundary", False)])
def test_frames_under_an_overhang(sun, name, valid, bm, torch_cuda, overhang_scene):
    g, h = WORLDS["cube"]
    scene = overhang_scene
    builds = scene.sun_plane_stats()[0]
    lit = check_frames(bm, torch_cuda, scene, camera_over(bm, g, h), sun, name)
    plane, plan = scene.sun_plane()
    if valid:
        assert scene.sun_plane_stats()[0] == builds + 1, "a new sun: one build"
        # under the slab the plane says neither "clear" nor "occupied": shadow rays from there are walked and meet the slab
        below = plane[1:-1, 1:-1, 1:-1][(h - 24) // 8 - 1, g // 8 // 8 + 1:g // 2 // 8 - 1, g // 4 // 8 + 1:g // 4 * 3 // 8 - 1]
        assert ((below != 255) | (below == 0)).all() and plan["valid"] == 1
        assert float(lit[..., :3].max()) > 0
    else:
        assert scene.sun_plane_stats()[0] == builds, "no plane for this sun: nothing is built, the frames use the octant planes"


def test_ring_of_two_suns(bm, torch_cuda, overhang_scene):
    """two frames with different suns as one launch: a wave-level ring; the plane is the first frame's, the second keeps its octant planes"""
    torch = torch_cuda
    g, h = WORLDS["cube"]
    scene, cam = overhang_scene, camera_over(bm, g, h)
    for flags in (bm.BM_FLAG_ORDERED, 0):
        want = []
        for k, sun in enumerate((SUN_X, SUN_Y)):
            inst = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
            dbg = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda:0")
            scene.render(cam, params(bm, sun, bm.BM_FLAG_ORDERED, sample_base=k), inst, debug=dbg)
            want.append(inst)
        got = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
        scene.render_frames(cam, [params(bm, sun, flags, sample_base=k) for k, sun in enumerate((SUN_X, SUN_Y))], got)
        torch.cuda.synchronize()
        assert scene.sun_plane()[1]["dom"] == 0, "the plane is the first frame's"
        for k in range(2):
            a, b = got[k].cpu().numpy(), want[k].cpu().numpy()
            assert np.array_equal(a[..., 3], b[..., 3])
            if flags:
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"ordered ring, frame {k}"
            else:
                assert float(np.abs(a[..., :3] - b[..., :3]).max()) <= RGB_TOL * float(np.abs(b[..., :3]).max()), f"helper-lane ring, frame {k}"


# ---------------------------------------------------------------- 5.3 the build counter
def test_build_counter(bm, torch_cuda, terrain):
    torch = torch_cuda
    g, h = WORLDS["cube"]
    scene = bm.Scene.from_voxels(torch.from_numpy(terrain["cube"].astype(np.uint8)).to("cuda:0"))
    cam = camera_over(bm, g, h)
    render_once(bm, torch, scene, cam, SUN_X)
    builds, ms = scene.sun_plane_stats()
    assert builds == 1 and ms > 0
    info, cells = scene.info(), g // 8
    # the ninth plane and the build's scratch: first stamped cell per column, two slabs of clear heights and of face values (16 bins per cell)
    assert info["sun_plane_bytes"] == info["cube_field_bytes"] // 8 + 4 * cells * cells + 2 * 4 * 4 * cells + 2 * 16 * cells * (h // 8)
    for k in range(3):
        render_once(bm, torch, scene, cam, SUN_X)
    assert scene.sun_plane_stats()[0] == 1, "same sun, same world: the plane stands"
    scene.edit([bm.edit_box(bm.BM_EDIT_SET, (8, 8, h - 16), (16, 16, h - 8)), bm.edit_box(bm.BM_EDIT_SET, (40, 40, h - 16), (48, 48, h - 8))])
    assert scene.sun_plane_stats()[0] == 1, "an edit alone builds nothing"
    render_once(bm, torch, scene, cam, SUN_X)
    render_once(bm, torch, scene, cam, SUN_X)
    assert scene.sun_plane_stats()[0] == 2, "one edit batch: one rebuild, by the next frame"
    scene.close()
