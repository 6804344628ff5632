"""Escape heights on the MI355X (csrc/escape.h, escape.hip; the rule's CPU replay is tests/test_escape_rule.py).

4.1  The table the device holds (bm_scene_escape_table) equals a numpy table computed from the device's index words, after generate,
     after load_voxels, after an edit that adds a brick high in the far corner of a quadrant, after the edit that removes it again, and
     after a region write across a chunk edge -- on the smallest world (128^3), a tall one (128 x 128 x 256) and a flat one (256 x 256 x 128).
4.2  Ordered frames of the production instantiation -- whose rays end at their escape point -- equal the instrumented one's bit for
     bit (the instrumented kernel never escapes: it walks every ray to the border like the reference), and alpha and hit records equal
     the oracle's, for scenes chosen by what the rule can get wrong.  The scenes are built with load_voxels from the terrain's own voxels
     less what a scene clears; the oracle's world, which cannot gain bricks, is the terrain cleared the same way (test_gpu_edit
     oracle_clear) -- and for the one scene that needs a brick where the terrain has none, a cleared world whose first brick slot is
     rewritten and named by the far corner cell's index word.
4.3  Helper-lane frames (the kernel bench.py times) as a uniform ring launch of 5: alpha exact, radiance within 1e-5 of the ordered frames.
4.4  After the adding edit, frames change in the pixels that now hit and still equal the instrumented frames.
Frames are 64 x 64 at most, 1 spp, 4 segments."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_edit import oracle_clear

pytestmark = pytest.mark.gpu

WORLDS = {"cube": (128, 128), "tall": (128, 256), "flat": (256, 128)}
W = H = 64
MB = 3
RGB_TOL = 1e-5  # of the frame's largest value: same paths, another order of the float-atomic additions (test_gpu_frame_groups.py)


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


# ---------------------------------------------------------------- 4.1 the table
def device_occupancy(scene):
    """bool [z, y, x] over brick cells: the device's index word is non-zero"""
    info = scene.info()
    sg, sgz = info["supergrid_xy"], info["supergrid_z"]
    occ = np.zeros((sgz * 16, sg * 16, sg * 16), bool)
    for sc in range(info["supercells"]):
        sx, sy, sz = sc % sg, (sc // sg) % sg, sc // (sg * sg)
        occ[sz * 16:sz * 16 + 16, sy * 16:sy * 16 + 16, sx * 16:sx * 16 + 16] = scene.device_indices(sc).reshape(16, 16, 16) != 0
    return occ


def numpy_table(occ):
    """int32 [8, cells, cells] (octant, y, x): the definition of include/brickmap.h bm_scene_escape_table, by brute force over the quadrant's columns
    (as running maxima / minima of the column tops / bottoms along the flipped axes)"""
    nz = occ.shape[0]
    z = np.arange(nz).reshape(-1, 1, 1)
    top = np.where(occ, z, -1).max(axis=0)
    bottom = np.where(occ, z, nz).min(axis=0)
    out = np.zeros((8,) + top.shape, np.int32)
    for o in range(8):
        a, fold = (bottom, np.minimum) if o & 4 else (top, np.maximum)
        # quadrant of octant o from (x, y): x' >= x unless bit 0 is set (then x' <= x), y' likewise with bit 1
        if not o & 1:
            a = a[:, ::-1]
        if not o & 2:
            a = a[::-1, :]
        a = fold.accumulate(fold.accumulate(a, axis=0), axis=1)
        if not o & 2:
            a = a[::-1, :]
        if not o & 1:
            a = a[:, ::-1]
        out[o] = a
    return out


def test_numpy_table_is_the_definition():
    """(no GPU work: the model above against the definition as four nested loops, on a small random occupancy)"""
    rng = np.random.default_rng(5)
    occ = rng.random((5, 6, 6)) < 0.08
    got = numpy_table(occ)
    for o in range(8):
        for y in range(6):
            for x in range(6):
                xs = slice(None, x + 1) if o & 1 else slice(x, None)
                ys = slice(None, y + 1) if o & 2 else slice(y, None)
                zs = np.nonzero(occ[:, ys, xs])[0]
                want = (zs.min() if len(zs) else 5) if o & 4 else (zs.max() if len(zs) else -1)
                assert got[o, y, x] == want, (o, x, y)


def assert_table(scene, what):
    got, want = scene.escape_table(), numpy_table(device_occupancy(scene))
    assert got.shape == want.shape and np.array_equal(got, want), f"{what}: {np.count_nonzero(got != want)} of {want.size} escape heights differ"
    return got


@pytest.mark.parametrize("world", list(WORLDS))
def test_table_equals_the_index_words(world, bm, torch_cuda, terrain):
    torch = torch_cuda
    g, h = WORLDS[world]
    cells_h = h // 8
    s = bm.Scene(g, h, device=0).generate()
    first = assert_table(s, "generate")
    assert len(np.unique(first[0])) > 1, "the terrain's table is not trivial"
    s.preload_all()
    assert np.array_equal(assert_table(s, "preload_all"), first)
    info = s.info()
    assert info["escape_bytes"] == info["cube_field_bytes"] // (cells_h + 2) * 4  # 8 octants x one 32-bit entry per byte of a field slice
    s.close()
    # load_voxels, device route: the same world, the same table
    s = bm.Scene.from_voxels(torch.from_numpy(terrain[world].astype(np.uint8)).to("cuda:0"))
    assert np.array_equal(assert_table(s, "load_voxels"), first)
    # a brick high in the far corner of octant 0's quadrant: every column of that octant sees it
    corner = np.array([[g - 1, g - 1, h - 1]], np.int32)
    s.set_voxels(corner, 1)
    added = assert_table(s, "adding edit")
    assert (added[0] == cells_h - 1).all() and not np.array_equal(added[:4], first[:4])
    s.set_voxels(corner, 0)
    assert np.array_equal(assert_table(s, "removing edit"), first)
    # a region write across a chunk edge (flat: the supercell edge at x = 128; tall: at z = 128; cube: the only chunk's edge = the world's,
    # where the box is clipped): the box's voxels inverted -- air becomes bricks, solid bricks go -- then the terrain put back
    lo = {"flat": (120, 40, h - 40), "tall": (40, 60, 120), "cube": (g - 10, 30, h - 40)}[world]
    before = s.read_region(lo, (lo[0] + 16, lo[1] + 20, lo[2] + 32)).astype(np.uint8)
    assert before.shape == (32, 20, 16)
    occ = device_occupancy(s)
    s.write_region(lo, np.ascontiguousarray(1 - before))
    assert_table(s, "region write")
    assert not np.array_equal(device_occupancy(s), occ), "the region write changed no cell's occupancy"
    s.write_region(lo, before)
    assert np.array_equal(assert_table(s, "region write back"), first)
    s.close()


# ---------------------------------------------------------------- 4.2 frames
def camera(bm, position, direction, up=(0.0, 0.0, 1.0)):
    n = math.sqrt(sum(v * v for v in direction))
    return bm.Camera(position=tuple(float(v) for v in position), direction=tuple(float(v / n) for v in direction), up=up)


def frames(bm, torch, scene, cam, sample_base=0):
    """the ordered frame three times: instrumented with hit records, production (ends rays at their escape point), and the accumulators"""
    def zeros(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device="cuda:0")
    p = bm.FrameParams(W, H, spp=1, sample_base=sample_base, max_bounces=MB, flags=bm.BM_FLAG_ORDERED)
    inst, dbg, prod = zeros(H, W, 4), zeros(H, W, 8, dtype=torch.int32), zeros(H, W, 4)
    scene.render(cam, p, inst, debug=dbg)
    scene.render(cam, p, prod)
    torch.cuda.synchronize()
    return inst.cpu().numpy(), dbg.cpu().numpy().view(np.uint32), prod.cpu().numpy()


def check_scene(bm, orc, torch, scene, world, cam, what):
    inst, dbg, prod = frames(bm, torch, scene, cam)
    assert np.array_equal(prod.view(np.uint32), inst.view(np.uint32)), f"{what}: {np.count_nonzero((prod != inst).any(-1))} pixels of the production frame differ from the instrumented one"
    oacc, odbg, _, _ = world.render(orc.make_camera(cam.position, cam.direction, up=cam.up), orc.make_frame(W, H, spp=1, max_bounces=MB))
    assert np.array_equal(dbg, odbg), f"{what}: {np.count_nonzero((dbg != odbg).any(-1))} pixels whose hit records differ from the oracle's"
    assert np.array_equal(prod[..., 3], oacc[..., 3]), f"{what}: alpha differs from the oracle's"
    err = np.abs(prod - oacc) / np.maximum(np.abs(oacc), 1e-6)
    assert float(err.max()) <= 1e-4, f"{what}: radiance differs from the oracle's: {err.max():.3e}"
    hit = dbg[..., 1] != 0
    return hit, prod


def build(bm, orc, torch, name, vox, remove=None):
    """product scene (load_voxels, device route) and oracle world of the terrain `vox` less `remove`"""
    g, h = WORLDS[name]
    keep = vox if remove is None else vox & ~remove
    scene = bm.Scene.from_voxels(torch.from_numpy(keep.astype(np.uint8)).to("cuda:0"))
    world = orc.World(g, h)
    if remove is not None:
        oracle_clear(world, remove)
    world.reset_device(True)
    return scene, world


def tops_of(vox):
    z = np.arange(vox.shape[0]).reshape(-1, 1, 1)
    return np.where(vox, z, -1).max(axis=0)  # [y, x]: highest solid voxel of the column


@pytest.mark.parametrize("world", list(WORLDS))
def test_camera_above_the_terrain(world, bm, orc, torch_cuda, terrain):
    """every upward primary ray has escaped where it starts; the downward ones walk as before -- in every world shape"""
    g, h = WORLDS[world]
    vox = terrain[world]
    top = int(tops_of(vox).max())
    assert top + 10 < h, "the terrain leaves no room above it"
    scene, w = build(bm, orc, torch_cuda, world, vox)
    table = scene.escape_table()
    cz = top + 9
    assert (table[:4] < cz // 8).all()
    hit, _ = check_scene(bm, orc, torch_cuda, scene, w, camera(bm, (g / 2 + 0.3, g / 2 + 0.7, cz), (1.0, 0.8, 0.02)), "camera above the terrain")
    assert hit.any() and not hit.all(), "the view shows terrain and sky"
    scene.close()


def test_camera_above_its_own_quadrant_only(bm, orc, torch_cuda, terrain):
    """the camera is below the world's top, but the terrain of the quadrant it looks into is cut down below it"""
    g, h = WORLDS["cube"]
    vox = terrain["cube"]
    tops = tops_of(vox)
    cz = int(tops.max()) - 6
    ym, xm = np.unravel_index(int(tops.argmax()), tops.shape)  # the highest column stays: the camera stands 12 voxels beside it and looks away from it
    sx = 1 if xm < g // 2 else -1
    px = int(xm) + 12 * sx
    remove = np.zeros_like(vox)
    if sx > 0:
        remove[cz - 10:, :, px - 8:] = True
    else:
        remove[cz - 10:, :, :px + 8] = True
    assert cz - 10 > 8 and 16 <= px < g - 16
    scene, w = build(bm, orc, torch_cuda, "cube", vox, remove)
    table = scene.escape_table()
    ahead, behind = (0, 1) if sx > 0 else (1, 0)  # octants by their x direction (y either way: the whole half is cut down)
    assert max(table[ahead, 64 // 8, px // 8], table[ahead | 2, 64 // 8, px // 8]) < cz // 8 <= max(table[behind, 64 // 8, px // 8], table[behind | 2, 64 // 8, px // 8]), \
        "escaped in the octants it looks into, not in the opposite ones (the highest column lies in one of those)"
    for direction in ((sx * 1.0, 0.9, 0.25), (-sx * 1.0, -0.8, 0.1), (sx * 1.0, -0.02, 0.0)):
        check_scene(bm, orc, torch_cuda, scene, w, camera(bm, (px + 0.4, 64.6, cz + 0.5), direction), f"camera above its quadrant, looking {direction}")
    scene.close()


def test_floating_slab_above_the_camera(bm, orc, torch_cuda, terrain):
    """a gap is cut through the hills: what is left above it floats, and upward rays from inside the gap must still find it"""
    g, h = WORLDS["cube"]
    vox = terrain["cube"]
    tops = tops_of(vox)
    b = int(np.percentile(tops, 70))
    a = b - 20
    assert a > 4 and int(tops.max()) > b + 4
    remove = np.zeros_like(vox)
    remove[a:b] = True
    y, x = np.unravel_index(int(tops.argmax()), tops.shape)
    scene, w = build(bm, orc, torch_cuda, "cube", vox, remove)
    cam = camera(bm, (x + 0.5, y + 0.5, b - 9.5), (0.3, 0.2, 1.0), up=(0.0, 1.0, 0.0))
    hit, _ = check_scene(bm, orc, torch_cuda, scene, w, cam, "floating slab")
    assert hit[H // 2 - 4:H // 2 + 4, W // 2 - 4:W // 2 + 4].any(), "rays through the middle of the frame hit the slab's underside"
    check_scene(bm, orc, torch_cuda, scene, w, camera(bm, (x + 0.5, y + 0.5, b - 9.5), (1.0, 0.7, 0.3)), "floating slab, sideways")
    scene.close()


def test_one_brick_in_the_far_top_corner_and_the_empty_world(bm, orc, torch_cuda, terrain):
    g, h = WORLDS["cube"]
    vox = terrain["cube"]
    everything = np.ones_like(vox)
    # ---- the empty world: every ray has escaped where it starts
    scene, w = build(bm, orc, torch_cuda, "cube", vox, everything)
    table = scene.escape_table()
    assert (table[:4] == -1).all() and (table[4:] == h // 8).all()
    for direction in ((1.0, 1.0, 1.0), (-0.3, 0.5, -1.0)):
        hit, prod = check_scene(bm, orc, torch_cuda, scene, w, camera(bm, (40.5, 41.5, 42.5), direction), "empty world")
        assert not hit.any() and (prod[..., 3] == 1).all()
    scene.close()
    # ---- one full brick in the far top corner cell: the oracle's first brick slot, rewritten, named by that cell's index word
    one = np.zeros_like(vox)
    one[h - 8:, g - 8:, g - 8:] = True
    scene = bm.Scene.from_voxels(torch_cuda.from_numpy(one.astype(np.uint8)).to("cuda:0"))
    idx = np.ctypeslib.as_array(C.cast(w.L.orc_world_sc_indices(w.h, 0), C.POINTER(C.c_uint32)), shape=(4096,))
    bricks = np.ctypeslib.as_array(C.cast(w.L.orc_world_sc_bricks(w.h, 0), C.POINTER(C.c_uint32)), shape=(w.sc_nbricks(0), 16))
    assert not idx.any()
    bricks[0] = 0xFFFFFFFF
    idx[4095] = np.uint32(0x80000000 | (0xFF << 12) | 0)
    w.reset_device(True)
    table = scene.escape_table()
    assert (table[0] == h // 8 - 1).all() and (table[1, :, :-1] == -1).all()
    hit, _ = check_scene(bm, orc, torch_cuda, scene, w, camera(bm, (40.5, 41.5, 42.5), (1.0, 0.99, 0.98)), "one brick in the far top corner")
    assert hit.any() and not hit.all(), "the brick is in view, and so is the sky around it"
    hit, _ = check_scene(bm, orc, torch_cuda, scene, w, camera(bm, (g - 4.5, g - 3.5, 8.5), (0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)), "under the corner brick")
    assert hit.any()
    scene.close()


def test_cameras_along_the_axes(bm, orc, torch_cuda, terrain):
    """a camera looking exactly horizontally (the middle rays have dz == 0: the rule of the octants that do not move down) and one looking exactly along +z"""
    g, h = WORLDS["cube"]
    vox = terrain["cube"]
    tops = tops_of(vox)
    scene, w = build(bm, orc, torch_cuda, "cube", vox)
    cz = int(np.percentile(tops, 60)) + 0.5
    y, x = np.unravel_index(int(tops.argmin()), tops.shape)
    for direction in ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0)):
        hit, _ = check_scene(bm, orc, torch_cuda, scene, w, camera(bm, (x + 0.5, y + 0.5, max(cz, tops[y, x] + 2.5)), direction), f"horizontal camera {direction}")
    assert hit.any() and not hit.all()
    check_scene(bm, orc, torch_cuda, scene, w, camera(bm, (x + 0.5, y + 0.5, tops[y, x] + 2.5), (0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)), "camera along +z")
    # straight up from a cell face: x, y and z on cell borders
    check_scene(bm, orc, torch_cuda, scene, w, camera(bm, (64.0, 72.0, float((int(tops[72, 64]) // 8 + 1) * 8)), (0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)), "camera along +z from a cell corner")
    scene.close()


# ---------------------------------------------------------------- 4.3 / 4.4
def test_helper_lane_ring_of_five(bm, torch_cuda, terrain):
    """the kernel the benchmark times: five production frames as one uniform ring launch against the five ordered frames"""
    torch = torch_cuda
    g, h = WORLDS["cube"]
    vox = terrain["cube"]
    scene = bm.Scene.from_voxels(torch.from_numpy(vox.astype(np.uint8)).to("cuda:0"))
    cam = camera(bm, (g / 2 + 0.3, g / 2 + 0.7, int(tops_of(vox).max()) + 9), (1.0, 0.8, 0.02))  # above the terrain: a sixth of the frame hits it
    ref = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    dbg = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda:0")
    for k in range(5):
        scene.render(cam, bm.FrameParams(W, H, spp=1, sample_base=k, max_bounces=MB, flags=bm.BM_FLAG_ORDERED), ref, debug=dbg)
    got = torch.zeros_like(ref)
    scene.render_frames(cam, [bm.FrameParams(W, H, spp=1, sample_base=k, max_bounces=MB) for k in range(5)], got)
    torch.cuda.synchronize()
    got, ref = got.cpu().numpy(), ref.cpu().numpy()
    assert np.array_equal(got[..., 3], ref[..., 3]) and ref[..., 3].min() >= 5, "terminated-path counts differ"
    err, bound = float(np.abs(got[..., :3] - ref[..., :3]).max()), RGB_TOL * float(np.abs(ref[..., :3]).max())
    print(f"helper-lane ring of 5: max |rgb difference| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    sky = dbg.cpu().numpy().view(np.uint32)[..., 1] == 0
    assert sky.any() and not sky.all()
    scene.close()


def test_frames_after_the_adding_edit(bm, torch_cuda, terrain):
    """a brick appears where rays used to escape: the pixels that now hit it change, and the production frame is still the instrumented one"""
    torch = torch_cuda
    g, h = WORLDS["cube"]
    vox = terrain["cube"]
    scene = bm.Scene.from_voxels(torch.from_numpy(vox.astype(np.uint8)).to("cuda:0"))
    top = int(tops_of(vox).max())
    cam = camera(bm, (g / 2 + 0.5, g / 2 + 0.5, top + 4.5), (g / 2 - 4.0, g / 2 - 4.0, h - 4.0 - (top + 4.5)))  # at the far top corner
    inst0, dbg0, prod0 = frames(bm, torch, scene, cam)
    assert np.array_equal(prod0.view(np.uint32), inst0.view(np.uint32)) and (dbg0[H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2, 1] == 0).all()
    scene.fill_box((g - 8, g - 8, h - 8), (g, g, h))
    inst1, dbg1, prod1 = frames(bm, torch, scene, cam)
    assert np.array_equal(prod1.view(np.uint32), inst1.view(np.uint32)), "after the edit the production frame differs from the instrumented one"
    corner = (g // 8 - 1) + (g // 8 - 1) * (g // 8) + (h // 8 - 1) * (g // 8) ** 2
    now_hit = (dbg1[..., 1] != 0) & (dbg1[..., 2] == corner)
    assert now_hit[H // 2:H // 2 + 2, W // 2:W // 2 + 2].all() and 8 <= now_hit.sum() < 200, "the middle of the frame shows the new brick (a few pixels wide from here)"
    changed = (prod1 != prod0).any(-1)
    assert changed[now_hit].all() and np.array_equal(dbg1[~now_hit][:, :4], dbg0[~now_hit][:, :4]), "first hits change exactly where the brick is seen"
    scene.close()
