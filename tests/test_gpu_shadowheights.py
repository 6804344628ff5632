"""Shadow heights on the MI355X (csrc/shadowheight.h, sunfield.hip, traverse.h ray_setup; the rule's CPU replay is tests/test_shadowheight_rule.py).

6.1  The table the device holds (bm_scene_shadow_heights) equals the rule written in numpy (numpy_dark_heights below, on the device's own
     index words and voxels and the plan the device reports): after generate, after load_voxels, after an edit that empties one voxel of
     every bottom brick of a shadowing slab -- no cell's occupancy changes, the sun plane stands, the slice alone is rebuilt --, its undoing, a
     region write, changes of sun (a z-dominant sun: all zero), reset_residency (all zero: a streaming scene has none) and preload_all, in a
     cube, a flat and a tall world.
6.2  Frames of the production instantiations -- whose shadow rays end at set-up below the shadow height -- against the instrumented one's,
     which never reads the table: ordered frames bit for bit, helper-lane frames with alpha exact and radiance within the bound
     test_gpu_sunfield uses for the same comparison.  Scenes: two walls with one-cell notches, an overhang, a hollow mountain and partly
     filled top bricks, each under an x- and a y-dominant sun; a sun whose cone crosses an octant boundary (no plane, no slice read); a
     ring of two suns.  Every scene asserts from the numpy model that shadow rays of surface cells the camera sees end at set-up.
Frames are 64 x 48, 1 spp, 4 segments; worlds of 128^3 to 256 x 256 x 128 voxels."""
import numpy as np
import pytest

from test_gpu_escape import RGB_TOL
from test_gpu_sunfield import SUN_ACROSS, SUN_LOW, SUN_X, SUN_Y, SUN_Z, WORLDS, camera_over

pytestmark = pytest.mark.gpu

W, H = 64, 48
MB = 3
LOADED, LOD_BITS = 0x80000000, 0xFF000
UNIT, MARGIN = 256, 4  # kSunHeightUnit, kSunHeightMargin


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


# ---------------------------------------------------------------- the rule in numpy
def device_full(scene):
    """bool [z, y, x] over brick cells: the device's index word says resident with all eight LoD bits, and all 512 voxels read back set"""
    info = scene.info()
    sg, sgz = info["supergrid_xy"], info["supergrid_z"]
    word_ok = np.zeros((sgz * 16, sg * 16, sg * 16), bool)
    for sc in range(info["supercells"]):
        sx, sy, sz = sc % sg, (sc // sg) % sg, sc // (sg * sg)
        idx = scene.device_indices(sc).reshape(16, 16, 16)
        word_ok[sz * 16:sz * 16 + 16, sy * 16:sy * 16 + 16, sx * 16:sx * 16 + 16] = ((idx & LOADED) != 0) & ((idx & LOD_BITS) == LOD_BITS)
    g, h = scene.grid_size, scene.grid_height
    vox = np.asarray(scene.read_region((0, 0, 0), (g, g, h))).astype(bool)
    solid = vox.reshape(h // 8, 8, g // 8, 8, g // 8, 8).all(axis=(1, 3, 5))
    return word_ok & solid


def numpy_dark_heights(full, plan, splan):
    """int64 [y, x]: Zd of csrc/shadowheight.h for the full cells `full` [z, y, x], the sun plane's plan and the shadow plan (rise_hi)"""
    nz, ny, nx = full.shape
    if not splan["valid"]:
        return np.zeros((ny, nx), np.int64)
    B, dom, m1, octant, lo, hi, rise_hi = plan["bins"], plan["dom"], plan["m1"], plan["octant"], plan["lo1"], plan["hi1"], splan["rise_hi"]
    assert plan["clear"] and dom in (0, 1) and m1 == 1 - dom

    def directed2(a):  # [y, x] -> [ud, u1], and back (flips and a 2-D transpose are their own inverses, applied in reverse order)
        for axis in range(2):
            if octant >> axis & 1:
                a = np.flip(a, 1 - axis)
        return np.transpose(a, (1 - dom, 1 - m1))

    top = directed2(np.cumprod(full, axis=0).sum(axis=0).astype(np.int64)) * UNIT  # full from the ground up without a gap
    nd, n1 = top.shape
    w = np.arange(n1)
    zd = np.zeros((nd, n1), np.int64)
    sn = np.zeros((n1 + 2, B), np.int64)  # S of the slab behind; outside the grid 0
    for ud in range(nd - 1, -1, -1):
        least = np.full(n1, 1 << 30, np.int64)
        for g in range(0, B + hi):
            least = np.minimum(least, sn[w + g // B, g % B])
        t = least - rise_hi - MARGIN
        zd[ud] = np.minimum(np.where(t > 0, (t - 1) // UNIT, 0), nz)
        sc = np.zeros_like(sn)
        for b in range(B):
            m = np.full(n1, 1 << 30, np.int64)
            for g in range(b + lo, b + hi + 1):
                m = np.minimum(m, sn[w + g // B, g % B])
            sc[:n1, b] = np.maximum(top[ud], m - rise_hi)
        sn = sc
    out = np.transpose(zd, (1 - dom, 1 - m1))
    for axis in range(2):
        if octant >> axis & 1:
            out = np.flip(out, 1 - axis)
    return np.ascontiguousarray(out)


def test_numpy_model_on_a_hand_made_world():
    """(no GPU work) a full wall of 6 cells at x = 6, sun along +x: rise_hi 64 of 256 per slab, so the shadow loses a quarter cell per slab"""
    full = np.zeros((8, 4, 8), bool)
    full[:6, :, 6] = True
    plan = dict(valid=1, octant=0, dom=0, m1=1, m2=2, lo1=0, hi1=1, lo2=0, hi2=1, clear=1, rise=20, bins=4)
    zd = numpy_dark_heights(full, plan, dict(valid=1, rise_hi=64))
    # column x = 5 enters the wall's slab next: cells with (z + 1) * 256 + 64 + 4 < 6 * 256, z = 0 ... 4; one slab further S is 64 less: still 5; four further, 4
    assert zd[1, 5] == 5 and zd[1, 4] == 5 and zd[1, 1] == 4 and (zd[:, 6:] == 0).all(), zd
    assert (zd[3] == 0).all(), "rays of the last row can leave the grid sideways (hi1 >= 1)"
    assert (numpy_dark_heights(full, plan, dict(valid=0, rise_hi=0)) == 0).all()


# ---------------------------------------------------------------- helpers
def params(bm, sun, flags=0, sample_base=0):
    return bm.FrameParams(W, H, spp=1, sample_base=sample_base, max_bounces=MB, flags=flags, sun_position=sun)


def render_once(bm, torch, scene, cam, sun):
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    scene.render(cam, params(bm, sun), acc)
    torch.cuda.synchronize()


def assert_slice(scene, what):
    """the device's table against the model; returns Zd [y, x]"""
    entries, splan, nbytes = scene.shadow_heights()
    plane, plan = scene.sun_plane()
    assert entries is not None and plane is not None, f"{what}: nothing was built"
    info = scene.info()
    cells, cells_h = scene.grid_size // 8, scene.grid_height // 8
    cf_plane = info["cube_field_bytes"] // 8
    pxy = cf_plane // (cells_h + 2)
    # the slice and the build's scratch: full tops per column, two slabs of S; none of it in the figures that were there before
    assert nbytes == 4 * pxy + 4 * cells * cells + 2 * 4 * 4 * cells, f"{what}: {nbytes} bytes"
    assert splan["valid"] == (1 if plan["clear"] else 0) and splan["unit"] == UNIT
    if splan["valid"]:
        assert splan["rise_hi"] > plan["rise"] == splan["rise"]
    zd = numpy_dark_heights(device_full(scene), plan, splan)
    want = np.where(zd > 0, 8 * cf_plane + (zd + 1) * pxy, 0).astype(np.uint32)
    assert np.array_equal(entries, want), f"{what}: {np.count_nonzero(entries != want)} of {want.size} entries differ from the rule"
    return zd


# ---------------------------------------------------------------- 6.1 the table
@pytest.mark.parametrize("world", list(WORLDS))
def test_slice_equals_the_rule(world, bm, torch_cuda, terrain):
    torch = torch_cuda
    g, h = WORLDS[world]
    cam = camera_over(bm, g, h)
    s = bm.Scene(g, h, device=0).generate().preload_all()
    assert s.shadow_heights()[0] is None, "built with the sun plane, by the first frame that reads it"
    render_once(bm, torch, s, cam, SUN_X)
    first = assert_slice(s, "generate")
    assert (first > 0).any() and (first == 0).any()
    s.close()
    s = bm.Scene.from_voxels(torch.from_numpy(terrain[world].astype(np.uint8)).to("cuda:0"))
    render_once(bm, torch, s, cam, SUN_X)
    assert np.array_equal(assert_slice(s, "load_voxels"), first)
    # one voxel out of the bottom brick of every column of one x slab (the slab whose loss changes the model's heights most): the slab's
    # full tops drop to 0, no cell's occupancy changes -- the sun plane stands (no build is counted), the slice alone is rebuilt
    full, (_, plan), splan = device_full(s), s.sun_plane(), s.shadow_heights()[1]

    def without(cx):
        f = full.copy()
        f[0, :, cx] = False
        return numpy_dark_heights(f, plan, splan)
    cx = max(range(g // 8), key=lambda c: int((first - without(c)).sum()))
    assert (without(cx) < first).any()
    builds = s.sun_plane_stats()[0]
    s.clear_box((cx * 8 + 3, 0, 3), (cx * 8 + 4, g, 4))
    render_once(bm, torch, s, cam, SUN_X)
    edited = assert_slice(s, "edit")
    assert s.sun_plane_stats()[0] == builds, "no occupancy changed: the plane stands"
    assert (edited <= first).all() and (edited < first).any(), "the column no longer shadows what it did"
    s.fill_box((cx * 8 + 3, 0, 3), (cx * 8 + 4, g, 4))
    render_once(bm, torch, s, cam, SUN_X)
    assert np.array_equal(assert_slice(s, "edit undone"), first)
    # a region write: a solid tower from the ground up
    s.write_region((g // 2 - 16, g // 2 - 16, 0), np.ones((h - 16, 32, 32), np.uint8))
    render_once(bm, torch, s, cam, SUN_X)
    tower = assert_slice(s, "region write")
    assert (tower >= first).all() and (tower > first).any()
    # the sun moves: another plan, another table; a z-dominant sun has none
    for sun in (SUN_Y, SUN_LOW):
        render_once(bm, torch, s, cam, sun)
        assert (assert_slice(s, f"sun {sun}") > 0).any()
    render_once(bm, torch, s, cam, SUN_Z)
    assert (assert_slice(s, "z dominant") == 0).all() and s.shadow_heights()[1]["valid"] == 0 and not s.shadow_heights()[0].any()
    # a scene that streams its bricks in has no shadow heights (a ray ended at set-up would request nothing); preloaded again, it has them back
    render_once(bm, torch, s, cam, SUN_X)
    assert s.shadow_heights()[0].any()
    s.reset_residency()
    render_once(bm, torch, s, cam, SUN_X)
    entries, splan, _ = s.shadow_heights()
    assert splan["valid"] == 0 and not entries.any(), "no shadow heights while bricks are streamed in"
    s.preload_all()
    render_once(bm, torch, s, cam, SUN_X)
    assert (assert_slice(s, "preloaded again") > 0).any()
    s.close()


# ---------------------------------------------------------------- 6.2 frames
def frames(bm, torch, scene, cam, sun):
    """the frame three ways: instrumented (ordered, with hit records), production ordered, production with helper lanes"""
    def zeros(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device="cuda:0")
    inst, dbg, prod, helped = zeros(H, W, 4), zeros(H, W, 8, dtype=torch.int32), zeros(H, W, 4), zeros(H, W, 4)
    scene.render(cam, params(bm, sun, bm.BM_FLAG_ORDERED), inst, debug=dbg)
    scene.render(cam, params(bm, sun, bm.BM_FLAG_ORDERED), prod)
    scene.render(cam, params(bm, sun), helped)
    torch.cuda.synchronize()
    return inst.cpu().numpy(), prod.cpu().numpy(), helped.cpu().numpy()


def check_frames(bm, torch, scene, cam, sun, what):
    inst, prod, helped = frames(bm, torch, scene, cam, sun)
    assert np.array_equal(prod.view(np.uint32), inst.view(np.uint32)), f"{what}: {np.count_nonzero((prod != inst).any(-1))} pixels of the ordered production frame differ from the instrumented one"
    assert np.array_equal(helped[..., 3], inst[..., 3]), f"{what}: alpha of the helper-lane frame differs"
    err, bound = float(np.abs(helped[..., :3] - inst[..., :3]).max()), RGB_TOL * float(np.abs(inst[..., :3]).max())
    print(f"{what}: helper-lane frame max |rgb difference| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: radiance of the helper-lane frame differs: {err:.3e} > {bound:.3e}"
    assert float(inst[..., :3].max()) > 0
    return inst


SCENES = ("notch", "overhang", "hollow", "partial top")


def scene_voxels(kind, base):
    """the cube terrain, lowered by 40 voxels, with two solid walls from the ground up, 104 voxels high, between the camera's view and either
    sun: along y at x cell 3 and along x at y cell 0.  notch: a gap one cell wide in each, level with the view; overhang: a slab that sticks out
    of the x wall's top, and one that floats; hollow: a box mountain in the view, walls and roof one cell thick over a full floor; partial top:
    the walls' top bricks keep their lower half only"""
    g = base.shape[1]
    vox = np.zeros_like(base)
    vox[:-40] = base[40:]
    vox[:104, :, 24:32] = True
    vox[:104, 0:8, :] = True
    if kind == "notch":
        vox[:, 72:80, 24:32] = False
        vox[:, 0:8, 96:104] = False
    elif kind == "overhang":
        vox[96:104, 16:g // 2, 32:64] = True
        vox[96:104, g // 4:g // 2, g // 2:g // 4 * 3] = True
    elif kind == "hollow":
        vox[:, 56:104, 72:112] = False
        vox[:88, 56:104, 72:112] = True
        vox[8:80, 64:96, 80:104] = False
    elif kind == "partial top":
        vox[100:104, :, 24:32] = False
        vox[100:104, 0:8, :] = False
    return vox


@pytest.fixture(scope="module")
def scenes(bm, torch_cuda, terrain):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = bm.Scene.from_voxels(torch_cuda.from_numpy(scene_voxels(kind, terrain["cube"]).astype(np.uint8)).to("cuda:0"))
        return made[kind]
    yield get
    for s in made.values():
        s.close()


def seen_dark_cells(scene, cam, zd):
    """primary hits of the frame's pixel centres whose shadow ray starts in a dark cell: the cell of the voxel in front of the hit face"""
    hits = scene.pixel_hits(cam, W, H)
    voxel, normal, level = hits.voxel.cpu().numpy(), hits.normal.cpu().numpy(), hits.level.cpu().numpy()
    start = (voxel + np.rint(normal).astype(np.int64))[level >= 0]
    g, h = scene.grid_size, scene.grid_height
    start = start[((start >= 0) & (start < np.array([g, g, h]))).all(axis=1)]
    cell = start // 8
    return int(np.count_nonzero(cell[:, 2] < zd[cell[:, 1], cell[:, 0]])), len(start)


@pytest.mark.parametrize("sun,sun_name", [(SUN_X, "x dominant"), (SUN_Y, "y dominant")])
@pytest.mark.parametrize("kind", SCENES)
def test_frames_in_shadow(kind, sun, sun_name, bm, torch_cuda, scenes):
    g, h = WORLDS["cube"]
    scene, cam = scenes(kind), camera_over(bm, g, h)
    check_frames(bm, torch_cuda, scene, cam, sun, f"{kind}, {sun_name}")
    zd = assert_slice(scene, f"{kind}, {sun_name}")
    dark, seen = seen_dark_cells(scene, cam, zd)
    print(f"{kind}, {sun_name}: {dark} of {seen} primary hits start their shadow ray in a dark cell")
    assert dark > seen // 50 and dark > 10, f"{kind}, {sun_name}: the rule ends too few of the view's shadow rays to be tested ({dark} of {seen})"


def test_cone_across_an_octant_boundary(bm, torch_cuda, scenes):
    """no plane for this sun, so no slice is read: the frames use the octant planes, whatever the table holds from the sun before"""
    g, h = WORLDS["cube"]
    scene, cam = scenes("notch"), camera_over(bm, g, h)
    render_once(bm, torch_cuda, scene, cam, SUN_X)
    builds = scene.sun_plane_stats()[0]
    check_frames(bm, torch_cuda, scene, cam, SUN_ACROSS, "cone across an octant boundary")
    assert scene.sun_plane_stats()[0] == builds
    assert (assert_slice(scene, "the table of the sun before") > 0).any()


def test_ring_of_two_suns(bm, torch_cuda, scenes):
    """two frames with different suns as one launch: plane and table are the first frame's, the second keeps its octant planes"""
    torch = torch_cuda
    g, h = WORLDS["cube"]
    scene, cam = scenes("overhang"), camera_over(bm, g, h)
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
