"""The view plane on the MI355X (csrc/viewfield.h, viewfield.hip; the rule's CPU replay is tests/test_view_rule.py).

6.1  The plane the device holds (bm_scene_view_plane) equals the rule -- tests/view_check.cpp in its `plane` mode, the header's own
     functions on the device's own index words -- after generate, after load_voxels, after an edit that puts a brick where the plane
     said "nothing can be hit from here on", after that edit's undoing and after a region write; in a cube, a flat and a tall world.
6.2  Frames of the production instantiations -- whose primary rays walk the plane -- against the instrumented one's, which never reads
     it: ordered frames bit for bit, helper-lane frames (what bench.py times) with alpha exact and radiance within the parity tolerance
     of test_gpu_escape.  Cameras above the terrain, one cell above it at a grazing angle, under an overhang, in the row, column and
     layer of occupied cells (the flat world, with a floating slab); turned in place (no rebuild), moved (no plane until it has rested), outside the world and with a lens
     (no plane); a uniform launch of three frames into one buffer, a ring of two origins, 4 spp as sample items, a streaming scene.
6.3  The build counter stands still across launches from one position and moves once after one edit batch.
Every case that expects the plane asserts through the stats that it was built, and from the instrumented first-hit records that the
cells between the camera and what the primary rays hit include cells whose view byte exceeds their octant's.
Frames are 64 x 64, 1 spp, 4 segments; worlds of 128^3 to 256 x 256 x 128 voxels."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_escape import RGB_TOL, camera, device_occupancy, tops_of
from test_gpu_sunfield import WORLDS

pytestmark = pytest.mark.gpu

W = H = 64
MB = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    """occupancy [z, y, x] over brick cells, origin (voxels), lens radius -> the rule's plane uint8 [z, y, x], or None where the rule gives no plan"""
    d = tmp_path_factory.mktemp("view_rule")
    exe = d / "view_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), os.path.join(ROOT, "tests", "view_check.cpp")])

    def plane(occ, origin, lens=0.0):
        nz, ny, nx = occ.shape
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([nx, ny, nz], np.int32).tobytes() + np.array(list(origin) + [lens], np.float32).tobytes() + occ.astype(np.uint8).tobytes())
        subprocess.check_call([str(exe), "plane", str(d / "in.bin"), str(d / "out.bin")])
        out = np.fromfile(d / "out.bin", np.uint8)
        return out.reshape(occ.shape) if out.size else None
    return plane


# ---------------------------------------------------------------- helpers
def params(bm, flags=0, sample_base=0, spp=1):
    return bm.FrameParams(W, H, spp=spp, sample_base=sample_base, max_bounces=MB, flags=flags)


def zeros(torch, *shape, dtype=None):
    return torch.zeros(shape, dtype=dtype or torch.float32, device="cuda:0")


def rest(bm, torch, scene, cam, launches=2):
    """production launches of one frame from `cam`: after the second the camera has rested"""
    acc = zeros(torch, H, W, 4)
    for _ in range(launches):
        scene.render(cam, params(bm), acc)
    torch.cuda.synchronize()


def assert_plane(scene, rule, cam, what):
    plane, origin = scene.view_plane()
    assert plane is not None, f"{what}: no view plane stands"
    assert np.array_equal(origin, np.array(cam.position, np.float32)), f"{what}: the plane was built for {origin}"
    assert (plane[0] == 255).all() and (plane[-1] == 255).all() and (plane[:, 0] == 255).all() and (plane[:, :, -1] == 255).all(), f"{what}: border"
    got, want = plane[1:-1, 1:-1, 1:-1], rule(device_occupancy(scene), cam.position)
    assert want is not None and np.array_equal(got, want), f"{what}: {np.count_nonzero(got != want)} of {want.size} bytes differ from the rule"
    return got


def longer_cells_on_primary_rays(scene, cam, dbg):
    """cells between the camera and the first hits of the instrumented frame `dbg` whose view byte (1 ... 254) exceeds the byte of their octant's plane"""
    plane = scene.view_plane()[0][1:-1, 1:-1, 1:-1]
    field = scene.device_cube_field()[:, 1:-1, 1:-1, 1:-1]
    nz, ny, nx = plane.shape
    hit = dbg[..., 1] != 0
    ids = dbg[..., 2][hit].astype(np.int64)
    centres = np.stack([ids % nx, ids // nx % ny, ids // (nx * ny)], -1) + 0.5
    p = np.array(cam.position, np.float32) / np.float32(8)
    t = np.linspace(0.0, 1.0, 64).reshape(-1, 1, 1)
    cells = np.unique(np.floor(p + t * (centres - p)).astype(np.int64).reshape(-1, 3), axis=0)
    cp = np.floor(p).astype(np.int64)
    cells = cells[(cells != cp).all(-1) & (cells >= 0).all(-1) & (cells < (nx, ny, nz)).all(-1)]
    octant = ((cells < cp) * (1, 2, 4)).sum(-1)
    v, o = plane[cells[:, 2], cells[:, 1], cells[:, 0]], field[octant, cells[:, 2], cells[:, 1], cells[:, 0]]
    return int(np.count_nonzero((v > o) & (v != 255)))


def frames(bm, torch, scene, cam):
    """the frame four ways: instrumented (ordered, with hit records), production ordered, production with helper lanes, and the hit records"""
    inst, dbg, prod, helped = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32), zeros(torch, H, W, 4), zeros(torch, H, W, 4)
    scene.render(cam, params(bm, bm.BM_FLAG_ORDERED), inst, debug=dbg)
    scene.render(cam, params(bm, bm.BM_FLAG_ORDERED), prod)
    scene.render(cam, params(bm), helped)
    torch.cuda.synchronize()
    return inst.cpu().numpy(), prod.cpu().numpy(), helped.cpu().numpy(), dbg.cpu().numpy().view(np.uint32)


def check_frames(bm, torch, scene, cam, what, plane=True, min_hits=W * H // 8):
    """rest the camera, then the three frames; plane: the production frames must have had the view plane of this camera"""
    rest(bm, torch, scene, cam)
    builds = scene.view_plane_stats()[0]
    inst, prod, helped, dbg = frames(bm, torch, scene, cam)
    assert scene.view_plane_stats()[0] == builds, f"{what}: a camera at rest rebuilt its plane"
    assert np.array_equal(prod.view(np.uint32), inst.view(np.uint32)), f"{what}: {np.count_nonzero((prod != inst).any(-1))} pixels of the ordered production frame differ from the instrumented one"
    assert np.array_equal(helped[..., 3], inst[..., 3]), f"{what}: alpha of the helper-lane frame differs"
    err, bound = float(np.abs(helped[..., :3] - inst[..., :3]).max()), RGB_TOL * float(np.abs(inst[..., :3]).max())
    print(f"{what}: helper-lane frame max |rgb difference| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: radiance of the helper-lane frame differs: {err:.3e} > {bound:.3e}"
    assert (dbg[..., 1] != 0).sum() >= min_hits, f"{what}: the view shows too little terrain for its primary rays to mean anything"
    if plane:
        got, origin = scene.view_plane()
        assert got is not None and np.array_equal(origin, np.array(cam.position, np.float32)), f"{what}: the frames had no view plane of this camera"
        longer = longer_cells_on_primary_rays(scene, cam, dbg)
        print(f"{what}: {longer} cells on the primary rays' way with a view byte above their octant's")
        assert longer > 0, f"{what}: no cell on the primary rays' way has a view byte above its octant's"
    return inst, dbg


def camera_over(bm, g, h):
    return bm.Camera(position=(g / 2, g / 8, 0.8 * h), horizontal_angle=0.8, vertical_angle=-0.5).update()


# ---------------------------------------------------------------- 6.1 the plane
@pytest.mark.parametrize("world", list(WORLDS))
def test_plane_equals_the_rule(world, bm, torch_cuda, terrain, rule):
    torch = torch_cuda
    g, h = WORLDS[world]
    cam = camera_over(bm, g, h)
    s = bm.Scene(g, h, device=0).generate().preload_all()
    assert s.view_plane()[0] is None and s.view_plane_stats()[0] == 0
    rest(bm, torch, s, cam, launches=1)
    assert s.view_plane()[0] is None and s.view_plane_stats()[0] == 0, "one frame from a position: the camera has not rested"
    rest(bm, torch, s, cam, launches=1)
    first = assert_plane(s, rule, cam, "generate")
    assert (first == 255).any() and ((first >= 4) & (first < 255)).any() and (first == 0).any() and s.view_plane_stats() [0] == 1
    field = s.device_cube_field()[:, 1:-1, 1:-1, 1:-1]
    assert ((first != 255) & (first > field.max(axis=0))).any(), "no byte is longer than every octant's"
    s.close()
    s = bm.Scene.from_voxels(torch.from_numpy(terrain[world].astype(np.uint8)).to("cuda:0"))
    rest(bm, torch, s, cam)
    assert np.array_equal(assert_plane(s, rule, cam, "load_voxels"), first)
    # a brick in a cell that read 255, away from the world's edge: the lowest such cell, near the middle
    zs, ys, xs = np.nonzero(first[:, 2:-2, 2:-2] == 255)
    k = int(np.argmin(zs * 4096 + np.abs(ys - len(first[0]) // 2) + np.abs(xs - len(first[0]) // 2)))
    cz, cy, cx = int(zs[k]), int(ys[k]) + 2, int(xs[k]) + 2
    s.fill_box((cx * 8, cy * 8, cz * 8), (cx * 8 + 8, cy * 8 + 8, cz * 8 + 8))
    assert s.view_plane()[0] is None, "the plane is stale after an edit"
    rest(bm, torch, s, cam, launches=1)
    edited = assert_plane(s, rule, cam, "edit")
    assert edited[cz, cy, cx] == 0 and ((first == 255) & (edited != 255) & (edited != 0)).any(), "the brick ends the escape of cells that were clear"
    s.clear_box((cx * 8, cy * 8, cz * 8), (cx * 8 + 8, cy * 8 + 8, cz * 8 + 8))
    rest(bm, torch, s, cam, launches=1)
    assert np.array_equal(assert_plane(s, rule, cam, "edit undone"), first)
    slab = np.ones((8, 40, 48), np.uint8)
    s.write_region((g // 2 - 20, g // 2 - 30, h - 24), slab)
    rest(bm, torch, s, cam, launches=1)
    assert not np.array_equal(assert_plane(s, rule, cam, "region write"), first)
    s.close()


# ---------------------------------------------------------------- 6.2 frames
FRAMES_WORLD = "flat"  # 32 x 32 x 16 cells: in the 16^3 cells of the cube a pencil has hardly room to be longer than a cube


@pytest.fixture(scope="module")
def overhang(bm, torch_cuda, terrain):
    """the flat terrain with a slab floating over a part of the world: (scene, voxels)"""
    g, h = WORLDS[FRAMES_WORLD]
    vox = terrain[FRAMES_WORLD].copy()
    vox[h - 24:h - 16, g // 8:g // 2, g // 4:g // 4 * 3] = True
    scene = bm.Scene.from_voxels(torch_cuda.from_numpy(vox.astype(np.uint8)).to("cuda:0"))
    yield scene, vox
    scene.close()


def cells_of(vox):
    """bool [z, y, x] over brick cells: the cell holds a voxel"""
    return vox.reshape(vox.shape[0] // 8, 8, vox.shape[1] // 8, 8, vox.shape[2] // 8, 8).any(axis=(1, 3, 5))


def ground_cameras(bm, vox):
    """name -> camera, placed by the terrain's own heights"""
    g, h = WORLDS[FRAMES_WORLD]
    tops = tops_of(vox[:h - 24])  # the terrain under the slab, per voxel column
    out = {}
    out["above the terrain"] = camera(bm, (6.5, 5.5, h - 7.0), (1.0, 1.0, -0.4))  # high in a corner, across the world
    x, y = 12, g - 12
    top_cell = int(tops[y - 4:y + 4, x - 4:x + 4].max()) // 8
    out["one cell above the terrain, grazing"] = camera(bm, (x + 0.5, y + 0.5, (top_cell + 1) * 8 + 4.5), (1.0, -0.8, 0.02))
    out["under the overhang"] = camera(bm, (g // 4 + 6.5, g // 8 + 8.5, h - 29.5), (0.6, 1.0, -0.3))
    # in the cell row, column and layer of occupied cells: an empty cell with all three, in a low corner of the tenth layer, looking along the layer at the hills
    cells = cells_of(vox)
    zs, ys, xs = np.nonzero(~cells & cells.any(axis=2, keepdims=True) & cells.any(axis=1, keepdims=True) & cells.any(axis=0, keepdims=True))
    k = int(np.argmin(np.abs(zs - 9) * 64 + np.abs(ys - 26) + np.abs(xs - 4)))
    out["in the layer of occupied cells"] = camera(bm, (int(xs[k]) * 8 + 4.5, int(ys[k]) * 8 + 4.5, int(zs[k]) * 8 + 4.5), (1.0, -1.0, 0.0))
    return out


@pytest.mark.parametrize("name", ["above the terrain", "one cell above the terrain, grazing", "under the overhang", "in the layer of occupied cells"])
def test_frames(name, bm, torch_cuda, overhang, rule):
    scene, vox = overhang
    cam = ground_cameras(bm, vox)[name]
    if name == "in the layer of occupied cells":
        cx, cy, cz = (int(v) // 8 for v in cam.position)
        cells = cells_of(vox)
        assert cells[cz, cy].any() and cells[cz, :, cx].any() and cells[:, cy, cx].any() and not cells[cz, cy, cx], "the camera's row, column and layer hold occupied cells"
    builds = scene.view_plane_stats()[0]
    check_frames(bm, torch_cuda, scene, cam, name)
    assert scene.view_plane_stats()[0] == builds + 1, "a new position: one build"
    assert_plane(scene, rule, cam, name)


def test_turned_and_moved(bm, torch_cuda, overhang):
    torch = torch_cuda
    scene, vox = overhang
    cam = ground_cameras(bm, vox)["above the terrain"]
    check_frames(bm, torch, scene, cam, "before the turn")
    builds = scene.view_plane_stats()[0]
    turned = camera(bm, cam.position, (1.0, 0.6, -0.6))
    check_frames(bm, torch, scene, turned, "turned in place")
    assert scene.view_plane_stats()[0] == builds, "the plane depends on the position alone"
    moved = camera(bm, (cam.position[0] + 9.0, cam.position[1] + 3.0, cam.position[2] - 2.0), (1.0, 1.0, -0.4))
    inst, dbg, prod = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32), zeros(torch, H, W, 4)
    scene.render(moved, params(bm, bm.BM_FLAG_ORDERED), inst, debug=dbg)
    scene.render(moved, params(bm, bm.BM_FLAG_ORDERED), prod)
    torch.cuda.synchronize()
    assert scene.view_plane_stats()[0] == builds, "the first launch from a new position builds nothing"
    assert np.array_equal(scene.view_plane()[1], np.array(cam.position, np.float32)), "the old position's plane stays, unused"
    assert np.array_equal(prod.cpu().numpy().view(np.uint32), inst.cpu().numpy().view(np.uint32)), "moved, not rested"
    check_frames(bm, torch, scene, moved, "moved and rested")
    assert scene.view_plane_stats()[0] == builds + 1


def test_no_plane_outside_the_world_and_with_a_lens(bm, torch_cuda, overhang):
    scene, vox = overhang
    g, h = WORLDS[FRAMES_WORLD]
    builds = scene.view_plane_stats()[0]
    outside = camera(bm, (g / 2, -20.0, h + 10.0), (0.0, 1.0, -0.6))
    check_frames(bm, torch_cuda, scene, outside, "outside the world", plane=False)
    lens = camera_over(bm, g, h)
    lens.lensRadius, lens.focalDistance = 0.5, 30.0
    check_frames(bm, torch_cuda, scene, lens, "with a lens", plane=False)
    assert scene.view_plane_stats()[0] == builds, "neither camera gets a plane"


def test_uniform_launch_ring_of_two_origins_and_sample_items(bm, torch_cuda, overhang):
    torch = torch_cuda
    scene, vox = overhang
    g, h = WORLDS[FRAMES_WORLD]
    cam = ground_cameras(bm, vox)["one cell above the terrain, grazing"]
    other = camera_over(bm, g, h)
    rest(bm, torch, scene, other)  # the plane is another position's when the launches below begin
    # ---- three frames into one buffer against three instrumented launches: the launch itself holds the camera at rest
    builds = scene.view_plane_stats()[0]
    ref, dbg = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32)
    for k in range(3):
        scene.render(cam, params(bm, bm.BM_FLAG_ORDERED, sample_base=k), ref, debug=dbg)
    got = zeros(torch, H, W, 4)
    scene.render_frames(cam, [params(bm, sample_base=k) for k in range(3)], got)
    torch.cuda.synchronize()
    assert scene.view_plane_stats()[0] == builds + 1 and np.array_equal(scene.view_plane()[1], np.array(cam.position, np.float32)), "three frames from one origin: built by that launch"
    a, b = got.cpu().numpy(), ref.cpu().numpy()
    assert np.array_equal(a[..., 3], b[..., 3]) and b[..., 3].min() >= 3
    assert float(np.abs(a[..., :3] - b[..., :3]).max()) <= RGB_TOL * float(np.abs(b[..., :3]).max())
    assert longer_cells_on_primary_rays(scene, cam, dbg.cpu().numpy().view(np.uint32)) > 0
    # ---- a ring of two frames with different origins: the plane is the first frame's, the second keeps its octant planes
    for flags in (bm.BM_FLAG_ORDERED, 0):
        want = []
        for k, c in enumerate((cam, other)):
            inst, d = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32)
            scene.render(c, params(bm, bm.BM_FLAG_ORDERED, sample_base=k), inst, debug=d)
            want.append(inst)
        out = [zeros(torch, H, W, 4) for _ in range(2)]
        scene.render_frames([cam, other], [params(bm, flags, sample_base=k) for k in range(2)], out)
        torch.cuda.synchronize()
        assert np.array_equal(scene.view_plane()[1], np.array(cam.position, np.float32)) and scene.view_plane_stats()[0] == builds + 1
        for k in range(2):
            a, b = out[k].cpu().numpy(), want[k].cpu().numpy()
            assert np.array_equal(a[..., 3], b[..., 3])
            if flags:
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"ordered ring, frame {k}"
            else:
                assert float(np.abs(a[..., :3] - b[..., :3]).max()) <= RGB_TOL * float(np.abs(b[..., :3]).max()), f"helper-lane ring, frame {k}"
    # ---- 4 spp as sample items
    ref = zeros(torch, H, W, 4)
    scene.render(cam, params(bm, bm.BM_FLAG_ORDERED, spp=4), ref, debug=zeros(torch, H, W, 8, dtype=torch.int32))
    got = zeros(torch, H, W, 4)
    scene.render(cam, params(bm, bm.BM_FLAG_SAMPLE_ITEMS, spp=4), got)
    torch.cuda.synchronize()
    a, b = got.cpu().numpy(), ref.cpu().numpy()
    assert np.array_equal(a[..., 3], b[..., 3]) and float(np.abs(a[..., :3] - b[..., :3]).max()) <= RGB_TOL * float(np.abs(b[..., :3]).max())
    assert scene.view_plane_stats()[0] == builds + 1


def test_streaming_scene(bm, torch_cuda):
    """from empty residency: two production frames of one launch (the plane is built by it) against two instrumented ones on a second scene --
    equal frames, equal index words (the requested bits) and equal brick requests"""
    torch = torch_cuda
    g, h = WORLDS["cube"]
    cam = camera_over(bm, g, h)
    scenes = []
    for _ in range(2):
        s = bm.Scene(g, h, device=0)
        s.set_queue_capacity(1 << 16)
        scenes.append(s.generate())
    prod, inst = scenes
    ps = [params(bm, bm.BM_FLAG_ORDERED, sample_base=k) for k in range(2)]
    for round_ in range(2):  # from nothing resident, then with what the first round requested
        a = [zeros(torch, H, W, 4) for _ in range(2)]
        b = [zeros(torch, H, W, 4) for _ in range(2)]
        prod.render_frames(cam, ps, a)
        inst.render_frames(cam, ps, b, debugs=[zeros(torch, H, W, 8, dtype=torch.int32) for _ in range(2)])
        torch.cuda.synchronize()
        assert prod.view_plane_stats()[0] == 1 and inst.view_plane_stats()[0] == 0, "the production launch built the plane; instrumented frames never do"
        for k in range(2):
            assert np.array_equal(a[k].cpu().numpy().view(np.uint32), b[k].cpu().numpy().view(np.uint32)), f"round {round_}, frame {k}"
        for sc in range(prod.info()["supercells"]):
            # (all but the brick's slot in its pool, which is dealt in the order the requests were filed in: loaded, unloaded, requested, LoD)
            assert np.array_equal(prod.device_indices(sc) & 0xFFFFF000, inst.device_indices(sc) & 0xFFFFF000), f"round {round_}: index words of supercell {sc} differ"
        n = prod.process_load_queue()
        assert n == inst.process_load_queue() and (n > 0 or round_ > 0)
    for s in scenes:
        s.close()


# ---------------------------------------------------------------- 6.3 the build counter
def test_build_counter(bm, torch_cuda, terrain):
    torch = torch_cuda
    g, h = WORLDS["cube"]
    scene = bm.Scene.from_voxels(torch.from_numpy(terrain["cube"].astype(np.uint8)).to("cuda:0"))
    cam = camera_over(bm, g, h)
    info = scene.info()
    rest(bm, torch, scene, cam, launches=4)
    builds, ms = scene.view_plane_stats()
    assert builds == 1 and ms > 0
    assert scene.info()["cube_field_bytes"] == info["cube_field_bytes"] and scene.info()["sun_plane_bytes"] >= info["cube_field_bytes"] // 8
    scene.edit([bm.edit_box(bm.BM_EDIT_SET, (8, 8, h - 16), (16, 16, h - 8)), bm.edit_box(bm.BM_EDIT_SET, (40, 40, h - 16), (48, 48, h - 8))])
    assert scene.view_plane_stats()[0] == 1, "an edit alone builds nothing"
    rest(bm, torch, scene, cam, launches=2)
    assert scene.view_plane_stats()[0] == 2, "one edit batch: one rebuild, by the next launch"
    scene.close()
