"""Scene.mesh_quads, Quads.triangles and Scene.extract_mesh on the MI355X (csrc/mesh.hip): the device's quads up to the count and its result
record must equal bm_host_mesh_quads -- the host routine that tests/test_mesh_host.py pins to the numpy model -- byte for byte, and the
triangles bm_host_mesh_triangles bit for bit.  Shapes: one voxel, one cell, extents just past a cell, ragged first cells from negative and
odd origins, bases 1 and 3 bytes into an allocation with pitches larger than the extents, more cells than one block of the offset scan, a
capacity that ends inside a cell and inside a wave.  Then the scene level -- terrain, a carved sphere, a streaming scene, adjacent boxes
without a wall between them -- and the loop: the extracted mesh voxelized again gives the volume back.  Every number is an integer, every
comparison exact."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EINVAL = 10001
SCAN_BLOCK = 256   # cells per workgroup of the offset scan (csrc/mesh.h kMeshScanBlock)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def scene(bm, torch_cuda):
    """a small generated scene (terrain), preloaded"""
    s = bm.Scene(128, 128, device=0).generate().preload_all()
    yield s
    s.close()


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_mesh.py took {time.time() - t0:.1f} s")


def random_volume(seed, shape, density):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def check(bm, torch, scene, vol, lo=(0, 0, 0), halo=False, unit=False, what=""):
    """device quads and record of a contiguous upload of `vol` against the host routine"""
    want, rec = bm.host_mesh_quads(vol, lo, halo=halo, unit=unit)
    got = scene.mesh_quads(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), lo, halo=halo, unit=unit)
    assert got.record == rec, f"{what}: {got.record} on the device, {rec} on the host"
    assert got.records.dtype == bm.QUAD_DTYPE and got.records.tobytes() == want.tobytes(), f"{what} {vol.shape} at {lo}: the quads differ"
    return want, rec


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("shape,lo", [((1, 1, 1), (0, 0, 0)), ((8, 8, 8), (0, 0, 0)), ((8, 8, 9), (0, 0, 0)), ((9, 10, 17), (0, 0, 0)), ((9, 10, 17), (3, -5, 6)),
                                      ((9, 12, 17), (-8, -16, 0)), ((20, 13, 31), (-1, 7, -9))])
def test_random_volumes_at_cell_edges_and_ragged_origins(shape, lo, density, bm, torch_cuda, scene):
    vol = random_volume(7, shape, density)
    if shape == (1, 1, 1):
        vol[:] = density < 0.9   # the one voxel solid, and empty
    for unit in (False, True):
        for halo in ((False, True) if min(shape) >= 3 else (False,)):
            check(bm, torch_cuda, scene, vol, lo, halo, unit, f"density {density} halo {halo} unit {unit}")


def test_empty_full_checkerboard_and_other_solid_bytes(bm, torch_cuda, scene):
    _, rec = check(bm, torch_cuda, scene, np.zeros((16, 16, 16), np.uint8), what="empty")
    assert tuple(rec.tolist()) == (0, 0)
    want, rec = check(bm, torch_cuda, scene, np.ones((16, 16, 16), np.uint8), what="full")
    assert len(want) == 24 and (want["shape"] >> 4 == 0x88).all() and rec["faces"] == 6 * 256
    z, y, x = np.indices((16, 16, 16))
    board = ((x + y + z) & 1).astype(np.uint8)
    want, rec = check(bm, torch_cuda, scene, board, what="checkerboard")
    assert len(want) == 8 * 1536 and rec["faces"] == len(want)
    vol = random_volume(1, (11, 12, 13), 0.4) * np.random.default_rng(2).choice(np.array([2, 255, 128, 1], np.uint8), size=(11, 12, 13))
    want, _ = check(bm, torch_cuda, scene, vol, what="bytes 2, 255, 128")
    assert want.tobytes() == bm.host_mesh_quads((vol != 0).astype(np.uint8))[0].tobytes()


@pytest.mark.parametrize("x0", [1, 3, 4, 6])
def test_a_base_inside_an_allocation_and_larger_pitches(x0, bm, torch_cuda, scene):
    """the volume is a slice of a larger tensor that starts 1, 3, 4 and 6 bytes into it: byte and word loads at every phase"""
    torch = torch_cuda
    big = random_volume(x0, (14, 19, 53), 0.45) * 7
    d_big = torch.from_numpy(big).cuda()
    for nx in (8, 17, 33, 53 - x0):
        view = (slice(2, 13), slice(3, 16), slice(x0, x0 + nx))
        for halo in (False, True):
            want, rec = bm.host_mesh_quads(big[view], (5, -3, 2), halo=halo)
            got = scene.mesh_quads(d_big[view], (5, -3, 2), halo=halo)
            assert got.record == rec and got.records.tobytes() == want.tobytes(), (x0, nx, halo)
    assert d_big[view].data_ptr() % 4 == (d_big.data_ptr() + 2 * 19 * 53 + 3 * 53 + x0) % 4


def test_more_cells_than_one_scan_block(bm, torch_cuda, scene):
    """80 x 80 x 40 voxels are 500 cells: two blocks of the offset scan, the second ragged"""
    vol = random_volume(3, (40, 80, 80), 0.3)
    assert 10 * 10 * 5 > SCAN_BLOCK
    want, _ = check(bm, torch_cuda, scene, vol, what="500 cells")
    assert len(want) > 100_000
    check(bm, torch_cuda, scene, vol[:, :, :79], (1, 0, 0), what="550 cells")


def test_capacity_ends_inside_a_cell_and_inside_a_wave(bm, torch_cuda, scene):
    torch = torch_cuda
    vol = random_volume(4, (16, 16, 24), 0.5)
    want, rec = bm.host_mesh_quads(vol)
    d_vol = torch.from_numpy(vol).cuda()
    in_cell0 = (want["x"] < 8) & (want["y"] < 8) & (want["z"] < 8)
    per_cell = int(np.argmin(in_cell0))          # the quads of cell 0 come first
    first_lane = int(np.argmin((want["shape"] & 15 == 0) & (want["x"] == 0) & in_cell0))   # those of its lane 0: direction -x, slice 0
    assert in_cell0[:per_cell].all() and not in_cell0[per_cell:].any() and 3 < first_lane < per_cell - 8 < len(want)
    need = bm.mesh_workspace_bytes(vol.shape)
    from brickmap_amd.host import _mesh_params
    par, ptr, _ = _mesh_params((0, 0, 0), d_vol, False, False)
    for cap in (0, 1, 3, first_lane - 1, first_lane + 1, per_cell - 1, per_cell, per_cell + 5, len(want) - 1, len(want), len(want) + 7):
        buf = torch.full((len(want) + 16, 4), -1, dtype=torch.int32, device="cuda")
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        res = torch.zeros(2, dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        assert scene._L.bm_mesh_quads(scene.gpuScene, C.byref(par), C.c_void_p(ptr), C.c_void_p(buf.data_ptr() if cap else 0), cap, C.c_void_p(res.data_ptr()),
                                      C.c_void_p(ws.data_ptr()), need, C.c_void_p(stream)) == 0
        got = buf.cpu().numpy()
        n = min(cap, len(want))
        assert got[:n].tobytes() == want[:n].tobytes(), cap
        assert (got[n:] == -1).all(), f"capacity {cap}: a record past it was written"
        assert res.cpu().numpy().view(bm.MESH_RESULT_DTYPE)[0] == rec, "the totals are the full ones whatever the capacity"
    q = scene.mesh_quads(d_vol, capacity=per_cell + 5)
    assert q.count == len(want) and len(q) == per_cell + 5 and q.records.tobytes() == want[:per_cell + 5].tobytes()
    assert tuple(q.triangles().shape) == (2 * (per_cell + 5), 3, 3)


def test_halo_tiles_on_the_device_have_no_walls(bm, torch_cuda, scene):
    torch = torch_cuda
    vol = random_volume(5, (32, 32, 32), 0.5)
    d_vol = torch.from_numpy(vol).cuda()
    whole = bm.host_mesh_quads(vol, halo=True)[0]
    tiles = []
    for z in (0, 16):
        for y in (0, 16):
            for x in (0, 16):
                lo = (max(x - 1, 0), max(y - 1, 0), max(z - 1, 0))
                hi = (min(x + 17, 32), min(y + 17, 32), min(z + 17, 32))
                tiles.append(scene.mesh_quads(d_vol[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]], lo, halo=True).records)
    got = np.concatenate(tiles)
    assert len(np.unique(got)) == len(got), "no quad twice"
    assert np.array_equal(np.sort(got, order=["z", "y", "x", "shape"]), np.sort(whole, order=["z", "y", "x", "shape"]))


def test_two_calls_on_two_streams(bm, torch_cuda, scene):
    torch = torch_cuda
    a, b = random_volume(8, (24, 40, 40), 0.5), random_volume(9, (33, 20, 47), 0.2)
    want_a, want_b = bm.host_mesh_quads(a), bm.host_mesh_quads(b, (1, 2, 3))
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):
        outs.append((scene.mesh_quads(da, capacity=len(want_a[0]), stream=s1.cuda_stream), scene.mesh_quads(db, (1, 2, 3), capacity=len(want_b[0]), stream=s2.cuda_stream)))
    torch.cuda.synchronize()
    for qa, qb in outs:
        assert qa.record == want_a[1] and qa.records.tobytes() == want_a[0].tobytes()
        assert qb.record == want_b[1] and qb.records.tobytes() == want_b[0].tobytes()


def test_triangles_equal_the_host_bit_for_bit(bm, torch_cuda, scene):
    torch = torch_cuda
    vol = random_volume(10, (9, 12, 17), 0.5)
    for lo in ((0, 0, 0), (-8000000, 3, 8388608 - 17)):
        q = scene.mesh_quads(torch.from_numpy(vol).cuda(), lo)
        want = bm.host_mesh_triangles(q.records)
        got = q.triangles().cpu().numpy()
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
    # every direction, size and a record with a direction above 5, at an address 4 bytes into an allocation
    recs = np.zeros(6 * 8 * 8 + 2, bm.QUAD_DTYPE)
    d, w, h = np.meshgrid(np.arange(6), np.arange(1, 9), np.arange(1, 9), indexing="ij")
    recs["shape"][:384] = (d | w << 4 | h << 8).reshape(-1)
    recs["x"], recs["y"], recs["z"] = np.arange(len(recs)) - 7, 3 * np.arange(len(recs)), -5
    recs["shape"][384:] = (6 | 1 << 4 | 1 << 8, 15 | 8 << 4 | 8 << 8)
    buf = torch.zeros(len(recs) * 4 + 1, dtype=torch.int32, device="cuda")
    buf[1:] = torch.from_numpy(recs.view(np.int32)).cuda()
    tri = torch.full((len(recs) * 18 + 1,), -1.0, dtype=torch.float32, device="cuda")
    assert scene._L.bm_mesh_triangles(scene.gpuScene, C.c_void_p(buf.data_ptr() + 4), len(recs), C.c_void_p(tri.data_ptr() + 4), None) == 0
    torch.cuda.synchronize()
    got = tri.cpu().numpy()
    assert got[0] == -1.0 and got[1:].tobytes() == bm.host_mesh_triangles(recs).tobytes()
    assert not got[1 + 384 * 18:].any()


def test_refusals_that_need_a_device(bm, torch_cuda, scene):
    torch = torch_cuda
    from brickmap_amd import _lib
    L = scene._L
    vol = torch.ones((8, 8, 8), dtype=torch.uint8, device="cuda")
    need = bm.mesh_workspace_bytes((8, 8, 8))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    res = torch.zeros(2, dtype=torch.int64, device="cuda")
    quads = torch.full((64, 4), -1, dtype=torch.int32, device="cuda")

    def call(extent=(8, 8, 8), lo=(0, 0, 0), row=0, sl=0, flags=0, reserved=0, v=vol.data_ptr(), q=quads.data_ptr(), cap=64, r=res.data_ptr(), w=ws.data_ptr(), wb=need):
        par = _lib.bm_mesh_params()
        par.lo[:] = list(lo)
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.flags, par.reserved = row, sl, flags, reserved
        return L.bm_mesh_quads(scene.gpuScene, C.byref(par), C.c_void_p(v), C.c_void_p(q), cap, C.c_void_p(r), C.c_void_p(w), wb, None)

    def fired(entry, fragment):
        """the refusal that fired: the message names the entry point and holds the fragment of its class"""
        msg = L.bm_last_error_string()
        return msg.startswith(entry + b": ") and fragment in msg

    def refused(kw, fragment):
        assert call(**kw) == EINVAL, kw
        assert fired(b"bm_mesh_quads", fragment), (kw, L.bm_last_error_string())

    extent, null, aligned, overlaps, outside = b"an extent below 1 (below 3 with BM_MESH_HALO) or above 16384", b"null", b"aligned", b"overlaps", b"a box outside +-2^23 voxels"
    bad = [(dict(extent=(0, 8, 8)), extent), (dict(extent=(8, 8, 16385)), extent), (dict(extent=(2, 8, 8), flags=1), extent), (dict(row=7), b"row_pitch below the extent along x"),
           (dict(sl=63), b"slice_pitch below row_pitch * the extent along y"), (dict(flags=4), b"unknown flag"), (dict(reserved=1), b"reserved is not 0"),
           (dict(v=0), null), (dict(r=0), null), (dict(w=0), null), (dict(q=0), null), (dict(q=quads.data_ptr() + 2), aligned), (dict(r=res.data_ptr() + 4), aligned),
           (dict(w=ws.data_ptr() + 8), aligned), (dict(wb=need - 1), b"smaller than"),
           (dict(w=vol.data_ptr(), wb=need), overlaps), (dict(v=ws.data_ptr() + 16), overlaps), (dict(q=ws.data_ptr()), overlaps), (dict(r=ws.data_ptr()), overlaps),
           (dict(lo=((1 << 23) - 7, 0, 0)), outside), (dict(lo=(0, -(1 << 23) - 1, 0)), outside)]
    for kw, fragment in bad:
        refused(kw, fragment)
    # a volume whose pitches carry it 56 MiB past an allocation of 512 bytes (one of its own: torch's tensors share theirs)
    own = C.c_void_p()
    assert L.bm_buffer_alloc(scene.device, 512, C.byref(own)) == 0
    refused(dict(row=1 << 20, sl=8 << 20, v=own.value), b"does not lie inside")
    torch.cuda.synchronize()
    assert (quads == -1).all().item() and not res.any().item() and not ws.any().item()
    assert call(v=own.value, q=0, cap=0) == 0
    assert L.bm_mesh_triangles(scene.gpuScene, C.c_void_p(quads.data_ptr()), 8, own, None) == EINVAL, "8 x 72 bytes do not fit an allocation of 512"
    assert fired(b"bm_mesh_triangles", b"does not lie inside"), L.bm_last_error_string()
    assert L.bm_synchronize(scene.gpuScene) == 0 and L.bm_buffer_free(scene.device, own) == 0
    assert call(q=0, cap=0) == 0 and call() == 0
    torch.cuda.synchronize()
    assert quads.cpu().numpy()[:6].tobytes() == bm.host_mesh_quads(np.ones((8, 8, 8), np.uint8))[0].tobytes() and (quads[6:] == -1).all().item()
    assert L.bm_mesh_triangles(scene.gpuScene, C.c_void_p(quads.data_ptr() + 2), 1, C.c_void_p(ws.data_ptr()), None) == EINVAL
    assert fired(b"bm_mesh_triangles", b"aligned"), L.bm_last_error_string()
    assert L.bm_mesh_triangles(scene.gpuScene, C.c_void_p(quads.data_ptr()), -1, C.c_void_p(ws.data_ptr()), None) == EINVAL
    assert fired(b"bm_mesh_triangles", b"a quad count below 0 or above 2^32"), L.bm_last_error_string()


# ---------------------------------------------------------------- the scene level
def scene_box_check(bm, scene, lo, hi, what=""):
    want, rec = bm.host_mesh_quads(scene.read_region(lo, hi).view(np.uint8), lo)
    got = scene.extract_mesh(lo, hi)
    assert got.record == rec and got.records.tobytes() == want.tobytes(), f"{what} {lo} ... {hi}"
    return want, rec


def surface_box(scene, size=64):
    """a box of size^3 across the terrain surface around the world's centre"""
    g = scene.grid_size
    column = scene.read_region((g // 2, g // 2, 0), (g // 2 + 1, g // 2 + 1, scene.grid_height)).reshape(-1)
    top = int(np.nonzero(column)[0].max()) if column.any() else size // 2
    z0 = max(0, min(scene.grid_height - size, top - size // 2))
    return (g // 2 - size // 2, g // 2 - size // 2, z0), (g // 2 + size // 2, g // 2 + size // 2, z0 + size)


def test_extract_mesh_of_terrain_before_and_after_a_carve(bm, torch_cuda, scene):
    lo, hi = surface_box(scene)
    want, rec = scene_box_check(bm, scene, lo, hi, "terrain")
    assert rec["quads"] > 100 and rec["faces"] > rec["quads"], "terrain merges"
    scene_box_check(bm, scene, (lo[0] + 3, lo[1] - 5, lo[2] + 1), (hi[0] - 6, hi[1] - 20, hi[2] - 9), "offset box")
    centre = ((lo[0] + hi[0]) // 2, (lo[1] + hi[1]) // 2, (lo[2] + hi[2]) // 2)
    before = scene.read_region(lo, hi, device=True)
    try:
        scene.carve_sphere(centre, 11)
        carved, _ = scene_box_check(bm, scene, lo, hi, "carved")
        assert carved.tobytes() != want.tobytes()
    finally:
        scene.write_region(lo, before)
    scene_box_check(bm, scene, lo, hi, "restored")


def test_extract_mesh_of_a_from_voxels_scene_and_past_the_world(bm, torch_cuda):
    vox = np.zeros((128, 128, 128), np.uint8)
    vox[:5] = 1
    vox[5:30, 90:128, 0:50] = random_volume(6, (25, 38, 50), 0.3)
    s = bm.Scene.from_voxels(vox)
    try:
        scene_box_check(bm, s, (0, 64, 0), (64, 128, 64), "a corner of the world")
        want, _ = scene_box_check(bm, s, (-3, 110, -2), (20, 135, 9), "a box that sticks out of the world")
        assert len(want) > 0
    finally:
        s.close()


def test_extract_mesh_of_a_streaming_scene_with_absent_bricks(bm, torch_cuda):
    from _box_cases import WORLDS, streaming_scene
    dims = WORLDS["cube"]
    s = streaming_scene(bm, torch_cuda, "cube")
    try:
        for lo, hi in (((0, 0, 0), (min(dims[0], 96), min(dims[1], 96), min(dims[2], 96))), ((37, 11, 5), (90, 64, 70))):
            assert int(s.query_volumes(bm.volume_box(lo, hi)).unresolved[0]) > 0, "bricks of the box are absent"
            scene_box_check(bm, s, lo, hi, "streaming")
    finally:
        s.close()


def test_open_boxes_share_no_wall(bm, torch_cuda, scene):
    lo, hi = surface_box(scene, 32)
    mid = (lo[0] + hi[0]) // 2
    a = scene.extract_mesh(lo, (mid, hi[1], hi[2]), closed=False).records
    b = scene.extract_mesh((mid, lo[1], lo[2]), hi, closed=False).records
    big = scene.read_region([v - 1 for v in lo], [v + 1 for v in hi]).view(np.uint8)
    for part, box_lo, box_hi in ((a, lo, (mid, hi[1], hi[2])), (b, (mid, lo[1], lo[2]), hi)):
        sub = big[:, :, box_lo[0] - lo[0]:box_hi[0] - lo[0] + 2]
        assert part.tobytes() == bm.host_mesh_quads(sub, [v - 1 for v in box_lo], halo=True)[0].tobytes()
    solid = scene.read_region((mid - 1, lo[1], lo[2]), (mid + 1, hi[1], hi[2]))
    both = solid[:, :, 0] & solid[:, :, 1]
    assert both.any(), "the shared plane crosses the ground"
    for part, d, x in ((a, 1, mid - 1), (b, 0, mid)):
        on_plane = part[(part["shape"] & 15 == d) & (part["x"] == x)]
        for q in on_plane:
            w, h = (q["shape"] >> 4) & 15, (q["shape"] >> 8) & 15
            assert not both[q["z"] - lo[2]:q["z"] - lo[2] + h, q["y"] - lo[1]:q["y"] - lo[1] + w].any(), "a wall between two solid voxels"
    closed = scene.extract_mesh(lo, (mid, hi[1], hi[2])).records

    def wall_faces(q):
        q = q[(q["shape"] & 15 == 1) & (q["x"] == mid - 1)]
        return int((((q["shape"] >> 4) & 15) * ((q["shape"] >> 8) & 15)).sum())
    assert wall_faces(closed) == wall_faces(a) + int(both.sum()), "the closed box has the wall, face for face"


# ---------------------------------------------------------------- the loop: voxels -> mesh -> voxels
def test_the_extracted_mesh_voxelizes_back_to_the_terrain(bm, torch_cuda, scene):
    lo, hi = surface_box(scene, 64)
    want = scene.read_region(lo, hi, device=True)
    assert 0 < int(want.count_nonzero()) < want.numel()
    for unit in (False, True):
        tri = scene.extract_mesh(lo, hi, unit=unit).triangles()
        got, res = scene.voxelize(tri, lo, (64, 64, 64), "solid")
        assert res.open_columns == 0 and res.degenerate == 0 and res.rejected == 0
        assert torch_cuda.equal(got, want)


def test_the_mesh_of_one_component_voxelizes_back_to_its_mask(bm, torch_cuda):
    vox = np.zeros((128, 128, 128), np.uint8)
    vox[:4] = 1
    vox[20:41, 17:40, 9:33] = random_volume(12, (21, 23, 24), 0.62)   # above the percolation threshold: one large piece and crumbs
    s = bm.Scene.from_voxels(vox)
    try:
        lo, hi = (5, 13, 16), (37, 45, 48)
        comps = s.components(lo, hi)
        assert len(comps) > 3
        largest = int(np.argmax(comps.records["voxels"]))
        mask = comps.mask(np.arange(len(comps)) == largest)
        q = s.mesh_quads(mask, lo)
        assert q.record == bm.host_mesh_quads(mask.cpu().numpy(), lo)[1]
        got, res = s.voxelize(q.triangles(), lo, tuple(mask.shape), "solid")
        assert res.open_columns == 0 and torch_cuda.equal(got, mask) and int(got.sum()) == int(comps.records["voxels"][largest])
    finally:
        s.close()


# ---------------------------------------------------------------- the example
def test_headless_main_writes_a_mesh_file(bm, torch_cuda, tmp_path):
    """examples/headless_main --mesh-out x0,y0,z0:x1,y1,z1=FILE: the box's triangles in the raw format --mesh reads (C++ Scene::extract_mesh)"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "headless_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    vox = np.zeros((128, 128, 128), np.uint8)
    vox[40:60, 30:47, 20:51] = random_volume(13, (20, 17, 31), 0.5)
    world = tmp_path / "world.raw"
    vox.tofile(world)
    mesh = tmp_path / "out.tri"
    out = tmp_path / "frame.ppm"
    r = subprocess.run([exe, "--voxels", str(world), "--mesh-out", f"16,28,36:56,52,64={mesh}", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    quads, rec = bm.host_mesh_quads(vox[36:64, 28:52, 16:56], (16, 28, 36))
    m = re.search(r"mesh-out: (\d+) quads, (\d+) faces, (\d+) triangles", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (int(rec["quads"]), int(rec["faces"]), 2 * len(quads)), r.stdout
    assert np.fromfile(mesh, np.float32).tobytes() == bm.host_mesh_triangles(quads).tobytes()
    r = subprocess.run([exe, "--voxels", str(world), "--mesh-out", "1,2,3", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--mesh-out wants" in r.stderr
