"""brickmap_amd.water on the MI355X (csrc/water.hip): the device's field, its result record and its mask must equal bm_host_water_field and
bm_host_water_mask -- the host routines that tests/test_water_host.py pins to the numpy model -- byte for byte.  The cases of the host test
again, then the shapes at which the tiling can go wrong: a lone tile, ragged tiles, a column, a bowl, a U-tube and corridors across tile
faces, a level that arrives late.  Then the scene level: pools() on a box across the terrain surface against the model.  Every number is
an integer, every comparison exact."""
import ctypes as C
import time

import numpy as np
import pytest

import _water_cases as cases
import _water_model as model

pytestmark = pytest.mark.gpu
EINVAL = 10001
NONE = model.NONE


@pytest.fixture(scope="module")
def water():
    from brickmap_amd import water
    return water


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def scene(bm, torch_cuda):
    """the smallest generated scene (terrain), preloaded"""
    s = bm.Scene(128, 128, device=0).generate().preload_all()
    yield s
    s.close()


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_water.py took {time.time() - t0:.1f} s")


def check(water, torch, scene, vol, drains=None, open=cases.SIDES, sea=0, what=""):
    """device field, record and masks of a contiguous upload of `vol` against the host routines"""
    want, rec = water.host_water_field(vol, drains, open, sea)
    got = water.water_field(scene, torch.from_numpy(np.ascontiguousarray(vol)).cuda(), drains, open, sea)
    field = got.field.cpu().numpy()
    assert field.dtype == np.int32 and field.shape == vol.shape
    assert field.tobytes() == want.tobytes(), f"{what} {vol.shape}: first difference at {np.argmax(field.ravel() != want.ravel())}"
    assert got.record == rec, f"{what} {vol.shape}: {got.record} on the device, {rec} on the host"
    for depth in (1, 2):
        mask = got.mask(depth)
        assert mask.dtype == torch.uint8 and mask.cpu().numpy().tobytes() == water.host_water_mask(want, depth).tobytes(), (what, depth)
    return want, rec


# ---------------------------------------------------------------- the cases of the host test
@pytest.mark.parametrize("case", cases.CASES + cases.RANDOM, ids=[c[0] for c in cases.CASES + cases.RANDOM])
def test_device_equals_the_host_routine(case, water, torch_cuda, scene):
    check(water, torch_cuda, scene, *case[1:], what=case[0])


def test_a_strided_slice_of_a_larger_tensor(water, torch_cuda, scene):
    big = cases.random_volume(5, 0.55, (12, 14, 40)) * 7
    view = (slice(1, 11), slice(2, 13), slice(3, 36))
    d_big = torch_cuda.from_numpy(big).cuda()
    want, rec = water.host_water_field(big[view], [(4, 4, 4)], cases.SIDES, 2)
    got = water.water_field(scene, d_big[view], [(4, 4, 4)], cases.SIDES, 2)
    assert not d_big[view].is_contiguous() and got.record == rec and got.field.cpu().numpy().tobytes() == want.tobytes()


# ---------------------------------------------------------------- where the tiling can go wrong
@pytest.mark.parametrize("shape", [(8, 8, 8), (9, 9, 9), (23, 5, 17), (40, 1, 1)], ids=["one tile", "ragged, eight tiles", "17x5x23", "a column"])
def test_a_lone_tile_ragged_tiles_and_a_column(shape, water, torch_cuda, scene):
    """shapes are (nz, ny, nx)"""
    for density in (0, 0.3, 0.55, 1):
        vol = cases.random_volume(sum(shape), density, shape) * 255
        for open, sea in ((cases.SIDES, 0), (("-z",), 0), (("+z",), shape[0] // 2), ((), 0)):
            z, y, x = np.argwhere(vol == 0)[0] if (vol == 0).any() else (0, 0, 0)
            check(water, torch_cuda, scene, vol, [(x, y, z), (-1, 0, 0)], open, sea, what=f"density {density} open {open}")


def test_a_bowl_whose_rim_crosses_a_tile_face_on_every_axis(water, torch_cuda, scene):
    vol = cases.bowl((20, 20, 20), top=12, lo=5, a=4, b=13)
    want, rec = check(water, torch_cuda, scene, vol, what="bowl")
    assert (want[5:12, 4:13, 4:13] == 12).all() and int(rec["wet"]) == 7 * 81 and int(rec["deepest"]) == 7
    want, rec = check(water, torch_cuda, scene, vol, [(4, 12, 5)], what="drained bowl")
    assert int(rec["wet"]) == 0


def test_a_u_tube_whose_arms_lie_in_different_tiles(water, torch_cuda, scene):
    vol = cases.u_tube(nx=24, left=2, right=18)
    want, rec = check(water, torch_cuda, scene, vol, what="u-tube")
    assert (want[1:10, 2, 2] == 10).all() and (want[1:10, 2, 18] == 10).all() and (want[10:13, 2, 18] == [10, 11, 12]).all()


def test_a_serpentine_takes_more_rounds_than_tiles_lie_between(water, torch_cuda, scene):
    """24 x 16 x 3 voxels are 3 x 2 x 1 tiles, no tile more than three faces from the entrance.  The corridor crosses a tile face 15 times:
    everything is final after round 16, and round 17 at the latest lists nothing.  The middle tile of the upper half is crossed by four
    rows and that of the lower half by three, one after the other, and a tile is visited once per round: at least 7 rounds and a last."""
    vol = cases.serpentine()
    want, rec = check(water, torch_cuda, scene, vol, None, ("-x",), what="serpentine")
    assert int(rec["closed"]) == 0 and int(rec["wet"]) == 0 and want[1, 13, 1] == 1
    got, (ms, rounds, looks, visits) = water.water_field_times(scene, torch_cuda.from_numpy(vol).cuda(), None, ("-x",), batch=1)
    assert got.field.cpu().numpy().tobytes() == want.tobytes()
    assert 8 <= rounds <= 17 and looks == rounds + 1 and visits >= rounds, (rounds, looks, visits)


def test_a_level_that_arrives_late_by_a_detour(water, torch_cuda, scene):
    """the shaft's tile hears of the high corridor after five rounds and of the low zigzag, which crosses a tile face every other step,
    later -- in each of five pairs of tiles the zigzag changes sides three times, at most once per round and tile: ten rounds or more --:
    its values fall twice, and the last word is the flood's"""
    vol = cases.late_detour()
    want, rec = check(water, torch_cuda, scene, vol, None, ("-x",), what="detour")
    assert (want[1:11, 3, 38] == np.arange(1, 11)).all() and int(rec["wet"]) == 0
    d_vol = torch_cuda.from_numpy(vol).cuda()
    early = water.water_field_times(scene, d_vol, None, ("-x",), batch=1)
    rounds = early[1][1]
    assert rounds >= 10, rounds
    # without the low way the shaft stands full: the value the shaft's tile held first
    high = vol.copy()
    high[1, 7:9, 0] = 1
    want, rec = check(water, torch_cuda, scene, high, None, ("-x",), what="the high way alone")
    assert (want[1:11, 3, 38] == 10).all() and int(rec["wet"]) > 9


# ---------------------------------------------------------------- calls
def test_two_runs_out_and_a_callers_stream(water, torch_cuda, scene):
    torch = torch_cuda
    vol = cases.random_volume(3, 0.6, (33, 40, 50))
    want, rec = water.host_water_field(vol, [(1, 1, 1)], cases.SIDES, 5)
    d_vol = torch.from_numpy(vol).cuda()
    a = water.water_field(scene, d_vol, [(1, 1, 1)], sea_level=5)
    out = torch.empty(vol.shape, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    b = water.water_field(scene, d_vol, [(1, 1, 1)], sea_level=5, out=out, stream=s.cuda_stream)
    assert b.field is out and a.field.data_ptr() != out.data_ptr()
    assert a.field.cpu().numpy().tobytes() == out.cpu().numpy().tobytes() == want.tobytes() and a.record == b.record == rec
    assert a.wet == int(rec["wet"]) > 0 and a.closed == int(rec["closed"]) > 0
    (x, y, z), depth = a.deepest()
    assert depth == int(rec["deepest"]) and want[z, y, x] - z == depth and (z * 40 + y) * 50 + x == int(rec["deepest_at"])
    mask = torch.full(vol.shape, 9, dtype=torch.uint8, device="cuda")
    assert b.mask(2, out=mask, stream=s.cuda_stream) is mask
    s.synchronize()
    assert mask.cpu().numpy().tobytes() == water.host_water_mask(want, 2).tobytes()
    with pytest.raises(ValueError):
        a.mask(0)
    with pytest.raises(ValueError):
        a.mask(1, out=torch.empty(vol.shape, dtype=torch.int32, device="cuda"))


def test_refusals_that_need_a_device(water, torch_cuda, scene):
    torch = torch_cuda
    from brickmap_amd import _lib
    L = scene._L
    vol = torch.zeros((8, 8, 8), dtype=torch.uint8, device="cuda")
    need = water.water_workspace_bytes((8, 8, 8))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    field = torch.full((8, 8, 8), -1, dtype=torch.int32, device="cuda")
    drains = torch.zeros((2, 3), dtype=torch.int32, device="cuda")

    def call(extent=(8, 8, 8), row=0, sl=0, flags=15, reserved=0, sea=0, v=vol.data_ptr(), s=drains.data_ptr(), n=2, f=field.data_ptr(), r=res.data_ptr(), w=ws.data_ptr(), wb=need):
        par = _lib.bm_water_params()
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.flags, par.reserved, par.sea_level = row, sl, flags, reserved, sea
        return L.bm_water_field(scene.gpuScene, C.byref(par), C.c_void_p(v), C.c_void_p(s), n, C.c_void_p(f), C.c_void_p(r), C.c_void_p(w), wb, None)

    def fired(entry, fragment):
        msg = L.bm_last_error_string()
        return msg.startswith(entry + b": ") and fragment in msg

    extent, null, aligned, overlaps = b"an extent below 1 or above 16384", b"null", b"aligned", b"overlaps"
    bad = [(dict(extent=(0, 8, 8)), extent), (dict(extent=(8, 8, 16385)), extent), (dict(extent=(16384, 16384, 8)), b"more than 2^31 - 2 voxels"),
           (dict(row=7), b"row_pitch below the extent along x"), (dict(sl=63), b"slice_pitch below row_pitch * the extent along y"), (dict(flags=64), b"unknown flag"),
           (dict(reserved=1), b"reserved is not 0"), (dict(sea=9), b"sea_level above the extent along z"), (dict(n=-1), b"a negative number of drains"), (dict(v=0), null),
           (dict(s=0), null), (dict(f=0), null), (dict(r=0), null), (dict(w=0), null), (dict(f=field.data_ptr() + 2), aligned), (dict(s=drains.data_ptr() + 2), aligned),
           (dict(r=res.data_ptr() + 4), aligned), (dict(w=ws.data_ptr() + 8), aligned), (dict(wb=need - 1), b"smaller than"), (dict(w=vol.data_ptr(), wb=need), overlaps),
           (dict(v=ws.data_ptr() + 16), overlaps), (dict(f=ws.data_ptr()), overlaps), (dict(s=ws.data_ptr() + need - 16), overlaps), (dict(r=ws.data_ptr() + need - 32), overlaps),
           (dict(f=vol.data_ptr()), overlaps), (dict(s=field.data_ptr() + 64), overlaps)]
    for kw, fragment in bad:
        assert call(**kw) == EINVAL, kw
        assert fired(b"bm_water_field", fragment), (kw, L.bm_last_error_string())
    own = C.c_void_p()
    assert L.bm_buffer_alloc(scene.device, 512, C.byref(own)) == 0
    for kw in (dict(row=1 << 20, sl=8 << 20, v=own.value), dict(f=own.value), dict(s=own.value + 500)):
        assert call(**kw) == EINVAL and fired(b"bm_water_field", b"does not lie inside"), (kw, L.bm_last_error_string())
    torch.cuda.synchronize()
    assert (field == -1).all().item() and not res.any().item() and not ws.any().item(), "nothing is launched and nothing written: the field is untouched"

    mask = torch.full((8, 8, 8), 9, dtype=torch.uint8, device="cuda")

    def mask_call(extent=(8, 8, 8), f=field.data_ptr(), depth=1, m=mask.data_ptr()):
        return L.bm_water_mask(scene.gpuScene, (C.c_int32 * 3)(*extent) if extent else None, C.c_void_p(f), depth, C.c_void_p(m), None)

    for kw, fragment in ((dict(extent=None), null), (dict(extent=(0, 8, 8)), extent), (dict(extent=(16384, 16384, 8)), b"more than 2^31 - 2 voxels"), (dict(f=0), null),
                         (dict(m=0), null), (dict(depth=0), b"a min_depth below 1"), (dict(f=field.data_ptr() + 2), aligned), (dict(m=field.data_ptr()), overlaps),
                         (dict(m=field.data_ptr() + 4 * 512 - 1), overlaps), (dict(f=own.value), b"does not lie inside"), (dict(m=own.value + 480), b"does not lie inside")):
        assert mask_call(**kw) == EINVAL, kw
        assert fired(b"bm_water_mask", fragment), (kw, L.bm_last_error_string())
    torch.cuda.synchronize()
    assert (mask == 9).all().item() and (field == -1).all().item()
    assert L.bm_synchronize(scene.gpuScene) == 0 and L.bm_buffer_free(scene.device, own) == 0
    assert call(sea=8) == 0, L.bm_last_error_string()
    assert res.cpu().numpy().view(water.WATER_RESULT_DTYPE)[0].tolist() == (512, 8, 0, 0, 0) and field[7, 7, 7].item() == 8, "the call has waited"
    assert mask_call(depth=8) == 0
    torch.cuda.synchronize()
    assert (mask[0] == 1).all().item() and (mask[1:] == 0).all().item()
    assert call(flags=0, n=0, s=0) == 0 and (field == -1).sum().item() == 0 and (field == NONE).all().item(), "nothing is an outlet: no round runs"
    assert L.bm_debug_water_times(scene.gpuScene, None, None, None, 0, None, None, None, 0, None, 0, None, None) == EINVAL
    with pytest.raises(ValueError):
        water.water_field(scene, np.zeros((8, 8, 8), np.uint8))
    with pytest.raises(ValueError):
        water.water_field(scene, vol, [(1, 2)])
    with pytest.raises(ValueError):
        water.water_field(scene, vol, open=("down",))
    with pytest.raises(ValueError):
        water.water_field(scene, vol, sea_level=-1)


# ---------------------------------------------------------------- the scene level
def test_pools_of_a_box_across_the_terrain_a_carved_pit_and_its_drain(water, torch_cuda, scene):
    lo, hi = (32, 32, 40), (96, 96, 104)
    before = scene.read_region(lo, hi)
    column = np.flatnonzero(before[:, 32, 32])
    assert column.size and column.max() < 58, "the terrain surface crosses the box, with room above it"
    top = lo[2] + int(column.max())
    centre, radius = (64, 64, top - 3), 5
    scene.carve_sphere(centre, radius)
    try:
        box = scene.read_region(lo, hi).view(np.uint8)
        assert box.any() and not box.all() and not box[top - 3 - lo[2], 32, 32] and before.sum() > box.sum()
        want, rec = model.model_water_field(box)
        got = water.pools(scene, lo, hi)
        assert got.lo == lo and got.field.cpu().numpy().tobytes() == want.tobytes() and got.record == rec
        assert got.wet == int(rec["wet"]) > 0
        z, y, x = np.indices(box.shape)
        inside = (box == 0) & before   # what the sphere took out of the ground
        assert inside.sum() > 100 and (want[inside] > z[inside]).any(), "the pit holds water"
        pit = np.argwhere(inside)[0]   # its lowest voxel (the first in index order)
        assert got.mask().cpu().numpy().tobytes() == model.model_water_mask(want).tobytes()
        drain = (int(pit[2]) + lo[0], int(pit[1]) + lo[1], int(pit[0]) + lo[2])
        drained = water.pools(scene, lo, hi, drains=[drain, (0, 0, 0)])
        want2, rec2 = model.model_water_field(box, [(int(pit[2]), int(pit[1]), int(pit[0])), (-32, -32, -40)])
        assert drained.field.cpu().numpy().tobytes() == want2.tobytes() and drained.record == rec2 and int(rec2["drains_rejected"]) == 1
        assert (want2[inside] == z[inside]).all(), "the drain makes the pit dry"
        sea = water.pools(scene, lo, hi, sea_level=top + 2)
        want3, rec3 = model.model_water_field(box, sea_level=top + 2 - lo[2])
        assert sea.field.cpu().numpy().tobytes() == want3.tobytes() and sea.record == rec3 and sea.wet > got.wet
        assert water.pools(scene, lo, hi, sea_level=10 ** 6).record == model.model_water_field(box, sea_level=64)[1], "the sea is clamped into the box"
        with pytest.raises(ValueError):
            water.pools(scene, hi, lo)
    finally:
        scene.write_region(lo, before, op="replace")


# ---------------------------------------------------------------- the example
def test_headless_main_prints_the_pools(water, torch_cuda, tmp_path):
    """examples/headless_main --pools x0,y0,z0:x1,y1,z1 (C++ Scene::pools): a pit of 8 x 8 x 10 voxels in flat ground stands full"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "headless_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    vox = np.zeros((128, 128, 128), np.uint8)
    vox[:40] = 1
    vox[30:40, 60:68, 60:68] = 0
    world = tmp_path / "world.raw"
    vox.tofile(world)
    out = tmp_path / "frame.ppm"
    lo, hi = (48, 48, 20), (80, 80, 52)
    want, rec = water.host_water_field(vox[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]])
    assert (int(rec["wet"]), int(rec["closed"]), int(rec["deepest"])) == (640, 0, 10)
    r = subprocess.run([exe, "--voxels", str(world), "--pools", "48,48,20:80,80,52", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pools: 640 wet, 0 closed\n" in r.stdout and "deepest: 10 at 60,60,30\n" in r.stdout, r.stdout
    vox[30, 64, :64] = 0   # a tunnel from the pit's floor to the world's side: inside the box it ends at the box's side
    vox.tofile(world)
    r = subprocess.run([exe, "--voxels", str(world), "--pools", "48,48,20:80,80,52", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pools: 0 wet, 0 closed\nnothing is wet\n" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe, "--voxels", str(world), "--pools", "1,2,3", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--pools wants" in r.stderr
