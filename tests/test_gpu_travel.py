"""Scene.travel_field, TravelField.paths, Scene.reach and Scene.find_path on the MI355X (csrc/travel.hip): the device's field and its result
record must equal bm_host_travel_field -- the host routine that tests/test_travel_host.py pins to the numpy model -- byte for byte, and the
device's paths bm_host_travel_paths'.  Shapes are the smallest at which each part can go wrong: a lone tile and ragged tiles at every base
phase; the longest corridor of a tile; every face of a tile; tiles that are entered again; limits at, before and after a tile face; seeds
of every kind; more listed tiles than a round has waves; more rounds than one batch.  Then the scene level: a tunnel through a hill, a plug,
clearance, a streaming scene.  Every number is an integer, every comparison exact."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import _travel_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
NONE = model.NONE
RULES = open(os.path.join(ROOT, "brickmap_amd", "csrc", "travel.h")).read()
MAX_WAVES = int(re.search(r"kTravelMaxWaves = (\d+);", RULES).group(1))
BATCH = int(re.search(r"kTravelBatch = (\d+);", RULES).group(1))


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
    print(f"tests/test_gpu_travel.py took {time.time() - t0:.1f} s")


def random_volume(seed, shape, density, byte=1):
    return ((np.random.default_rng(seed).random(shape) < density) * byte).astype(np.uint8)


def random_points(seed, shape, n, margin=0):
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    return np.stack([rng.integers(-margin, nx + margin, n), rng.integers(-margin, ny + margin, n), rng.integers(-margin, nz + margin, n)], axis=1).astype(np.int32)


def first_open(vol):
    z, y, x = np.argwhere(vol == 0)[0]
    return int(x), int(y), int(z)


def check(bm, torch, scene, vol, seeds, max_steps=0, what=""):
    """device field and record of a contiguous upload of `vol` against the host routine"""
    want, rec = bm.host_travel_field(vol, seeds, max_steps)
    got = scene.travel_field(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), seeds, max_steps)
    field = got.field.cpu().numpy()
    assert field.dtype == np.int32 and field.shape == vol.shape
    assert field.tobytes() == want.tobytes(), f"{what} {vol.shape} limit {max_steps}: first difference at {np.argmax(field.ravel() != want.ravel())}"
    assert got.record == rec, f"{what} {vol.shape} limit {max_steps}: {got.record} on the device, {rec} on the host"
    return want, rec


def snake_tile():
    """the longest corridor without a branch of an 8^3 tile, [z, y, x] (tests/travel_check.cpp): 143 voxels from (0, 0, 0) to (0, 0, 6)"""
    v = np.ones((8, 8, 8), np.uint8)
    for z in (0, 2, 4, 6):
        v[z, 0::2, :] = 0
        v[z, 1, 7] = v[z, 3, 0] = v[z, 5, 7] = 0
    v[1, 6, 0] = v[3, 0, 0] = v[5, 6, 0] = 0
    return v


# ---------------------------------------------------------------- a lone tile and ragged tiles
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 9), (3, 4, 5), (9, 10, 11), (7, 13, 6)])
def test_a_lone_tile_and_ragged_tiles(shape, bm, torch_cuda, scene):
    for density in (0, 0.2, 0.3, 1):
        vol = random_volume(sum(shape), shape, density, 255)
        seeds = np.concatenate([random_points(1, shape, 2), [first_open(vol)] if (vol == 0).any() else [(0, 0, 0)]])
        for limit in (0, 3):
            check(bm, torch_cuda, scene, vol, seeds, limit, f"density {density}")


@pytest.mark.parametrize("x0", [1, 3, 4, 6])
def test_a_base_inside_an_allocation_and_larger_pitches(x0, bm, torch_cuda, scene):
    torch = torch_cuda
    big = random_volume(x0, (14, 19, 60), 0.25) * 7
    d_big = torch.from_numpy(big).cuda()
    for nx in (2, 8, 17, 33, 60 - x0):
        view = (slice(2, 13), slice(3, 16), slice(x0, x0 + nx))
        seeds = [first_open(big[view]), (nx - 1, 12, 10), (nx, 0, 0)]
        want, rec = bm.host_travel_field(big[view], seeds)
        got = scene.travel_field(d_big[view], seeds)
        assert got.record == rec and got.field.cpu().numpy().tobytes() == want.tobytes(), (x0, nx)
    assert d_big[view].data_ptr() % 4 == (d_big.data_ptr() + 2 * 19 * 60 + 3 * 60 + x0) % 4


# ---------------------------------------------------------------- the in-tile bound
def test_the_longest_corridor_of_a_tile_and_its_continuation(bm, torch_cuda, scene):
    """alone in an 8^3 volume the corridor is settled by one wave in one round; along each axis; then continued through a second tile"""
    tile = snake_tile()
    for axes in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        want, rec = check(bm, torch_cuda, scene, np.ascontiguousarray(tile.transpose(axes)), [(0, 0, 0)], what=f"corridor {axes}")
        assert (int(rec["reached"]), int(rec["farthest"])) == (143, 142)
    two = np.ones((16, 8, 8), np.uint8)
    two[:8], two[8:] = tile, tile
    two[7, 0, 0] = 0
    want, rec = check(bm, torch_cuda, scene, two, [(0, 0, 0)], what="two tiles")
    assert (int(rec["reached"]), int(rec["farthest"]), int(rec["farthest_at"])) == (287, 286, 14 * 64)
    want, rec = check(bm, torch_cuda, scene, two, [(0, 0, 14)], what="two tiles, from the far end")
    assert int(rec["farthest"]) == 286 and int(rec["farthest_at"]) == 0


# ---------------------------------------------------------------- every face
@pytest.mark.parametrize("corner", range(8))
def test_every_face_from_every_corner(corner, bm, torch_cuda, scene):
    seed = tuple(16 if (corner >> k) & 1 else 0 for k in range(3))
    want, rec = check(bm, torch_cuda, scene, np.zeros((17, 17, 17), np.uint8), [seed], what=f"corner {seed}")
    z, y, x = np.indices(want.shape)
    assert np.array_equal(want, abs(x - seed[0]) + abs(y - seed[1]) + abs(z - seed[2])) and int(rec["farthest"]) == 48
    vol = random_volume(17, (17, 17, 17), 0.3)
    vol[seed[2], seed[1], seed[0]] = 0
    check(bm, torch_cuda, scene, vol, [seed], what=f"corner {seed} at density 0.3")


# ---------------------------------------------------------------- a tile that is entered again
def test_a_tile_that_is_entered_again(bm, torch_cuda, scene):
    wall = np.zeros((8, 24, 24), np.uint8)
    wall[:, :23, 12] = 1   # across the middle tile column; the only gap is at the far end
    want, rec = check(bm, torch_cuda, scene, wall, [(0, 0, 0)], what="wall")
    assert want[0, 0, 13] == 12 + 23 + 23 + 1
    maze = np.ones((2, 24, 24), np.uint8)
    maze[0, 0::2, :] = 0
    maze[0, 1::4, 23] = 0
    maze[0, 3:23:4, 0] = 0
    want, rec = check(bm, torch_cuda, scene, maze, [(0, 0, 0)], what="serpentine")
    assert int(rec["reached"]) == 12 * 24 + 11 and int(rec["farthest"]) == 12 * 24 + 11 - 1, "one corridor: every tile of the 3 x 3 is crossed four times"
    check(bm, torch_cuda, scene, maze, [(23, 22, 0), (5, 0, 0)], what="serpentine, two seeds")


# ---------------------------------------------------------------- limits
@pytest.mark.parametrize("limit", [0, 1, 7, 8, 9, 20])
def test_limits_at_before_and_after_a_tile_face(limit, bm, torch_cuda, scene):
    want, rec = check(bm, torch_cuda, scene, np.zeros((20, 20, 20), np.uint8), [(0, 0, 0)], limit, "empty")
    z, y, x = np.indices(want.shape)
    d = x + y + z
    assert np.array_equal(want, np.where((d <= limit) | (limit == 0), d, NONE)) and int(rec["farthest"]) == (limit or 57)
    vol = random_volume(20, (20, 20, 20), 0.2)
    vol[0, 0, 0] = 0
    check(bm, torch_cuda, scene, vol, [(0, 0, 0)], limit, "density 0.2")


# ---------------------------------------------------------------- seeds
def test_seeds_of_every_kind(bm, torch_cuda, scene):
    vol = random_volume(3, (19, 21, 23), 0.3)
    want, rec = check(bm, torch_cuda, scene, vol, [], what="no seed")
    assert (want == NONE).all() and rec.tolist() == (0, NONE, 0, 0, 0)
    blocked = np.argwhere(vol != 0)[:5, ::-1]
    want, rec = check(bm, torch_cuda, scene, vol, np.concatenate([blocked, [(-1, 0, 0), (23, 0, 0), (0, 21, 0), (0, 0, 19)]]), what="all rejected")
    assert (want == NONE).all() and rec.tolist() == (0, NONE, 9, 0, 0)
    seeds = random_points(7, vol.shape, 1000, margin=1)
    seeds[500:] = seeds[:500]
    want, rec = check(bm, torch_cuda, scene, vol, seeds, what="1000 seeds")
    assert 0 < int(rec["seeds_rejected"]) < 1000 and int(rec["reached"]) > 1000
    check(bm, torch_cuda, scene, vol, seeds, 2, what="1000 seeds, limit 2")
    pocket = np.zeros((9, 9, 9), np.uint8)
    pocket[3:6, 3:6, 3:6] = 1
    pocket[4, 4, 4] = 0
    want, rec = check(bm, torch_cuda, scene, pocket, [(4, 4, 4)], what="pocket")
    assert rec.tolist() == (1, 0, 0, 4 * 81 + 4 * 9 + 4, 0)
    want, rec = check(bm, torch_cuda, scene, pocket, [(0, 0, 0)], what="round the pocket")
    assert want[4, 4, 4] == NONE and int(rec["reached"]) == 729 - 27
    want, rec = check(bm, torch_cuda, scene, np.full((9, 17, 8), 3, np.uint8), [(1, 1, 1), (7, 16, 8)], what="everything blocked")
    assert (want == NONE).all() and rec.tolist() == (0, NONE, 2, 0, 0)
    a_bool = scene.travel_field(torch_cuda.from_numpy(pocket != 0).cuda(), torch_cuda.tensor([[0, 0, 0]], dtype=torch_cuda.int32, device="cuda"))
    assert int(a_bool.record["reached"]) == 729 - 27, "a bool tensor is a volume and a device tensor a list of seeds"


# ---------------------------------------------------------------- more listed tiles than a round has waves, more rounds than a batch
def test_more_listed_tiles_than_the_grid_has_waves(bm, torch_cuda, scene):
    n = 168
    tiles = (n // 8) ** 3
    assert n % 8 == 0 and MAX_WAVES < tiles < 2 * MAX_WAVES, "every wave of the first round takes a second tile, the last turn ragged"
    vol = random_volume(5, (n, n, n), 0.2)
    c = np.arange(4, n, 8)
    zz, yy, xx = np.meshgrid(c, c, c, indexing="ij")
    vol[zz, yy, xx] = 0
    seeds = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1).astype(np.int32)
    want, rec = check(bm, torch_cuda, scene, vol, seeds, what="one seed per tile")
    assert len(seeds) == tiles and int(rec["seeds_rejected"]) == 0


def test_more_rounds_than_one_batch(bm, torch_cuda, scene):
    nx = 8 * (BATCH + 3)
    row = np.zeros((1, 1, nx), np.uint8)
    want, rec = check(bm, torch_cuda, scene, row, [(0, 0, 0)], what="a row")
    assert np.array_equal(want[0, 0], np.arange(nx)) and int(rec["farthest_at"]) == nx - 1
    got, (ms, rounds, looks) = scene.travel_field_times(torch_cuda.from_numpy(row).cuda(), [(0, 0, 0)])
    assert BATCH + 3 <= rounds <= 2 * BATCH and looks == 2 and len(ms) == 3 and all(t > 0 for t in ms)
    got, (ms, rounds, looks) = scene.travel_field_times(torch_cuda.from_numpy(row).cuda(), [(0, 0, 0)], batch=4)
    assert looks == -(-(BATCH + 4) // 4) and got.field.cpu().numpy().tobytes() == want.tobytes()
    check(bm, torch_cuda, scene, row, [(nx - 1, 0, 0)], BATCH * 8 + 1, what="a row, from the far end, with a limit")


# ---------------------------------------------------------------- mixed, twice; paths
@pytest.fixture(scope="module")
def mixed(bm):
    """33 x 70 x 129 at density 0.3, seeded at its first open voxel: (volume, seed, host field, host record), computed once"""
    vol = random_volume(4, (33, 70, 129), 0.3)
    seed = first_open(vol)
    field, rec = bm.host_travel_field(vol, [seed])
    assert int(rec["reached"]) > 0.99 * int((vol == 0).sum()) and int(rec["farthest"]) > 200, "long fronts, not an empty field"
    return vol, seed, field, rec


def test_mixed_twice_gives_the_same_bytes(mixed, bm, torch_cuda, scene):
    torch = torch_cuda
    vol, seed, want, rec = mixed
    d_vol = torch.from_numpy(vol).cuda()
    a = scene.travel_field(d_vol, [seed])
    out = torch.empty(vol.shape, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    b = scene.travel_field(d_vol, [seed], out=out, stream=s.cuda_stream)
    assert b.field is out and a.field.data_ptr() != out.data_ptr()
    assert a.field.cpu().numpy().tobytes() == out.cpu().numpy().tobytes() == want.tobytes() and a.record == b.record == rec
    assert a.reached == int(rec["reached"])


@pytest.mark.parametrize("capacity", [1, 8, 300])
def test_paths_against_the_host_routine(capacity, mixed, bm, torch_cuda, scene):
    torch = torch_cuda
    vol, seed, want, rec = mixed
    got = scene.travel_field(torch.from_numpy(vol).cuda(), [seed])
    starts = np.concatenate([random_points(capacity, vol.shape, 198, margin=1), [seed], [(int(rec["farthest_at"]) % 129, int(rec["farthest_at"]) // 129 % 70, int(rec["farthest_at"]) // (129 * 70))]])
    want_path, want_len = bm.host_travel_paths(want, starts, capacity)
    path, lengths = got.paths(starts, capacity)
    assert tuple(path.shape) == (200, capacity, 3) and path.dtype == torch.int32 and lengths.dtype == torch.int32
    path, lengths = path.cpu().numpy(), lengths.cpu().numpy()
    assert lengths.tobytes() == want_len.tobytes() and path.tobytes() == want_path.tobytes()
    assert (lengths == 0).any() and (lengths > 8).any() and lengths[-2] == 1 and lengths[-1] == int(rec["farthest"]) + 1 and not (lengths < 0).any()
    full = np.flatnonzero((lengths > 0) & (lengths <= capacity))
    assert len(full) > (100 if capacity == 300 else 0)
    for q in full:
        model.check_full_path(vol, want, path[q, :lengths[q]])
        assert tuple(path[q, lengths[q] - 1]) == seed
    if capacity == 300:
        whole = got.path(starts[-1])
        assert whole.shape == (int(rec["farthest"]) + 1, 3) and whole.tobytes() == path[-1, :lengths[-1]].tobytes()
        assert got.path((-1, 0, 0)) is None and got.path(np.argwhere(vol != 0)[0][::-1]) is None
        bad = got.field.clone()
        bad[bad == int(rec["farthest"]) - 3] = 5   # no voxel holds that value any more: the walk ends after three steps
        lengths = bm.TravelField(scene, bad, got.result).paths([whole[0]], 300)[1]
        assert lengths.cpu().numpy().tolist() == [-1], "a field that was not made by bm_travel_field"


# ---------------------------------------------------------------- refusals
def test_refusals_that_need_a_device(bm, torch_cuda, scene):
    torch = torch_cuda
    from brickmap_amd import _lib
    L = scene._L
    vol = torch.zeros((8, 8, 8), dtype=torch.uint8, device="cuda")
    need = bm.travel_workspace_bytes((8, 8, 8))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    field = torch.full((8, 8, 8), -1, dtype=torch.int32, device="cuda")
    seeds = torch.zeros((2, 3), dtype=torch.int32, device="cuda")

    def call(extent=(8, 8, 8), row=0, sl=0, flags=0, reserved=0, v=vol.data_ptr(), s=seeds.data_ptr(), n=2, f=field.data_ptr(), r=res.data_ptr(), w=ws.data_ptr(), wb=need):
        par = _lib.bm_travel_params()
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.flags, par.reserved = row, sl, flags, reserved
        return L.bm_travel_field(scene.gpuScene, C.byref(par), C.c_void_p(v), C.c_void_p(s), n, C.c_void_p(f), C.c_void_p(r), C.c_void_p(w), wb, None)

    def fired(entry, fragment):
        msg = L.bm_last_error_string()
        return msg.startswith(entry + b": ") and fragment in msg

    extent, null, aligned, overlaps = b"an extent below 1 or above 16384", b"null", b"aligned", b"overlaps"
    bad = [(dict(extent=(0, 8, 8)), extent), (dict(extent=(8, 8, 16385)), extent), (dict(extent=(16384, 16384, 8)), b"more than 2^31 - 2 voxels"),
           (dict(row=7), b"row_pitch below the extent along x"), (dict(sl=63), b"slice_pitch below row_pitch * the extent along y"), (dict(flags=1), b"unknown flag"),
           (dict(reserved=1), b"reserved is not 0"), (dict(n=-1), b"a negative number of seeds"), (dict(v=0), null), (dict(s=0), null), (dict(f=0), null), (dict(r=0), null),
           (dict(w=0), null), (dict(f=field.data_ptr() + 2), aligned), (dict(s=seeds.data_ptr() + 2), aligned), (dict(r=res.data_ptr() + 4), aligned),
           (dict(w=ws.data_ptr() + 8), aligned), (dict(wb=need - 1), b"smaller than"), (dict(w=vol.data_ptr(), wb=need), overlaps), (dict(v=ws.data_ptr() + 16), overlaps),
           (dict(f=ws.data_ptr()), overlaps), (dict(s=ws.data_ptr() + need - 16), overlaps), (dict(r=ws.data_ptr() + need - 32), overlaps), (dict(f=vol.data_ptr()), overlaps),
           (dict(s=field.data_ptr() + 64), overlaps)]
    for kw, fragment in bad:
        assert call(**kw) == EINVAL, kw
        assert fired(b"bm_travel_field", fragment), (kw, L.bm_last_error_string())
    # a volume whose pitches carry it 56 MiB past an allocation of 512 bytes (one of its own: torch's tensors share theirs)
    own = C.c_void_p()
    assert L.bm_buffer_alloc(scene.device, 512, C.byref(own)) == 0
    for kw in (dict(row=1 << 20, sl=8 << 20, v=own.value), dict(f=own.value), dict(s=own.value + 500)):
        assert call(**kw) == EINVAL and fired(b"bm_travel_field", b"does not lie inside"), (kw, L.bm_last_error_string())
    torch.cuda.synchronize()
    assert (field == -1).all().item() and not res.any().item() and not ws.any().item(), "nothing is launched and nothing written"

    path = torch.full((2, 4, 3), -5, dtype=torch.int32, device="cuda")
    lengths = torch.full((2,), -5, dtype=torch.int32, device="cuda")

    def walk(extent=(8, 8, 8), f=field.data_ptr(), s=seeds.data_ptr(), n=2, capacity=4, p=path.data_ptr(), l=lengths.data_ptr()):
        return L.bm_travel_paths(scene.gpuScene, (C.c_int32 * 3)(*extent) if extent else None, C.c_void_p(f), C.c_void_p(s), n, capacity, C.c_void_p(p), C.c_void_p(l), None)

    for kw, fragment in ((dict(extent=None), null), (dict(extent=(0, 8, 8)), extent), (dict(extent=(16384, 16384, 8)), b"more than 2^31 - 2 voxels"), (dict(f=0), null),
                         (dict(s=0), null), (dict(p=0), null), (dict(l=0), null), (dict(n=-1), b"a negative number of starts"), (dict(capacity=0), b"a capacity below 1"),
                         (dict(f=field.data_ptr() + 2), aligned), (dict(p=path.data_ptr() + 1), aligned), (dict(p=field.data_ptr()), overlaps), (dict(l=seeds.data_ptr()), overlaps),
                         (dict(f=own.value), b"does not lie inside"), (dict(p=own.value + 480), b"does not lie inside")):
        assert walk(**kw) == EINVAL, kw
        assert fired(b"bm_travel_paths", fragment), (kw, L.bm_last_error_string())
    torch.cuda.synchronize()
    assert (path == -5).all().item() and (lengths == -5).all().item()
    assert L.bm_synchronize(scene.gpuScene) == 0 and L.bm_buffer_free(scene.device, own) == 0
    assert call() == 0, L.bm_last_error_string()
    assert res.cpu().numpy().view(bm.TRAVEL_RESULT_DTYPE)[0].tolist() == (512, 21, 0, 511, 0) and field[7, 7, 7].item() == 21, "the call has waited"
    assert walk(s=0, p=0, l=0, n=0) == 0 and walk() == 0
    torch.cuda.synchronize()
    assert lengths.cpu().numpy().tolist() == [1, 1] and path[:, 0].cpu().numpy().tolist() == [[0, 0, 0], [0, 0, 0]]
    assert L.bm_debug_travel_times(scene.gpuScene, None, None, None, 0, None, None, None, 0, None, 0, None, None) == EINVAL
    with pytest.raises(ValueError):
        scene.travel_field(np.zeros((8, 8, 8), np.uint8), [])
    with pytest.raises(ValueError):
        scene.travel_field(vol, [(1, 2)])
    with pytest.raises(ValueError):
        scene.travel_field(vol, [], max_steps=-1)
    with pytest.raises(ValueError):
        bm.TravelField(scene, field, res).paths([(0, 0, 0)], 0)


# ---------------------------------------------------------------- the scene level
HILL_LO, HILL_HI = (40, 50, 100), (80, 62, 112)   # above the terrain of the generated world (its columns end below z = 96)
MOUTH_A, MOUTH_B = (39, 55, 105), (80, 55, 105)   # just outside the hill, at the two ends of the tunnel


def host_search(scene, lo, hi, start, goal, max_steps=0):
    """the length in voxels of a shortest path inside the box by the numpy model over read_region, or None"""
    box = scene.read_region(lo, hi).view(np.uint8)
    field, _ = model.model_travel_field(box, [[g - l for g, l in zip(goal, lo)]], max_steps)
    t = int(field[start[2] - lo[2], start[1] - lo[1], start[0] - lo[0]])
    return None if t == NONE else t + 1


@pytest.fixture()
def hill(scene):
    """a solid block in the air with a tunnel of one voxel's width along x through its middle; the box is emptied again afterwards"""
    assert not scene.read_region((30, 40, 96), (90, 72, 120)).any(), "the air above the terrain"
    scene.fill_box(HILL_LO, HILL_HI)
    scene.clear_box((40, 55, 105), (80, 56, 106))
    yield scene
    scene.clear_box(HILL_LO, HILL_HI)


def test_a_tunnel_through_a_hill_a_plug_and_the_way_round(hill, bm, torch_cuda):
    scene = hill
    path = scene.find_path(MOUTH_A, MOUTH_B)
    assert path.dtype == np.int32 and path.shape == (42, 3), "the tunnel's 40 voxels and the two mouths"
    assert np.array_equal(path, np.stack([np.arange(39, 81), np.full(42, 55), np.full(42, 105)], axis=1)), "straight through, the start first"
    lo, hi = [7, 23, 73], [113, 88, 128]   # the default box: the bounding box enlarged by 32, clipped to the world
    assert host_search(scene, lo, hi, MOUTH_A, MOUTH_B) == 42
    # an edit issued before find_path is seen by it: a plug across the tunnel
    scene.fill_box((60, 55, 105), (61, 56, 106))
    path = scene.find_path(MOUTH_A, MOUTH_B)
    want = host_search(scene, lo, hi, MOUTH_A, MOUTH_B)
    assert want == 42 + 12 and len(path) == want, "round the hill's side: six voxels out and six back"
    assert tuple(path[0]) == MOUTH_A and tuple(path[-1]) == MOUTH_B and (np.abs(np.diff(path, axis=0)).sum(axis=1) == 1).all()
    assert not scene.read_region(lo, hi)[path[:, 2] - lo[2], path[:, 1] - lo[1], path[:, 0] - lo[0]].any(), "no voxel of the path is solid"
    assert scene.find_path(MOUTH_A, MOUTH_B, max_steps=45) is None and host_search(scene, lo, hi, MOUTH_A, MOUTH_B, 45) is None
    # inside a box that holds the hill's cross-section and nothing round it there is no way
    assert scene.find_path(MOUTH_A, MOUTH_B, lo=(30, 50, 100), hi=(90, 62, 112)) is None
    assert scene.find_path(MOUTH_A, (60, 55, 105)) is None, "a goal inside the plug is a rejected seed"
    scene.clear_box((60, 55, 105), (61, 56, 106))
    assert len(scene.find_path(MOUTH_A, MOUTH_B)) == 42


def test_clearance_in_a_corridor_three_voxels_wide(hill, bm, torch_cuda):
    """reach() blocks a voxel when a solid one lies closer than clearance_sq: on the centre line of a corridor 3 voxels wide the nearest
    solid voxel is two steps away, squared distance 4, so clearance_sq 1 and 4 pass it and 5 does not; the tunnel of one voxel's width
    passes 1 only"""
    scene = hill
    lo, hi = (30, 50, 100), (90, 62, 112)   # the hill's cross-section: the only way is through
    assert len(scene.find_path(MOUTH_A, MOUTH_B, lo, hi, clearance_sq=1)) == 42
    assert scene.find_path(MOUTH_A, MOUTH_B, lo, hi, clearance_sq=2) is None
    scene.clear_box((40, 54, 104), (80, 57, 107))
    for clearance_sq, passes in ((0, True), (1, True), (2, True), (4, True), (5, False), (9, False)):
        path = scene.find_path(MOUTH_A, MOUTH_B, lo, hi, clearance_sq=clearance_sq)
        assert (path is not None) == passes, clearance_sq
        if passes and clearance_sq >= 2:
            assert np.array_equal(path[1:-1, 1:], np.tile([55, 105], (40, 1))), "only the centre line is that far from the walls"
    got = scene.reach(lo, hi, [MOUTH_B], clearance_sq=4)
    box = scene.read_region([v - 2 for v in lo], [v + 2 for v in hi])
    blocked = bm.host_distance_mask(bm.host_distance_field(box.view(np.uint8))[0], 3)[2:-2, 2:-2, 2:-2]
    want, rec = bm.host_travel_field(blocked, [[g - l for g, l in zip(MOUTH_B, lo)]])
    assert got.field.cpu().numpy().tobytes() == want.tobytes() and got.record == rec
    with pytest.raises(ValueError):
        scene.reach(lo, hi, [MOUTH_B], clearance_sq=-1)
    with pytest.raises(ValueError):
        scene.reach(hi, lo, [MOUTH_B])


def test_reach_in_a_streaming_scene_equals_the_preloaded_scenes(bm, torch_cuda, scene):
    lo, hi = (40, 40, 60), (72, 72, 100)   # across the terrain surface
    seeds = [(41, 41, 99), (70, 70, 99), (0, 0, 0)]
    want = scene.reach(lo, hi, seeds, max_steps=30)
    box = scene.read_region(lo, hi)
    assert box.any() and not box.all()
    host, rec = bm.host_travel_field(box.view(np.uint8), np.asarray(seeds) - np.asarray(lo))
    full = scene.reach(lo, hi, seeds)
    assert full.field.cpu().numpy().tobytes() == host.tobytes() and full.record == rec and int(rec["seeds_rejected"]) == 1
    s = bm.Scene(128, 128, device=0).generate()
    try:
        assert int(s.query_volumes(bm.volume_box(lo, hi)).unresolved[0]) > 0, "bricks of the box are absent"
        got = s.reach(lo, hi, seeds, max_steps=30)
        assert got.field.cpu().numpy().tobytes() == want.field.cpu().numpy().tobytes() and got.record == want.record
        assert int(got.record["farthest"]) == 30
    finally:
        s.close()


# ---------------------------------------------------------------- the example
def test_headless_main_finds_a_path(bm, torch_cuda, tmp_path):
    """examples/headless_main --path x0,y0,z0:x1,y1,z1 (C++ Scene::find_path): the length and the voxels it prints are the host routine's"""
    import subprocess
    exe = os.path.join(ROOT, "examples", "headless_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    vox = np.zeros((128, 128, 128), np.uint8)
    vox[40:60, 30:50, 20:60] = random_volume(13, (20, 20, 40), 0.3)
    vox[45, 35, 25] = vox[55, 45, 55] = 0
    world = tmp_path / "world.raw"
    vox.tofile(world)
    out = tmp_path / "frame.ppm"
    r = subprocess.run([exe, "--voxels", str(world), "--path", "25,35,45:55,45,55", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lo, hi = (0, 3, 13), (88, 78, 88)
    box = vox[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    field, _ = bm.host_travel_field(box, [(55 - lo[0], 45 - lo[1], 55 - lo[2])])
    path, lengths = bm.host_travel_paths(field, [(25 - lo[0], 35 - lo[1], 45 - lo[2])], 4096)
    m = re.search(r"path of (\d+) voxels:((?: -?\d+,-?\d+,-?\d+)+)", r.stdout)
    assert m and int(m.group(1)) == int(lengths[0]) > 50, r.stdout
    got = np.array([[int(v) for v in p.split(",")] for p in m.group(2).split()])
    assert np.array_equal(got, path[0, :lengths[0]] + np.asarray(lo))
    vox[44:47, 34:37, 24:27] = 1
    vox[45, 35, 25] = 0
    vox.tofile(world)
    r = subprocess.run([exe, "--voxels", str(world), "--path", "25,35,45:55,45,55", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "no path" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe, "--voxels", str(world), "--path", "1,2,3", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--path wants" in r.stderr
