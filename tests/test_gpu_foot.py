"""brickmap_amd.foot on the MI355X (csrc/foot.hip): the device's room bytes, field, record and paths must equal those of the host routines
-- which tests/test_foot_host.py pins to the numpy model -- byte for byte, on the cases of tests/_foot_model.py: the smallest shapes at
which each rule can go wrong (one voxel, a column taller than the cap, steps, ledges, lintels, two stands in one column, fronts wider
than a workgroup, more rounds than three batches, pitched volumes, seeds of every kind, 72 random volumes).  Then a live scene: a
staircase and a ledge.  Every number is an integer, every comparison exact."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

import _foot_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
RULES = open(os.path.join(ROOT, "brickmap_amd", "csrc", "foot.h")).read()
BATCH = int(re.search(r"kFootBatch = (\d+);", RULES).group(1))
NONE = model.NONE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def foot(bm):
    from brickmap_amd import foot
    return foot


@pytest.fixture(scope="module")
def scene(bm, torch_cuda):
    """an empty world of 128^3 voxels, the smallest there is: the operators only need its device"""
    s = bm.Scene.from_voxels(np.zeros((128, 128, 128), np.uint8))
    yield s
    s.close()


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_foot.py took {time.time() - t0:.1f} s")


def agent(c):
    return dict(height=c.height, climb=c.climb, drop=c.drop, toward=c.toward)


def host(foot, c):
    room = foot.host_foot_room(c.volume, c.floor)
    field, rec = foot.host_foot_field(room, c.seeds, max_steps=c.max_steps, **agent(c))
    return room, field, rec


def device_volume(torch, volume):
    """the volume on the device with the strides it has on the host: a view of a larger tensor where it is one there"""
    if volume.flags["C_CONTIGUOUS"]:
        return torch.from_numpy(volume).cuda()
    nz, ny, nx = volume.shape
    big = torch.ones((nz + 1, ny + 2, nx + 3), dtype=torch.uint8, device="cuda")
    big[:nz, :ny, :nx] = torch.from_numpy(np.ascontiguousarray(volume)).cuda()
    return big[:nz, :ny, :nx]


def device(torch, foot, scene, c, **kw):
    room = foot.foot_room(scene, device_volume(torch, c.volume), floor=c.floor)
    return room, foot.foot_field(scene, room, c.seeds, max_steps=c.max_steps, **agent(c), **kw)


@pytest.mark.parametrize("name", model.NAMES)
def test_device_equals_the_host_routines(name, foot, torch_cuda, scene):
    c = model.cases()[name]
    room, field, rec = host(foot, c)
    d_room, got = device(torch_cuda, foot, scene, c)
    print(name, "host", rec, "device", got.record)
    r = d_room.cpu().numpy()
    assert r.dtype == np.uint8 and r.shape == room.shape and r.tobytes() == room.tobytes(), f"room: first difference at {np.argmax(r.ravel() != room.ravel())}"
    f = got.field.cpu().numpy()
    assert f.dtype == np.int32 and f.shape == field.shape and f.tobytes() == field.tobytes(), f"field: first difference at {np.argmax(f.ravel() != field.ravel())}"
    assert got.record.tobytes() == rec.tobytes(), (got.record, rec)
    if name.startswith("random"):   # the issue's condition, on the host routine's record: no case passes by reaching nothing
        assert int(rec["reached"]) * 4 >= int(rec["standable"]) and int(rec["farthest"]) >= 25, rec
    if name == "pitched":
        assert not c.volume.flags["C_CONTIGUOUS"]
    # paths: from the farthest voxel in full and truncated, from the first seed, from a voxel that is no stand, from outside
    far = model.voxel_of(rec["farthest_at"], field.shape)
    starts = [far, c.seeds[0] if c.seeds else (0, 0, 0), (0, 0, field.shape[0] - 1), (-1, 0, 0), (0, field.shape[1], 0)]
    full = int(rec["farthest"]) + 1 if int(rec["reached"]) else 1
    for capacity in sorted({full, min(3, full)}):
        path, lengths = foot.host_foot_paths(room, field, starts, capacity, **agent(c))
        d_path, d_lengths = got.paths(starts, capacity)
        assert d_path.cpu().numpy().tobytes() == path.tobytes() and d_lengths.cpu().numpy().tobytes() == lengths.tobytes(), (capacity, d_lengths, lengths)
        assert int(lengths[0]) == (full if int(rec["reached"]) else 0) and lengths[3] == 0 and lengths[4] == 0
    whole = got.path(far)
    if int(rec["reached"]):
        assert whole.shape == (full, 3) and whole.tobytes() == foot.host_foot_paths(room, field, [far], full, **agent(c))[0][0].tobytes()
    else:
        assert whole is None


def test_the_host_looks_several_times_along_the_serpentine(foot, torch_cuda, scene):
    """the corridor is 300 stands long and one wide: a level is one stand, so the field needs 300 rounds -- the last finds nothing -- which
    is more than three batches, whatever the batch"""
    c = model.cases()["serpentine"]
    room, field, rec = host(foot, c)
    d_room = foot.foot_room(scene, device_volume(torch_cuda, c.volume))
    for batch in (0, 1, 7, 64):
        got, (ms, rounds, looks) = foot.foot_field_times(scene, d_room, c.seeds, batch=batch, **agent(c))
        b = batch or BATCH
        print(f"batch {b}: {rounds} rounds, {looks} looks, {ms} ms")
        assert got.field.cpu().numpy().tobytes() == field.tobytes() and got.record.tobytes() == rec.tobytes()
        assert rounds == -(-300 // b) * b and rounds >= 300 > 3 * BATCH and looks == rounds // b and len(ms) == 3
    cut, (ms, rounds, looks) = foot.foot_field_times(scene, d_room, c.seeds, max_steps=150, batch=8, **agent(c))
    assert int(cut.record["farthest"]) == 150 and cut.reached == 151 and rounds == 152 and looks == 19, "max_steps + 2 rounds at most"


def test_two_runs_and_a_side_stream_give_the_same_bytes(foot, torch_cuda, scene):
    """the volume is written on the current stream just before the calls on a side stream, which must see it"""
    torch = torch_cuda
    c = model.cases()[model.random_name(3, 0.3, (2, 2, 8), True)]
    room, field, rec = host(foot, c)
    _, a = device(torch, foot, scene, c)
    side = torch.cuda.Stream()
    staged = torch.from_numpy(c.volume).cuda()
    volume = torch.zeros_like(staged)
    big = torch.ones((4096, 4096), device="cuda")
    for _ in range(4):
        big = big @ big * 1e-4   # work in front of the copy on the producer's stream
    volume.copy_(staged)
    d_room = foot.foot_room(scene, volume, stream=side.cuda_stream)
    b = foot.foot_field(scene, d_room, c.seeds, stream=side.cuda_stream, **agent(c))
    assert a.field.data_ptr() != b.field.data_ptr()
    assert a.field.cpu().numpy().tobytes() == b.field.cpu().numpy().tobytes() == field.tobytes()
    assert d_room.cpu().numpy().tobytes() == room.tobytes() and a.record.tobytes() == b.record.tobytes() == rec.tobytes()
    out = torch.full(field.shape, 5, dtype=torch.int32, device="cuda")
    again = foot.foot_field(scene, d_room, c.seeds, out=out, **agent(c))
    assert again.field is out and out.cpu().numpy().tobytes() == field.tobytes()


def test_a_field_spoiled_by_hand_ends_the_walk(foot, torch_cuda, scene):
    c = model.cases()["serpentine"]
    room, field, rec = host(foot, c)
    _, got = device(torch_cuda, foot, scene, c)
    start = model.voxel_of(rec["farthest_at"], field.shape)
    x, y, z = got.path(start)[10].tolist()
    got.field[z, y, x] += 1
    spoiled = field.copy()
    spoiled[z, y, x] += 1
    path, lengths = got.paths([start, start], 400)
    want, want_lengths = foot.host_foot_paths(room, spoiled, [start, start], 400, **agent(c))
    assert lengths.tolist() == [-1, -1] == want_lengths.tolist() and path.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(RuntimeError):
        got.path(start)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_buffers_untouched(bm, foot, torch_cuda, scene):
    torch = torch_cuda
    from brickmap_amd import _lib
    L = scene._L
    c = model.cases()["seeds"]
    nz, ny, nx = c.volume.shape
    volume = torch.from_numpy(c.volume).cuda()
    good_room = foot.foot_room(scene, volume)
    room = torch.full((nz, ny, nx), 7, dtype=torch.uint8, device="cuda")
    need = foot.foot_workspace_bytes(c.volume.shape)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    field = torch.full((nz, ny, nx), 7, dtype=torch.int32, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    seeds = torch.tensor(c.seeds, dtype=torch.int32, device="cuda")
    n = len(c.seeds)
    path = torch.full((n, 4, 3), 7, dtype=torch.int32, device="cuda")
    lengths = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    vp = C.c_void_p

    def params(**kw):
        p = _lib.bm_foot_params()
        p.extent[:] = kw.pop("extent", (nx, ny, nz))
        p.height, p.climb, p.drop = 2, 1, 3
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def f_room(p=None, v=volume.data_ptr(), r=room.data_ptr()):
        return L.bm_foot_room(scene.gpuScene, p or params(), vp(v), vp(r), None)

    def f_field(p=None, r=good_room.data_ptr(), s=seeds.data_ptr(), n=n, f=field.data_ptr(), o=res.data_ptr(), w=ws.data_ptr(), wb=need):
        return L.bm_foot_field(scene.gpuScene, p or params(), vp(r), vp(s), n, vp(f), vp(o), vp(w), wb, None)

    def f_paths(p=None, r=good_room.data_ptr(), f=field.data_ptr(), s=seeds.data_ptr(), n=n, capacity=4, pa=path.data_ptr(), le=lengths.data_ptr()):
        return L.bm_foot_paths(scene.gpuScene, p or params(), vp(r), vp(f), vp(s), n, capacity, vp(pa), vp(le), None)

    def fired(who, fragment):
        msg = L.bm_last_error_string()
        return msg.startswith(who + b": ") and fragment in msg

    for kw, fragment in [(dict(height=0), b"height"), (dict(height=33), b"height"), (dict(climb=-1), b"climb"), (dict(climb=33), b"climb"), (dict(drop=-1), b"drop"),
                         (dict(drop=65), b"drop"), (dict(flags=4), b"unknown flag"), (dict(reserved=1), b"reserved"), (dict(reserved2=1), b"reserved"),
                         (dict(extent=(0, ny, nz)), b"an extent below 1"), (dict(extent=(16384, 16384, 8)), b"more than 2^31 - 2 voxels"), (dict(row_pitch=nx - 1), b"row_pitch"),
                         (dict(slice_pitch=nx * ny - 1), b"slice_pitch")]:
        for fn, who in ((f_room, b"bm_foot_room"), (f_field, b"bm_foot_field"), (f_paths, b"bm_foot_paths")):
            assert fn(p=params(**kw)) == EINVAL and fired(who, fragment), (kw, who, L.bm_last_error_string())
    null, aligned, overlaps = b"null", b"aligned", b"overlaps"
    for kw, fragment in [(dict(v=0), null), (dict(r=0), null), (dict(r=volume.data_ptr() + 8), overlaps)]:
        assert f_room(**kw) == EINVAL and fired(b"bm_foot_room", fragment), (kw, L.bm_last_error_string())
    for kw, fragment in [(dict(n=-1), b"a negative number of seeds"), (dict(r=0), null), (dict(s=0), null), (dict(f=0), null), (dict(o=0), null), (dict(w=0), null),
                         (dict(wb=need - 1), b"smaller than"), (dict(f=field.data_ptr() + 2), aligned), (dict(s=seeds.data_ptr() + 2), aligned), (dict(o=res.data_ptr() + 4), aligned),
                         (dict(w=ws.data_ptr() + 8), aligned), (dict(f=ws.data_ptr() + 16), overlaps), (dict(s=ws.data_ptr()), overlaps), (dict(o=ws.data_ptr() + need - 32), overlaps),
                         (dict(o=field.data_ptr() + 8), b"the field overlaps"), (dict(r=field.data_ptr() + 4), b"the room volume overlaps"),
                         (dict(r=ws.data_ptr() + 16), b"the room volume overlaps"), (dict(r=res.data_ptr() - 8), b"the room volume overlaps")]:
        assert f_field(**kw) == EINVAL and fired(b"bm_foot_field", fragment), (kw, L.bm_last_error_string())
    for kw, fragment in [(dict(n=-1), b"a negative number of starts"), (dict(capacity=0), b"capacity"), (dict(r=0), null), (dict(f=0), null), (dict(s=0), null), (dict(pa=0), null),
                         (dict(le=0), null), (dict(pa=path.data_ptr() + 2), aligned), (dict(capacity=1 << 30, n=1 << 20), b"2^40"), (dict(pa=field.data_ptr()), overlaps),
                         (dict(le=seeds.data_ptr()), overlaps), (dict(le=path.data_ptr() + 4), overlaps), (dict(r=path.data_ptr()), b"the room volume overlaps"),
                         (dict(r=lengths.data_ptr()), b"the room volume overlaps")]:
        assert f_paths(**kw) == EINVAL and fired(b"bm_foot_paths", fragment), (kw, L.bm_last_error_string())
    own = C.c_void_p()   # an allocation of 512 bytes of its own: torch's tensors share theirs
    assert L.bm_buffer_alloc(scene.device, 512, C.byref(own)) == 0
    outside = b"does not lie inside"
    assert f_room(v=own.value + 500) == EINVAL and fired(b"bm_foot_room", outside) and f_room(r=own.value + 500) == EINVAL and fired(b"bm_foot_room", outside)
    for kw in (dict(r=own.value + 500), dict(f=own.value + 400), dict(w=own.value + 496), dict(o=own.value + 488)):
        assert f_field(**kw) == EINVAL and fired(b"bm_foot_field", outside), (kw, L.bm_last_error_string())
    for kw in (dict(r=own.value + 500), dict(f=own.value + 400), dict(pa=own.value + 400), dict(le=own.value + 508)):
        assert f_paths(**kw) == EINVAL and fired(b"bm_foot_paths", outside), (kw, L.bm_last_error_string())
    torch.cuda.synchronize()
    assert (room == 7).all().item() and (field == 7).all().item() and (path == 7).all().item() and (lengths == 7).all().item() and not res.any().item() and not ws.any().item(), \
        "nothing is launched and nothing written"
    assert L.bm_synchronize(scene.gpuScene) == 0 and L.bm_buffer_free(scene.device, own) == 0
    assert L.bm_debug_foot_times(scene.gpuScene, params(), vp(good_room.data_ptr()), vp(seeds.data_ptr()), n, vp(field.data_ptr()), vp(res.data_ptr()), vp(ws.data_ptr()), need, None, 0,
                                 None, None) == EINVAL
    assert L.bm_foot_room(None, params(), vp(volume.data_ptr()), vp(room.data_ptr()), None) == EINVAL
    # the calls as they are meant pass, and the field call has waited when it returns
    want_room, want_field, want_rec = host(foot, c)
    assert f_room() == 0 and f_field(w=ws.data_ptr() + 16) == 0, L.bm_last_error_string()
    assert field.cpu().numpy().tobytes() == want_field.tobytes() and res.cpu().numpy().tobytes() == want_rec.tobytes()
    assert f_paths() == 0
    want_path, want_lengths = foot.host_foot_paths(want_room, want_field, c.seeds, 4, **agent(c))
    torch.cuda.synchronize()
    assert room.cpu().numpy().tobytes() == want_room.tobytes() and lengths.cpu().numpy().tobytes() == want_lengths.tobytes()
    for q, length in enumerate(want_lengths.tolist()):   # (the C call leaves the rest of the buffer as it was)
        assert (path[q].cpu().numpy()[:min(length, 4)] == want_path[q, :min(length, 4)]).all() and (path[q, max(min(length, 4), 0):] == 7).all().item()
    assert f_field(n=0, s=0) == 0 and f_paths(n=0, s=0, pa=0, le=0) == 0 and (field == NONE).all().item(), "without seeds or starts the pointers may be null"
    for bad_room in (want_room, good_room.to(torch.int32), good_room[:, :, ::2]):
        with pytest.raises(ValueError):
            foot.foot_field(scene, bad_room, c.seeds)
    with pytest.raises(ValueError):
        foot.foot_field(scene, good_room, c.seeds, height=0)
    with pytest.raises(ValueError):
        foot.foot_room(scene, c.volume)


# ---------------------------------------------------------------- a live scene
BOX = ((0, 0, 0), (64, 64, 64))   # the 64^3 box of the world that holds the staircase and the ledge


def stairs_world():
    """128^3: ground four voxels thick; between y = 10 and y = 30 a staircase that rises by one every two voxels from x = 20 to a plateau
    whose stands are at z = 12 (x = 36 ... 49), and behind the plateau's edge a terrace three voxels lower (x = 50 ... 59)"""
    v = np.zeros((128, 128, 128), np.uint8)
    v[0:4] = 1
    for i in range(8):
        v[4:5 + i, 10:30, 20 + 2 * i:22 + 2 * i] = 1
    v[4:12, 10:30, 36:50] = 1
    v[4:9, 10:30, 50:60] = 1
    return v


def host_walk(foot, vox, start, goal, height=2, climb=1, drop=3):
    lo, hi = BOX
    box = np.ascontiguousarray(vox[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]).view(np.uint8)
    room = foot.host_foot_room(box, floor=lo[2] == 0)
    ends = foot.ground(room, [[s - l for s, l in zip(start, lo)], [g - l for g, l in zip(goal, lo)]], height)
    if None in ends:
        return room, None
    field, _ = foot.host_foot_field(room, [ends[1]], height, climb, drop, toward=True)
    t = int(field[ends[0][2], ends[0][1], ends[0][0]])
    if t == NONE:
        return room, None
    path, lengths = foot.host_foot_paths(room, field, [ends[0]], t + 1, height, climb, drop, toward=True)
    assert lengths.tolist() == [t + 1]
    return room, path[0] + np.asarray(lo, np.int32)


def test_find_walk_takes_the_stairs_and_the_ledge(bm, foot, torch_cuda):
    vox = stairs_world()
    scene = bm.Scene.from_voxels(vox)
    try:
        start, goal = (5, 20, 30), (55, 20, 40)   # in the air above the ground and above the terrace: both snap down
        walk = foot.find_walk(scene, start, goal, *BOX)
        room, want = host_walk(foot, scene.voxels(), start, goal)
        assert walk is not None and walk.dtype == np.int32 and walk.tobytes() == want.tobytes()
        assert walk[0].tolist() == [5, 20, 4] and walk[-1].tolist() == [55, 20, 9] and len(walk) == 51, "50 moves: one per column along x"
        assert walk[:, 2].max() == 12 and [12, 9] in [[int(a[2]), int(b[2])] for a, b in zip(walk, walk[1:])], "up the stairs, across the plateau, down the ledge"
        cells = model.lists(room)
        for p, q in zip(walk.tolist(), walk[1:].tolist()):
            assert model.legal(cells, tuple(p), tuple(q), 2, 1, 3), (p, q)
        assert foot.find_walk(scene, goal, start, *BOX) is None, "a ledge of three is not climbed"
        assert foot.find_walk(scene, start, goal, *BOX, drop=2) is None and foot.find_walk(scene, start, (100, 20, 40), *BOX) is None
        default = foot.find_walk(scene, (5, 20, 4), (30, 20, 40))   # the default box: the two ends' bounding box enlarged
        assert default is not None and default[-1].tolist() == [30, 20, 10] and len(default) == 26
        # an edit that makes the ledge too high: the terrace loses its top layer
        scene.clear_box((50, 10, 8), (60, 30, 9))
        room, want = host_walk(foot, scene.voxels(), start, goal)
        assert want is None and foot.find_walk(scene, start, goal, *BOX) is None, "find_walk sees the edit: a drop of four"
        # and one that builds a step in front of it: the walk comes back, one move longer in height only
        scene.fill_box((50, 19, 8), (51, 22, 10))
        walk = foot.find_walk(scene, start, goal, *BOX)
        room, want = host_walk(foot, scene.voxels(), start, goal)
        assert walk is not None and walk.tobytes() == want.tobytes() and walk[-1].tolist() == [55, 20, 8]
    finally:
        scene.close()


def test_headless_main_walks_like_the_host_routine(bm, foot, torch_cuda, tmp_path):
    """examples/headless_main --walk x0,y0,z0:x1,y1,z1 (C++ Scene::find_walk): the length it prints is the host routine's"""
    exe = os.path.join(ROOT, "examples", "headless_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    vox = stairs_world()
    world = tmp_path / "world.raw"
    vox.tofile(world)
    r = subprocess.run([exe, "--voxels", str(world), "--walk", "5,20,30:55,20,40", "128", "128", "64", "48", "1", str(tmp_path / "frame.ppm")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"walk of (\d+) voxels:((?: -?\d+,-?\d+,-?\d+)+)", r.stdout)
    assert m, r.stdout
    got = np.array([[int(v) for v in p.split(",")] for p in m.group(2).split()], np.int32)
    assert int(m.group(1)) == len(got) == 51 and got[0].tolist() == [5, 20, 4] and got[-1].tolist() == [55, 20, 9]
    cells = model.lists(foot.host_foot_room(vox))
    for p, q in zip(got.tolist(), got[1:].tolist()):
        assert model.legal(cells, tuple(p), tuple(q), 2, 1, 3), (p, q)
    r = subprocess.run([exe, "--voxels", str(world), "--walk", "55,20,40:5,20,30", "128", "128", "64", "48", "1", str(tmp_path / "frame.ppm")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "no way on foot" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe, "--walk", "1,2,3", "128", "128", "64", "48", "1", str(tmp_path / "frame.ppm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--walk wants" in r.stderr
