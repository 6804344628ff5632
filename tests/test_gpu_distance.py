"""Scene.distance_field, DistanceField.mask, Scene.clearance, Scene.grow and Scene.shrink on the MI355X (csrc/distance.hip): the device's
field and its result record must equal bm_host_distance_field -- the host routine that tests/test_distance_host.py pins to the brute-force
numpy model -- byte for byte.  Shapes are the smallest at which each pass can go wrong: rows of one lane, of a segment of a wave, of one
chunk exactly and of several chunks with a ragged last one; lines past a wave, short and long; sources far away, none and everywhere; bases
1, 3, 4 and 6 bytes into an allocation with pitches above the extents.  Then the scene level: grow and shrink against a numpy dilation by
shifting, at the world's border, in a streaming scene, and seen by a ray.  Every number is an integer, every comparison exact."""
import ctypes as C
import time

import numpy as np
import pytest

import _distance_model as model

pytestmark = pytest.mark.gpu
EINVAL = 10001
NONE = model.NONE
FLAGS = [("solid", False), ("solid", True), ("empty", False), ("empty", True)]


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
    print(f"tests/test_gpu_distance.py took {time.time() - t0:.1f} s")


def random_volume(seed, shape, density, byte=1):
    return ((np.random.default_rng(seed).random(shape) < density) * byte).astype(np.uint8)


def check(bm, torch, scene, vol, to="solid", outside=False, what=""):
    """device field and record of a contiguous upload of `vol` against the host routine"""
    want, rec = bm.host_distance_field(vol, to, outside)
    got = scene.distance_field(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), to, outside)
    field = got.field.cpu().numpy()
    assert field.dtype == np.int32 and field.shape == vol.shape
    assert field.tobytes() == want.tobytes(), f"{what} {vol.shape} to {to} outside {outside}: first difference at {np.argmax(field.ravel() != want.ravel())}"
    assert got.record == rec, f"{what} {vol.shape} to {to} outside {outside}: {got.record} on the device, {rec} on the host"
    return want, rec


# ---------------------------------------------------------------- the x pass: chunk carry and ragged ends
@pytest.mark.parametrize("nx", [1, 31, 63, 64, 65, 129, 200])
def test_rows_at_chunk_edges(nx, bm, torch_cuda, scene):
    """(nz, ny) = (2, 3); sources only at the first voxel, only at the last, none; random densities 0.03 and 0.5"""
    first, last, none = (np.zeros((2, 3, nx), np.uint8) for _ in range(3))
    first[:, :, 0] = 9
    last[:, :, -1] = 255
    for name, vol in (("first", first), ("last", last), ("none", none), ("0.03", random_volume(nx, (2, 3, nx), 0.03)), ("0.5", random_volume(nx, (2, 3, nx), 0.5, 128))):
        for to, outside in FLAGS:
            check(bm, torch_cuda, scene, vol, to, outside, name)
    # one row with sources, one without, side by side
    mixed = np.zeros((2, 3, nx), np.uint8)
    mixed[1, 1, nx // 2] = 1
    want, _ = check(bm, torch_cuda, scene, mixed, what="one source")
    assert want[1, 1, 0] == (nx // 2) ** 2


@pytest.mark.parametrize("shape", [(96, 97, 33), (261, 260, 5), (725, 726, 1)])
def test_more_rows_than_one_round_of_waves(shape, bm, torch_cuda, scene):
    """the x pass's grid ends at 2048 workgroups of four waves (csrc/distance.hip kRowBlocks): beyond 8192 turns -- of one row, of eight
    rows and of 64 rows -- a wave takes a second turn, the last one ragged"""
    nz, ny, nx = shape
    per_turn = 1 if nx > 32 else 64 // (1 << (nx - 1).bit_length())
    assert 8192 < -(-nz * ny // per_turn) < 2 * 8192 and (per_turn == 1 or (nz * ny) % per_turn != 0)
    check(bm, torch_cuda, scene, random_volume(6, shape, 0.1), what="two turns")
    check(bm, torch_cuda, scene, random_volume(7, shape, 0.6), "empty", True, what="two turns")


# ---------------------------------------------------------------- the line passes: lanes past a wave, short and long lines
@pytest.mark.parametrize("shape", [(3, 1, 65), (1, 2, 65), (65, 2, 3), (2, 130, 5), (130, 3, 67)])
def test_lines_past_a_wave_short_and_long(shape, bm, torch_cuda, scene):
    for density in (0.002, 0.05, 0.5):
        for to, outside in FLAGS:
            check(bm, torch_cuda, scene, random_volume(3, shape, density), to, outside, f"density {density}")


@pytest.mark.parametrize("at", [(0, 0, 0), (39, 39, 39), (20, 20, 20), (39, 0, 17)])
def test_far_sites(at, bm, torch_cuda, scene):
    vol = np.zeros((40, 40, 40), np.uint8)
    vol[at] = 200
    want, rec = check(bm, torch_cuda, scene, vol, what="one source")
    z, y, x = np.indices(vol.shape)
    assert np.array_equal(want, (z - at[0]) ** 2 + (y - at[1]) ** 2 + (x - at[2]) ** 2) and int(rec["sources"]) == 1
    check(bm, torch_cuda, scene, vol, outside=True, what="one source")


def test_no_source_and_all_sources(bm, torch_cuda, scene):
    for shape in ((5, 6, 7), (3, 5, 70)):
        want, rec = check(bm, torch_cuda, scene, np.zeros(shape, np.uint8), what="no source")
        assert (want == NONE).all() and (int(rec["sources"]), int(rec["max_sq"]), int(rec["max_at"])) == (0, NONE, 0)
        want, rec = check(bm, torch_cuda, scene, np.ones(shape, np.uint8), to="empty", what="no source")
        assert (want == NONE).all() and (int(rec["sources"]), int(rec["max_sq"]), int(rec["max_at"])) == (0, NONE, 0)
        check(bm, torch_cuda, scene, np.zeros(shape, np.uint8), outside=True, what="the border only")
        want, rec = check(bm, torch_cuda, scene, np.full(shape, 3, np.uint8), what="all sources")
        assert not want.any() and (int(rec["sources"]), int(rec["max_sq"]), int(rec["max_at"])) == (want.size, 0, 0)
        want, rec = check(bm, torch_cuda, scene, np.zeros(shape, np.uint8), to="empty", outside=True, what="all sources")
        assert not want.any() and int(rec["sources"]) == want.size


@pytest.mark.parametrize("density", [0.001, 0.05, 0.5])
def test_mixed(density, bm, torch_cuda, scene):
    vol = random_volume(4, (33, 70, 129), density, 255)
    for to, outside in FLAGS:
        check(bm, torch_cuda, scene, vol, to, outside, f"density {density}")


@pytest.mark.parametrize("x0", [1, 3, 4, 6])
def test_a_base_inside_an_allocation_and_larger_pitches(x0, bm, torch_cuda, scene):
    """the volume is a slice of a larger tensor that starts 1, 3, 4 and 6 bytes into it: byte and word loads at every phase"""
    torch = torch_cuda
    big = random_volume(x0, (14, 19, 210), 0.04) * 7
    d_big = torch.from_numpy(big).cuda()
    for nx in (2, 8, 17, 33, 64, 131, 210 - x0):
        view = (slice(2, 13), slice(3, 16), slice(x0, x0 + nx))
        for to, outside in (("solid", False), ("empty", True)):
            want, rec = bm.host_distance_field(big[view], to, outside)
            got = scene.distance_field(d_big[view], to, outside)
            assert got.record == rec and got.field.cpu().numpy().tobytes() == want.tobytes(), (x0, nx, to, outside)
    assert d_big[view].data_ptr() % 4 == (d_big.data_ptr() + 2 * 19 * 210 + 3 * 210 + x0) % 4


def test_result_record_and_the_tie(bm, torch_cuda, scene):
    vol = np.zeros((9, 9, 9), np.uint8)
    vol[4, 4, 2] = vol[4, 4, 6] = 1
    want, rec = check(bm, torch_cuda, scene, vol, what="two symmetric sources")
    assert (int(rec["sources"]), int(rec["max_sq"]), int(rec["max_at"])) == (2, 36, 0) and int((want == 36).sum()) == 12
    # ties in other waves and other lines: the farthest voxels are the two ends of a long axis
    vol = np.zeros((3, 131, 3), np.uint8)
    vol[1, 65, 1] = 1
    want, rec = check(bm, torch_cuda, scene, vol, what="mirrored along y")
    assert int(rec["max_at"]) == 0 and want.ravel()[0] == want.ravel()[-1] == int(rec["max_sq"])
    got = scene.distance_field(torch_cuda.from_numpy(vol).cuda())
    assert got.largest() == ((0, 0, 0), 65 * 65 + 2) and got.sources == 1
    assert scene.distance_field(torch_cuda.zeros((2, 2, 2), dtype=torch_cuda.uint8, device="cuda")).largest() is None
    b = scene.distance_field(torch_cuda.from_numpy(vol != 0).cuda())
    assert b.record == rec, "a bool tensor is a volume too"


# ---------------------------------------------------------------- the mask
def test_mask_against_numpy(bm, torch_cuda, scene):
    torch = torch_cuda
    vol = random_volume(5, (7, 9, 11), 0.02)   # 693 voxels: no multiple of 4
    vol[3] = 0
    for v in (vol, np.zeros((3, 5, 7), np.uint8)):
        got = scene.distance_field(torch.from_numpy(v).cuda())
        field = got.field.cpu().numpy()
        for limit in (0, 1, 2, 9, NONE - 1, NONE, 0xFFFFFFFF):
            for above in (False, True):
                m = got.mask(limit, above)
                assert m.dtype == torch.uint8 and tuple(m.shape) == v.shape
                assert m.cpu().numpy().tobytes() == model.model_mask(field, limit, above).tobytes() == bm.host_distance_mask(field, limit, above).tobytes(), (limit, above)
    # an output at every byte phase, with guard bytes around it
    got = scene.distance_field(torch.from_numpy(vol).cuda())
    want = model.model_mask(got.field.cpu().numpy(), 4).reshape(-1)
    for phase in (0, 1, 2, 3):
        for n in (want.size, 1, 2, 3, 5):
            buf = torch.full((want.size + 16,), 77, dtype=torch.uint8, device="cuda")
            assert scene._L.bm_distance_mask(scene.gpuScene, n, C.c_void_p(got.field.data_ptr()), 4, 0, C.c_void_p(buf.data_ptr() + 4 + phase), None) == 0
            torch.cuda.synchronize()
            out = buf.cpu().numpy()
            assert (out[:4 + phase] == 77).all() and (out[4 + phase + n:] == 77).all(), f"phase {phase} count {n}: a byte outside the output was written"
            assert np.array_equal(out[4 + phase:4 + phase + n], want[:n]), (phase, n)
    with pytest.raises(ValueError):
        got.mask(-1)


def test_two_runs_on_two_streams_give_the_same_bytes(bm, torch_cuda, scene):
    torch = torch_cuda
    vol = random_volume(4, (33, 70, 129), 0.05)
    want, rec = bm.host_distance_field(vol, "solid", True)
    d_vol = torch.from_numpy(vol).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = scene.distance_field(d_vol, outside=True, stream=s1.cuda_stream)
    b = scene.distance_field(d_vol, outside=True, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert a.field.data_ptr() != b.field.data_ptr()
    assert a.field.cpu().numpy().tobytes() == b.field.cpu().numpy().tobytes() == want.tobytes() and a.record == b.record == rec
    out = torch.empty(vol.shape, dtype=torch.int32, device="cuda")
    c = scene.distance_field(d_vol, outside=True, out=out)
    assert c.field is out and out.cpu().numpy().tobytes() == want.tobytes()
    d, ms = scene.distance_field_times(d_vol, outside=True)
    assert len(ms) == 3 and all(t > 0 for t in ms) and d.field.cpu().numpy().tobytes() == want.tobytes()


def test_refusals_that_need_a_device(bm, torch_cuda, scene):
    torch = torch_cuda
    from brickmap_amd import _lib
    L = scene._L
    vol = torch.ones((8, 8, 8), dtype=torch.uint8, device="cuda")
    need = bm.distance_workspace_bytes((8, 8, 8))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    field = torch.full((8, 8, 8), -1, dtype=torch.int32, device="cuda")

    def call(extent=(8, 8, 8), row=0, sl=0, flags=0, reserved=0, v=vol.data_ptr(), f=field.data_ptr(), r=res.data_ptr(), w=ws.data_ptr(), wb=need):
        par = _lib.bm_distance_params()
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.flags, par.reserved = row, sl, flags, reserved
        return L.bm_distance_field(scene.gpuScene, C.byref(par), C.c_void_p(v), C.c_void_p(f), C.c_void_p(r), C.c_void_p(w), wb, None)

    def fired(entry, fragment):
        msg = L.bm_last_error_string()
        return msg.startswith(entry + b": ") and fragment in msg

    def refused(kw, fragment):
        assert call(**kw) == EINVAL, kw
        assert fired(b"bm_distance_field", fragment), (kw, L.bm_last_error_string())

    extent, null, aligned, overlaps = b"an extent below 1 or above 16384", b"null", b"aligned", b"overlaps"
    bad = [(dict(extent=(0, 8, 8)), extent), (dict(extent=(8, 8, 16385)), extent), (dict(extent=(16384, 16384, 8)), b"more than 2^31 - 2 voxels"),
           (dict(row=7), b"row_pitch below the extent along x"), (dict(sl=63), b"slice_pitch below row_pitch * the extent along y"), (dict(flags=4), b"unknown flag"),
           (dict(reserved=1), b"reserved is not 0"), (dict(v=0), null), (dict(f=0), null), (dict(r=0), null), (dict(w=0), null),
           (dict(f=field.data_ptr() + 2), aligned), (dict(r=res.data_ptr() + 4), aligned), (dict(w=ws.data_ptr() + 8), aligned), (dict(wb=need - 1), b"smaller than"),
           (dict(w=vol.data_ptr(), wb=need), overlaps), (dict(v=ws.data_ptr() + 16), overlaps), (dict(f=ws.data_ptr()), overlaps), (dict(f=ws.data_ptr() + need - 16), overlaps),
           (dict(r=ws.data_ptr() + need - 32), overlaps), (dict(f=vol.data_ptr()), overlaps)]
    for kw, fragment in bad:
        refused(kw, fragment)
    # a volume whose pitches carry it 56 MiB past an allocation of 512 bytes (one of its own: torch's tensors share theirs)
    own = C.c_void_p()
    assert L.bm_buffer_alloc(scene.device, 512, C.byref(own)) == 0
    refused(dict(row=1 << 20, sl=8 << 20, v=own.value), b"does not lie inside")
    refused(dict(f=own.value), b"does not lie inside")   # 2048 bytes of field do not fit 512
    torch.cuda.synchronize()
    assert (field == -1).all().item() and not res.any().item() and not ws.any().item(), "nothing is launched and nothing written"
    # the mask's
    out = torch.full((520,), 9, dtype=torch.uint8, device="cuda")
    for args, fragment in (((0, field.data_ptr(), 1, 0, out.data_ptr()), b"a count of 0"), ((512, field.data_ptr(), 1, 2, out.data_ptr()), b"unknown flag"),
                           ((512, 0, 1, 0, out.data_ptr()), null), ((512, field.data_ptr(), 1, 0, 0), null), ((512, field.data_ptr() + 2, 1, 0, out.data_ptr()), aligned),
                           ((512, field.data_ptr(), 1, 0, field.data_ptr() + 100), overlaps), ((512, field.data_ptr(), 1, 0, own.value + 1), b"does not lie inside")):
        assert L.bm_distance_mask(scene.gpuScene, args[0], C.c_void_p(args[1]), args[2], args[3], C.c_void_p(args[4]), None) == EINVAL, args
        assert fired(b"bm_distance_mask", fragment), (args, L.bm_last_error_string())
    torch.cuda.synchronize()
    assert (out == 9).all().item() and (field == -1).all().item()
    assert L.bm_synchronize(scene.gpuScene) == 0 and L.bm_buffer_free(scene.device, own) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert not field.any().item() and res.cpu().numpy().view(bm.DISTANCE_RESULT_DTYPE)[0].tolist() == (512, 0, 0, 0, 0)
    assert L.bm_debug_distance_times(scene.gpuScene, None, None, None, None, None, 0, None, None) == EINVAL
    with pytest.raises(ValueError):
        scene.distance_field(np.ones((8, 8, 8), np.uint8))
    with pytest.raises(ValueError):
        scene.distance_field(vol, to="nowhere")


# ---------------------------------------------------------------- the scene level
def surface_box(scene, size=24, x0=None, y0=None):
    """a box of size^3 across the terrain surface: around the world's centre, or with its lower corner's (x, y) given"""
    g = scene.grid_size
    x0 = g // 2 - size // 2 if x0 is None else x0
    y0 = g // 2 - size // 2 if y0 is None else y0
    column = scene.voxels()[:, y0 + size // 2, x0 + size // 2]
    top = int(np.nonzero(column)[0].max()) if column.any() else size // 2
    z0 = max(0, min(scene.grid_height - size, top - size // 2))
    return (x0, y0, z0), (x0 + size, y0 + size, z0 + size)


def box_of(world, lo, hi, margin=0):
    """the voxels lo - margin <= v < hi + margin of a world [z, y, x], empty outside it"""
    pad = np.pad(world, margin)
    return pad[lo[2]:hi[2] + 2 * margin, lo[1]:hi[1] + 2 * margin, lo[0]:hi[0] + 2 * margin]


def morph_check(scene, lo, hi, radius_sq, op):
    """grow or shrink the box and compare the whole world with the model's; restores the box.  Returns the voxels changed."""
    before = scene.voxels().copy()
    m = model.model_ball(radius_sq)[1]
    sub = box_of(before, lo, hi, m)
    want_box = (model.model_dilate(sub, radius_sq) if op == "grow" else model.model_erode(sub, radius_sq))[m:-m, m:-m, m:-m]
    want = before.copy()
    want[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = want_box
    try:
        changed = getattr(scene, op)(lo, hi, radius_sq)
        after = scene.voxels()
        assert np.array_equal(after, want), f"{op} {lo} ... {hi} by {radius_sq}: {int((after != want).sum())} voxels differ from the model"
        assert changed == int((want != before).sum()), f"{op} by {radius_sq}: {changed} reported"
        assert np.array_equal(scene.read_region(lo, hi), want_box), "the device world follows"
    finally:
        scene.write_region(lo, before[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].view(np.uint8))
    assert np.array_equal(scene.voxels(), before)
    return changed


@pytest.mark.parametrize("radius_sq", [1, 2, 3, 9])
def test_grow_and_shrink_equal_the_numpy_morphology(radius_sq, bm, torch_cuda, scene):
    lo, hi = surface_box(scene)
    assert morph_check(scene, lo, hi, radius_sq, "grow") > 0
    assert morph_check(scene, lo, hi, radius_sq, "shrink") > 0


def test_grow_and_shrink_at_the_worlds_border(bm, torch_cuda, scene):
    """the margin is clipped: beyond the world's border counts as empty, so solid voxels at the border erode"""
    lo, hi = surface_box(scene, x0=0, y0=0)
    for radius_sq in (2, 9):
        assert morph_check(scene, lo, hi, radius_sq, "grow") > 0
        assert morph_check(scene, lo, hi, radius_sq, "shrink") > 0
    g = scene.grid_size
    lo, hi = surface_box(scene, x0=g - 24, y0=g - 24)
    assert morph_check(scene, lo, hi, 5, "shrink") > 0
    assert morph_check(scene, (0, 0, 0), (24, 24, 24), 4, "shrink") > 0, "the floor and two walls of the world"
    with pytest.raises(ValueError):
        scene.grow(lo, hi, 0)
    with pytest.raises(ValueError):
        scene.shrink(hi, lo, 1)


def test_grow_and_shrink_in_a_streaming_scene_that_is_not_preloaded(bm, torch_cuda):
    s = bm.Scene(128, 128, device=0).generate()
    try:
        lo, hi = surface_box(s)
        assert int(s.query_volumes(bm.volume_box(lo, hi)).unresolved[0]) > 0, "bricks of the box are absent"
        assert morph_check(s, lo, hi, 3, "grow") > 0
        assert morph_check(s, lo, hi, 3, "shrink") > 0
    finally:
        s.close()


def test_a_ray_straight_down_sees_the_grown_column(bm, torch_cuda, scene):
    lo, hi = surface_box(scene)
    before = scene.voxels().copy()
    ys, xs = np.mgrid[lo[1]:hi[1], lo[0]:hi[0]]
    origins = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5, np.full(xs.size, scene.grid_height - 0.25)], axis=1).astype(np.float32)
    directions = np.tile(np.array([1e-4, 1e-4, -1.0], np.float32), (xs.size, 1))

    def tops(world):
        columns = world[:, lo[1]:hi[1], lo[0]:hi[0]].reshape(world.shape[0], -1)
        return np.where(columns.any(axis=0), world.shape[0] - 1 - np.argmax(columns[::-1], axis=0), -1)

    hit_before = scene.cast_rays(origins, directions).voxel
    try:
        scene.grow(lo, hi, 1)
        hit_after = scene.cast_rays(origins, directions).voxel
        top_before, top_after = tops(before), tops(scene.voxels())
    finally:
        scene.write_region(lo, before[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].view(np.uint8))
    rose = top_after == top_before + 1
    assert rose.sum() > 100, "the terrain's columns inside the box rise by one"
    assert np.array_equal(hit_before[rose, 2], top_before[rose]) and np.array_equal(hit_after[rose, 2], top_before[rose] + 1)
    assert np.array_equal(hit_after[rose, :2], np.stack([xs.ravel(), ys.ravel()], axis=1)[rose])


def test_clearance_equals_the_model(bm, torch_cuda, scene):
    lo, hi = surface_box(scene)
    sub = box_of(scene.voxels(), lo, hi)
    want, rec = model.model_distance_field(sub.view(np.uint8))
    got = scene.clearance(lo, hi)
    assert got.field.cpu().numpy().tobytes() == want.tobytes() and got.record == rec
    at = int(rec["max_at"])
    assert got.largest() == ((at % 24, at // 24 % 24, at // 576), int(rec["max_sq"])) and int(rec["max_sq"]) > 9
    x, y, z = got.largest()[0]
    assert not sub[z, y, x], "the centre of the largest empty ball is empty"


# ---------------------------------------------------------------- the example
def test_headless_main_grows_and_shrinks(bm, torch_cuda, tmp_path):
    """examples/headless_main --grow x0,y0,z0:x1,y1,z1=r2 --shrink ...=r2 (C++ Scene::grow and Scene::shrink): the counts it prints and,
    through --mesh-out, the world it leaves equal the model's"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "headless_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    vox = np.zeros((128, 128, 128), np.uint8)
    vox[40:60, 30:47, 20:51] = random_volume(13, (20, 17, 31), 0.3)
    vox[0:6] = 1   # a floor, so that the shrink meets the world's border
    world = tmp_path / "world.raw"
    vox.tofile(world)
    mesh, out = tmp_path / "out.tri", tmp_path / "frame.ppm"
    g_lo, g_hi, s_lo, s_hi = (18, 28, 38), (50, 50, 62), (0, 0, 0), (40, 35, 12)
    r = subprocess.run([exe, "--voxels", str(world), "--grow", "18,28,38:50,50,62=5", "--shrink", "0,0,0:40,35,12=3", "--mesh-out", f"0,0,0:64,64,64={mesh}",
                        "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    solid = vox != 0
    grown = solid.copy()
    m = model.model_ball(5)[1]
    grown[g_lo[2]:g_hi[2], g_lo[1]:g_hi[1], g_lo[0]:g_hi[0]] = model.model_dilate(box_of(solid, g_lo, g_hi, m), 5)[m:-m, m:-m, m:-m]
    shrunk = grown.copy()
    m = model.model_ball(3)[1]
    shrunk[s_lo[2]:s_hi[2], s_lo[1]:s_hi[1], s_lo[0]:s_hi[0]] = model.model_erode(box_of(grown, s_lo, s_hi, m), 3)[m:-m, m:-m, m:-m]
    a, b = re.search(r"grew (\d+) voxels", r.stdout), re.search(r"shrank (\d+) voxels", r.stdout)
    assert a and b and (int(a.group(1)), int(b.group(1))) == (int((grown != solid).sum()), int((shrunk != grown).sum())) and int(a.group(1)) > 0 and int(b.group(1)) > 0, r.stdout
    quads, _ = bm.host_mesh_quads(shrunk[:64, :64, :64].view(np.uint8))
    assert np.fromfile(mesh, np.float32).tobytes() == bm.host_mesh_triangles(quads).tobytes()
    r = subprocess.run([exe, "--voxels", str(world), "--grow", "1,2,3:4,5,6=0", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--grow wants" in r.stderr
