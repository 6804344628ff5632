"""bm_host_travel_field and bm_host_travel_paths (csrc/travel_host.cpp: plain loops over the rules of csrc/travel.h) against the numpy model
of the travel-field contract (tests/_travel_model.py: a level-by-level search by shifting), byte for byte; where scipy imports, the reached
count against the size of the seed's component -- CPU only.  And tests/travel_check.cpp, a program with its own main that links the host
routine alone and runs the kernels' in-tile sweeps and round scheme lane by lane, built plain and under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _travel_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
NONE = model.NONE
SHAPES = [(1, 1, 1), (1, 1, 9), (5, 1, 1), (1, 7, 1), (3, 4, 5), (9, 10, 11), (7, 13, 6), (16, 16, 16)]
LIMITS = [0, 1, 7, 8, 9]


def random_volume(seed, shape, density, byte=1):
    return ((np.random.default_rng(seed).random(shape) < density) * byte).astype(np.uint8)


def random_points(seed, shape, n, margin=0):
    """n points (x, y, z), with margin > 0 some of them outside the volume"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    return np.stack([rng.integers(-margin, nx + margin, n), rng.integers(-margin, ny + margin, n), rng.integers(-margin, nz + margin, n)], axis=1).astype(np.int32)


def both(bm, vol, seeds, max_steps=0):
    want, rec = model.model_travel_field(vol, seeds, max_steps)
    got, r = bm.host_travel_field(vol, seeds, max_steps)
    assert got.dtype == np.int32 and got.shape == vol.shape
    assert got.tobytes() == want.tobytes(), f"{vol.shape} limit {max_steps}: first difference at {np.argmax(got.ravel() != want.ravel())}"
    assert r == rec, (r, rec)
    return got, r


# ---------------------------------------------------------------- the host routine against the model
@pytest.mark.parametrize("density", [0, 1, 0.2, 0.3])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_equals_the_model(bm, shape, density):
    """shapes are (nz, ny, nx); blocked bytes 2, 128 and 255; every limit; seeds inside and outside, open and blocked, and twice"""
    for k, byte in enumerate((2, 128, 255)):
        vol = random_volume(20 + k, shape, density, byte)
        seeds = random_points(30 + k, shape, 3, margin=1)
        seeds = np.concatenate([seeds, seeds[:1]])
        for limit in LIMITS:
            got, rec = both(bm, vol, seeds, limit)
            assert (got >= 0).all() and (got[vol != 0] == NONE).all()
            finite = got[got != NONE]
            assert int(rec["reached"]) == finite.size and (limit == 0 or (finite <= limit).all())


def test_no_seed_rejected_seeds_and_duplicates(bm):
    vol = np.zeros((5, 6, 7), np.uint8)
    vol[2, 3, 4] = 9
    for seeds, rejected in (([], 0), (np.zeros((0, 3), np.int32), 0), ([(-1, 0, 0), (7, 0, 0), (0, 6, 0), (0, 0, 5), (4, 3, 2)], 5)):
        got, rec = both(bm, vol, seeds)
        assert (got == NONE).all() and (int(rec["reached"]), int(rec["farthest"]), int(rec["seeds_rejected"]), int(rec["farthest_at"])) == (0, NONE, rejected, 0)
    got, rec = both(bm, vol, [(1, 1, 1), (1, 1, 1), (1, 1, 1), (9, 9, 9)])
    one, rec1 = both(bm, vol, [(1, 1, 1)])
    assert got.tobytes() == one.tobytes() and int(rec["seeds_rejected"]) == 1 and int(rec1["seeds_rejected"]) == 0 and int(rec["reached"]) == 5 * 6 * 7 - 1
    z, y, x = np.indices(vol.shape)
    manhattan = abs(z - 1) + abs(y - 1) + abs(x - 1)
    assert (got[vol == 0] == manhattan[vol == 0]).all(), "one blocked voxel in the open lengthens no path here"
    got, rec = both(bm, np.ones((3, 3, 3), np.uint8), [(1, 1, 1)])
    assert (got == NONE).all() and int(rec["seeds_rejected"]) == 1


def test_the_record_and_its_tie(bm):
    row = np.zeros((1, 1, 11), np.uint8)
    got, rec = both(bm, row, [(5, 0, 0)])
    assert got[0, 0, 0] == got[0, 0, 10] == 5 and (int(rec["farthest"]), int(rec["farthest_at"]), int(rec["reached"])) == (5, 0, 11), "both ends: the lower index"
    vol = np.zeros((7, 3, 3), np.uint8)
    got, rec = both(bm, vol, [(1, 1, 3)])
    assert got.ravel()[0] == got.ravel()[-1] == 5 and (int(rec["farthest"]), int(rec["farthest_at"])) == (5, 0)
    got, rec = both(bm, vol, [(1, 1, 3)], max_steps=2)
    assert int(rec["farthest"]) == 2 and int(rec["farthest_at"]) == int(np.flatnonzero(got.ravel() == 2)[0]) and int(rec["reached"]) == 1 + 6 + 14
    got, rec = both(bm, vol, [(0, 0, 0)])
    assert (int(rec["farthest"]), int(rec["farthest_at"])) == (10, 62) and got[6, 2, 2] == 10


def test_a_closed_pocket_and_a_wall(bm):
    vol = np.zeros((9, 9, 9), np.uint8)
    vol[3:6, 3:6, 3:6] = 1
    vol[4, 4, 4] = 0
    got, rec = both(bm, vol, [(4, 4, 4)])
    assert int(rec["reached"]) == 1 and got[4, 4, 4] == 0
    got, rec = both(bm, vol, [(0, 0, 0)])
    assert got[4, 4, 4] == NONE and int(rec["reached"]) == 9 ** 3 - 27
    wall = np.zeros((4, 12, 12), np.uint8)
    wall[:, 6, :11] = 200
    got, rec = both(bm, wall, [(0, 0, 0)])
    assert got[0, 7, 0] == 11 + 7 + 11, "round the far end of the wall"


def test_a_slice_of_a_larger_array(bm):
    big = random_volume(5, (12, 14, 40), 0.25, 7)
    view = big[1:11, 2:13, 3:36]
    assert not view.flags["C_CONTIGUOUS"]
    seeds = random_points(6, view.shape, 4)
    for limit in (0, 9):
        got, rec = both(bm, view, seeds, limit)
        tight, rec2 = bm.host_travel_field(np.ascontiguousarray(view), seeds, limit)
        assert got.tobytes() == tight.tobytes() and rec == rec2
    assert bm.host_travel_field(view.astype(bool), seeds)[0].tobytes() == bm.host_travel_field(view, seeds)[0].tobytes()


def test_reached_is_the_seeds_component_where_scipy_imports(bm):
    ndimage = pytest.importorskip("scipy.ndimage")
    vol = random_volume(8, (33, 40, 65), 0.4)
    labels, _ = ndimage.label(vol == 0)
    for x, y, z in random_points(9, vol.shape, 8):
        got, rec = bm.host_travel_field(vol, [(x, y, z)])
        want = int((labels == labels[z, y, x]).sum()) if labels[z, y, x] else 0
        assert int(rec["reached"]) == want and ((got != NONE) == ((labels == labels[z, y, x]) & (labels != 0))).all()


# ---------------------------------------------------------------- paths
def paths_both(bm, field, starts, capacity):
    want, want_len = model.model_travel_paths(field, starts, capacity)
    got, got_len = bm.host_travel_paths(field, starts, capacity)
    assert got.dtype == np.int32 and got.shape == want.shape and got_len.tobytes() == want_len.tobytes(), (got_len, want_len)
    assert got.tobytes() == want.tobytes()
    return got, got_len


def test_paths_against_the_model(bm):
    vol = random_volume(11, (9, 10, 11), 0.25)
    z, y, x = np.argwhere(vol == 0)[0]
    field, rec = bm.host_travel_field(vol, [(x, y, z), (10, 9, 8)])
    assert int(rec["reached"]) > vol.size // 2
    starts = np.concatenate([random_points(12, vol.shape, 60, margin=1), [(x, y, z)]])
    for capacity in (1, 2, 8, 40):
        path, lengths = paths_both(bm, field, starts, capacity)
        for q in np.flatnonzero((lengths > 0) & (lengths <= capacity)):
            model.check_full_path(vol, field, path[q, :lengths[q]])
    assert (lengths == 0).any() and (lengths > 1).any()


def test_the_neighbour_order_at_a_tie(bm):
    field, _ = bm.host_travel_field(np.zeros((3, 3, 3), np.uint8), [(1, 1, 1)])
    path, lengths = paths_both(bm, field, [(0, 0, 0), (2, 2, 2), (2, 0, 1)], 4)
    assert lengths.tolist() == [4, 4, 3]
    assert path[0].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], "+x before +y before +z"
    assert path[1].tolist() == [[2, 2, 2], [1, 2, 2], [1, 1, 2], [1, 1, 1]], "-x before -y before -z"
    assert path[2].tolist() == [[2, 0, 1], [1, 0, 1], [1, 1, 1], [-1, -1, -1]], "-x before +y"


def test_truncation_a_start_on_none_and_a_malformed_field(bm):
    vol = np.zeros((1, 1, 9), np.uint8)
    vol[0, 0, 7] = 1
    field, _ = bm.host_travel_field(vol, [(0, 0, 0)])
    path, lengths = paths_both(bm, field, [(6, 0, 0), (7, 0, 0), (8, 0, 0), (9, 0, 0), (0, 0, 0)], 3)
    assert lengths.tolist() == [7, 0, 0, 0, 1] and path[0].tolist() == [[6, 0, 0], [5, 0, 0], [4, 0, 0]] and (path[1:4] == -1).all()
    assert path[4].tolist() == [[0, 0, 0], [-1, -1, -1], [-1, -1, -1]]
    bad = field.copy()
    bad[0, 0, 3] = 9   # 6 5 4 9 2 1 0: the walk from 6 finds no 3
    path, lengths = paths_both(bm, bad, [(6, 0, 0), (2, 0, 0)], 9)
    assert lengths.tolist() == [-1, 3] and path[0, :3].tolist() == [[6, 0, 0], [5, 0, 0], [4, 0, 0]]
    assert bm.host_travel_paths(bad.view(np.uint32), [(2, 0, 0)], 9)[1].tolist() == [3]
    assert bm.host_travel_paths(field, [], 4)[0].shape == (0, 4, 3)


# ---------------------------------------------------------------- refusals
def test_every_refusal(bm):
    from brickmap_amd import _lib
    L = bm.load()
    vol = np.zeros((8, 8, 8), np.uint8)
    field = np.full((8, 8, 8), -7, np.int32)
    seeds = np.zeros((2, 3), np.int32)
    res = _lib.bm_travel_result(77, 77, 77, 77, 77)

    def call(extent=(8, 8, 8), row=0, sl=0, flags=0, reserved=0, v=vol.ctypes.data, s=seeds.ctypes.data, n=2, f=field.ctypes.data, r=C.byref(res)):
        par = _lib.bm_travel_params()
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.flags, par.reserved = row, sl, flags, reserved
        return L.bm_host_travel_field(C.byref(par), C.c_void_p(v), C.c_void_p(s), n, C.c_void_p(f), r)

    for kw in (dict(extent=(0, 8, 8)), dict(extent=(8, -1, 8)), dict(extent=(8, 8, 16385)), dict(extent=(16384, 16384, 8)), dict(row=7), dict(row=-8), dict(sl=63), dict(sl=-1),
               dict(flags=1), dict(flags=0x80000000), dict(reserved=1), dict(v=0), dict(f=0), dict(r=None), dict(s=0), dict(n=-1)):
        assert call(**kw) == EINVAL, kw
        assert (field == -7).all() and (res.reached, res.farthest, res.seeds_rejected, res.farthest_at, res.reserved) == (77, 77, 77, 77, 77), "nothing is written"
    assert L.bm_host_travel_field(None, C.c_void_p(vol.ctypes.data), C.c_void_p(seeds.ctypes.data), 2, C.c_void_p(field.ctypes.data), C.byref(res)) == EINVAL
    assert call(s=0, n=0) == 0 and (field == NONE).all() and (res.reached, res.farthest, res.seeds_rejected, res.farthest_at, res.reserved) == (0, NONE, 0, 0, 0)
    assert call(row=8, sl=64) == 0 and (res.reached, res.farthest, res.seeds_rejected, res.farthest_at, res.reserved) == (512, 21, 0, 511, 0)

    path, lengths = np.full((2, 4, 3), -5, np.int32), np.full(2, -5, np.int32)

    def walk(extent=(8, 8, 8), f=field.ctypes.data, s=seeds.ctypes.data, n=2, capacity=4, p=path.ctypes.data, l=lengths.ctypes.data):
        return L.bm_host_travel_paths((C.c_int32 * 3)(*extent) if extent else None, C.c_void_p(f), C.c_void_p(s), n, capacity, C.c_void_p(p), C.c_void_p(l))

    for kw in (dict(extent=None), dict(extent=(0, 8, 8)), dict(extent=(8, 8, 16385)), dict(extent=(16384, 16384, 8)), dict(f=0), dict(s=0), dict(p=0), dict(l=0), dict(n=-1),
               dict(capacity=0), dict(capacity=-3)):
        assert walk(**kw) == EINVAL, kw
        assert (path == -5).all() and (lengths == -5).all(), "nothing is written"
    assert walk(s=0, p=0, l=0, n=0) == 0 and walk() == 0 and lengths.tolist() == [1, 1]

    size = C.c_size_t(0)
    par = _lib.bm_travel_params()
    assert L.bm_travel_workspace_bytes(C.byref(par), C.byref(size)) == EINVAL, "extents of 0"
    par.extent[:] = [8, 8, 8]
    assert L.bm_travel_workspace_bytes(C.byref(par), None) == EINVAL and L.bm_travel_workspace_bytes(None, C.byref(size)) == EINVAL
    par.flags = 2
    assert L.bm_travel_workspace_bytes(C.byref(par), C.byref(size)) == EINVAL
    assert bm.travel_workspace_bytes((8, 8, 8)) == 64 + 3 * 16 + 64, "one tile: its brick, a stamp and two list entries each rounded up to 16, and the tail"
    assert bm.travel_workspace_bytes((9, 8, 8)) == 2 * 64 + 3 * 16 + 64 and bm.travel_workspace_bytes((17, 17, 17)) == 27 * 64 + 3 * 112 + 64
    assert bm.travel_workspace_bytes((7, 16384, 16384)) == (1 << 22) * 64 + 3 * (1 << 24) + 64
    with pytest.raises(ValueError):
        bm.host_travel_field(np.zeros((8, 8, 8), np.int32), [])
    with pytest.raises(ValueError):
        bm.host_travel_field(vol, [(1, 2)])
    with pytest.raises(ValueError):
        bm.host_travel_field(vol, [(0.5, 0, 0)])
    with pytest.raises(ValueError):
        bm.host_travel_field(vol, [], max_steps=-1)
    with pytest.raises(ValueError):
        bm.host_travel_paths(np.zeros((2, 2, 2), np.float32), [], 1)
    assert bm.TRAVEL_NONE == NONE == bm.BM_TRAVEL_NONE and bm.TRAVEL_RESULT_DTYPE == model.RESULT_DTYPE and bm.TRAVEL_RESULT_DTYPE.itemsize == 32
    assert C.sizeof(_lib.bm_travel_params) == 40 and C.sizeof(_lib.bm_travel_result) == 32


# ---------------------------------------------------------------- the stand-alone program: the host routine linked alone
SRCS = [os.path.join(ROOT, "tests", "travel_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "travel_host.cpp")]
WANT = {"rows": 4096, "snake": 3, "tiles": 10000, "volumes": 40, "refused": 16, "failures": 0}


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def _check(n):
    assert {k: n[k] for k in WANT} == WANT, n
    assert 0 < n["most_sweeps"] < 512, "the in-tile sweeps stay below their bound"
    assert n["rounds_over"] == 0, "no volume needed more rounds than farthest + 2"


def test_travel_check_program(tmp_path):
    exe = tmp_path / "travel_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe)] + SRCS)
    _check(_run(exe))


def test_travel_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "travel_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + SRCS)
    _check(_run(exe))
