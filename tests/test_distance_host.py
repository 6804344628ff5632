"""bm_host_distance_field and bm_host_distance_mask (csrc/distance_host.cpp: plain loops over the rules of csrc/distance.h) against the numpy
model of the distance-field contract (tests/_distance_model.py: a brute-force minimum over all sources), byte for byte; where scipy
imports, against its Euclidean transform as well -- CPU only.  And tests/distance_check.cpp, a program with its own main that links the
host routine alone, built plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _distance_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
NONE = model.NONE
SHAPES = [(1, 1, 1), (1, 1, 9), (5, 1, 1), (1, 7, 1), (3, 4, 5), (9, 10, 11), (7, 13, 6), (16, 16, 16)]


def random_volume(seed, shape, density, byte=1):
    return ((np.random.default_rng(seed).random(shape) < density) * byte).astype(np.uint8)


def both(bm, vol, to="solid", outside=False):
    want, rec = model.model_distance_field(vol, to, outside)
    got, r = bm.host_distance_field(vol, to, outside)
    assert got.dtype == np.int32 and got.shape == vol.shape
    assert got.tobytes() == want.tobytes(), f"{vol.shape} to {to} outside {outside}: first difference at {np.argmax(got.ravel() != want.ravel())}"
    assert r == rec, (r, rec)
    return got, r


# ---------------------------------------------------------------- the host routine against the model
@pytest.mark.parametrize("density", [0, 1, 0.02, 0.3])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_equals_the_model(bm, shape, density):
    """shapes are (nz, ny, nx); both flags on and off; solid bytes 2, 128 and 255"""
    for k, byte in enumerate((2, 128, 255)):
        vol = random_volume(10 + k, shape, density, byte)
        for to in ("solid", "empty"):
            for outside in (False, True):
                got, rec = both(bm, vol, to, outside)
                assert (got >= 0).all() and int(rec["sources"]) == int(model.model_sources(vol, to).sum())
                assert ((got == 0) == model.model_sources(vol, to)).all(), "a source, and only a source, has D = 0"


def test_no_source_and_all_sources(bm):
    got, rec = both(bm, np.zeros((5, 6, 7), np.uint8))
    assert (got == NONE).all() and (int(rec["sources"]), int(rec["max_sq"]), int(rec["max_at"])) == (0, NONE, 0)
    got, rec = both(bm, np.zeros((5, 6, 7), np.uint8), outside=True)
    assert (int(rec["sources"]), int(rec["max_sq"])) == (0, 9) and int(rec["max_at"]) == (2 * 6 + 2) * 7 + 2, "the volume's border is all there is"
    got, rec = both(bm, np.ones((5, 6, 7), np.uint8))
    assert not got.any() and (int(rec["sources"]), int(rec["max_sq"]), int(rec["max_at"])) == (210, 0, 0)
    got, rec = both(bm, np.ones((5, 6, 7), np.uint8), to="empty")
    assert (got == NONE).all() and (int(rec["sources"]), int(rec["max_sq"]), int(rec["max_at"])) == (0, NONE, 0)


@pytest.mark.parametrize("at", [(0, 0, 0), (19, 19, 19), (10, 10, 10), (0, 19, 7)])
def test_a_single_source_in_20_cubed(bm, at):
    vol = np.zeros((20, 20, 20), np.uint8)
    vol[at] = 255
    got, rec = both(bm, vol)
    z, y, x = np.indices(vol.shape)
    assert np.array_equal(got, (z - at[0]) ** 2 + (y - at[1]) ** 2 + (x - at[2]) ** 2)
    both(bm, vol, outside=True)
    both(bm, vol, to="empty")


def test_two_symmetric_sources_the_tie_goes_to_the_lower_index(bm):
    vol = np.zeros((9, 9, 9), np.uint8)
    vol[4, 4, 2] = vol[4, 4, 6] = 1
    got, rec = both(bm, vol)
    far = np.flatnonzero(got.ravel() == got.max())
    assert len(far) == 12 and int(rec["max_at"]) == far[0] == 0 and int(rec["max_sq"]) == 16 + 16 + 4
    # in a row: both ends are as far as it gets
    row = np.zeros((1, 1, 11), np.uint8)
    row[0, 0, 5] = 1
    got, rec = both(bm, row)
    assert got[0, 0, 0] == got[0, 0, 10] == 25 and (int(rec["max_sq"]), int(rec["max_at"])) == (25, 0)
    # ... and mirrored along z only, where the key has to beat a higher index with the same value
    vol = np.zeros((7, 3, 3), np.uint8)
    vol[3, 1, 1] = 1
    got, rec = both(bm, vol)
    assert int(rec["max_at"]) == 0 and got.ravel()[0] == got.ravel()[-1] == int(rec["max_sq"]) == 11


def test_a_slice_of_a_larger_array(bm):
    big = random_volume(5, (12, 14, 40), 0.1, 7)
    view = big[1:11, 2:13, 3:36]
    assert not view.flags["C_CONTIGUOUS"]
    for to in ("solid", "empty"):
        for outside in (False, True):
            got, rec = both(bm, view, to, outside)
            tight, rec2 = bm.host_distance_field(np.ascontiguousarray(view), to, outside)
            assert got.tobytes() == tight.tobytes() and rec == rec2
    assert bm.host_distance_field(view.astype(bool))[0].tobytes() == bm.host_distance_field(view)[0].tobytes()


def test_against_scipy_where_it_imports(bm):
    ndimage = pytest.importorskip("scipy.ndimage")
    src = np.random.default_rng(6).random((33, 40, 65)) < 0.01
    got, _ = bm.host_distance_field(src.astype(np.uint8))
    want = np.rint(ndimage.distance_transform_edt(~src) ** 2).astype(np.int64)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- the mask
@pytest.mark.parametrize("above", [False, True])
@pytest.mark.parametrize("limit", [0, 1, 2, NONE - 1])
def test_mask(bm, limit, above):
    vol = random_volume(7, (7, 9, 11), 0.05)
    vol[3] = 0   # and a slab that is far from everything
    for field in (bm.host_distance_field(vol)[0], bm.host_distance_field(np.zeros((2, 3, 5), np.uint8))[0]):
        got = bm.host_distance_mask(field, limit, above)
        assert got.dtype == np.uint8 and got.shape == field.shape and got.tobytes() == model.model_mask(field, limit, above).tobytes()
        assert set(np.unique(got)) <= {0, 1}
    none = np.full(5, NONE, np.int32)
    assert not bm.host_distance_mask(none, 0xFFFFFFFF).any() and bm.host_distance_mask(none, 0xFFFFFFFF, True).all(), "none is above every limit"


# ---------------------------------------------------------------- refusals
def test_every_refusal(bm):
    from brickmap_amd import _lib
    L = bm.load()
    vol = np.ones((8, 8, 8), np.uint8)
    field = np.full((8, 8, 8), -7, np.int32)
    res = _lib.bm_distance_result(77, 77, 77, 77, 77)

    def call(extent=(8, 8, 8), row=0, sl=0, flags=0, reserved=0, v=vol.ctypes.data, f=field.ctypes.data, r=C.byref(res)):
        par = _lib.bm_distance_params()
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.flags, par.reserved = row, sl, flags, reserved
        return L.bm_host_distance_field(C.byref(par), C.c_void_p(v), C.c_void_p(f), r)

    for kw in (dict(extent=(0, 8, 8)), dict(extent=(8, -1, 8)), dict(extent=(8, 8, 16385)), dict(extent=(16384, 16384, 8)), dict(row=7), dict(row=-8), dict(sl=63), dict(sl=-1),
               dict(flags=4), dict(flags=0x80000001), dict(reserved=1), dict(v=0), dict(f=0), dict(r=None)):
        assert call(**kw) == EINVAL, kw
        assert (field == -7).all() and (res.sources, res.max_sq, res.max_at, res.reserved1) == (77, 77, 77, 77), "nothing is written"
    assert L.bm_host_distance_field(None, C.c_void_p(vol.ctypes.data), C.c_void_p(field.ctypes.data), C.byref(res)) == EINVAL
    assert call(row=8, sl=64) == 0 and not field.any() and (res.sources, res.max_sq, res.reserved0, res.max_at, res.reserved1) == (512, 0, 0, 0, 0)
    out = np.full(8, 9, np.uint8)
    for args in ((0, field.ctypes.data, 1, 0, out.ctypes.data), ((1 << 31) - 1, field.ctypes.data, 1, 0, out.ctypes.data), (8, field.ctypes.data, 1, 2, out.ctypes.data),
                 (8, 0, 1, 0, out.ctypes.data), (8, field.ctypes.data, 1, 0, 0)):
        assert L.bm_host_distance_mask(args[0], C.c_void_p(args[1]), args[2], args[3], C.c_void_p(args[4])) == EINVAL, args
        assert (out == 9).all()
    size = C.c_size_t(0)
    par = _lib.bm_distance_params()
    assert L.bm_distance_workspace_bytes(C.byref(par), C.byref(size)) == EINVAL, "extents of 0"
    par.extent[:] = [8, 8, 8]
    assert L.bm_distance_workspace_bytes(C.byref(par), None) == EINVAL and L.bm_distance_workspace_bytes(None, C.byref(size)) == EINVAL
    assert bm.distance_workspace_bytes((8, 8, 8)) == 2048 + 2048 + 32, "4 bytes per voxel twice and the tail"
    assert bm.distance_workspace_bytes((1, 1, 1)) == 16 + 16 + 32, "each part rounded up to 16"
    assert bm.distance_workspace_bytes((3, 3, 3)) == 112 + 112 + 32 and bm.distance_workspace_bytes((40, 80, 80)) == 2 * 1024000 + 32
    assert bm.distance_workspace_bytes((16384, 16384, 7)) == 2 * 4 * 7 * (1 << 28) + 32
    with pytest.raises(ValueError):
        bm.host_distance_field(np.ones((8, 8, 8), np.int32))
    with pytest.raises(ValueError):
        bm.host_distance_field(vol, to="nowhere")
    with pytest.raises(ValueError):
        bm.host_distance_mask(np.zeros(4, np.float32), 1)
    assert bm.DISTANCE_NONE == NONE == bm.BM_DISTANCE_NONE and bm.DISTANCE_RESULT_DTYPE == model.RESULT_DTYPE and bm.DISTANCE_RESULT_DTYPE.itemsize == 32
    assert C.sizeof(_lib.bm_distance_params) == 40 and C.sizeof(_lib.bm_distance_result) == 32


# ---------------------------------------------------------------- the stand-alone program: the host routine linked alone
SRCS = [os.path.join(ROOT, "tests", "distance_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "distance_host.cpp")]


def _run(exe, rounds):
    r = subprocess.run([str(exe), str(rounds)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_distance_check_program(tmp_path):
    exe = tmp_path / "distance_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe)] + SRCS)
    n = _run(exe, 100000)
    assert n["patterns"] == 4096 and n["lines"] == 100000 and n["short"] == 5 ** 2 + 5 ** 3 and n["volumes"] >= 40 and n["refused"] == 14


def test_distance_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "distance_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + SRCS)
    n = _run(exe, 100000)
    assert n["patterns"] == 4096 and n["lines"] == 100000 and n["refused"] == 14
