"""bm_host_voxelize (csrc/voxelize_host.cpp: plain loops over the rules of csrc/voxelize.h) against the numpy model of the voxelization
contract (tests/_voxelize_model.py), byte for byte, and the model against what the rules are meant to compute: exact clipping of the
triangle against the voxel's cube for the surface rule; for the solid rule, parity along x equal to parity along y and z wherever no
surface voxel lies, and an integer box equal to the voxels whose centres lie inside -- CPU only.  And tests/voxelize_check.cpp, a
program with its own main that links the host routine alone, built plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _voxelize_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
MODES = {"surface": 1, "solid": 2, "solid+surface": 3}


def both(bm, tri, lo, shape, mode="solid+surface"):
    want, rec = model.model_voxelize(tri, lo, shape, MODES[mode])
    got, r = bm.host_voxelize(tri, lo, shape, mode=mode)
    assert got.dtype == np.uint8 and got.shape == tuple(shape)
    assert np.array_equal(got, want), f"{mode} {lo} {shape}: {np.count_nonzero(got != want)} bytes differ"
    assert r == rec, (r, rec)
    return got, r


# ---------------------------------------------------------------- the host routine against the model
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", range(4))
def test_random_quarter_voxel_triangles(bm, seed, mode):
    """coordinates in quarter voxels: vertices, edges and faces land on voxel faces and centres all the time"""
    tri = model.quarter_triangles(seed, 24, -3, 15)
    got, _ = both(bm, tri, (0, 0, 0), (9, 11, 13), mode)
    assert got.any()
    both(bm, tri, (-2, 3, 1), (12, 7, 10), mode)


@pytest.mark.parametrize("center", [(16.5, 16.5, 16.5), (16.0, 16.0, 16.0), (16.3, 15.9, 16.2)])
def test_icospheres_on_and_off_voxel_centres(bm, center):
    for sub in (1, 2):
        tri = model.icosphere(center, 12.3, sub)
        for mode in MODES:
            got, r = both(bm, tri, (0, 0, 0), (33, 32, 31), mode)
            assert r["open_columns"] == 0
    # the solid sphere is a ball: within half a voxel diagonal of the radius
    solid, _ = bm.host_voxelize(model.icosphere(center, 12.3, 3), (0, 0, 0), (33, 32, 31), mode="solid")
    z, y, x = np.nonzero(solid)
    d = np.sqrt((x + 0.5 - center[0]) ** 2 + (y + 0.5 - center[1]) ** 2 + (z + 0.5 - center[2]) ** 2)
    assert d.max() <= 12.3 and abs(solid.sum() / (4 / 3 * np.pi * 12.3 ** 3) - 1) < 0.03


@pytest.mark.parametrize("lo,hi", [((3, 4, 5), (20, 21, 22)), ((3.5, 4.5, 5.5), (20.5, 21.5, 22.5)), ((-5, -6, -7), (50, 50, 50)), ((10, -3, 8), (12.25, 60, 9))])
def test_boxes_at_integer_and_half_integer_corners_and_sticking_out(bm, lo, hi):
    tri = model.box_mesh(lo, hi)
    for mode in MODES:
        got, r = both(bm, tri, (0, 0, 0), (24, 28, 33), mode)
        assert r["open_columns"] == 0, "crossings beyond either end of a row still pair up"
    # the solid voxels are those whose centre lies inside (a centre on a face: the low face counts, the high one does not)
    solid, _ = bm.host_voxelize(tri, (0, 0, 0), (24, 28, 33), mode="solid")
    c = [np.arange(n) + 0.5 for n in (33, 28, 24)]
    inside = [(ck >= l) & (ck < h) for ck, l, h in zip(c, lo, hi)]
    assert np.array_equal(solid.astype(bool), inside[2][:, None, None] & inside[1][None, :, None] & inside[0][None, None, :])


def test_torus_and_a_moved_origin(bm):
    tri = model.torus((16, 16, 8), 10, 4)
    a, r = both(bm, tri, (0, 0, 0), (17, 33, 40))
    assert r["open_columns"] == 0 and not a[8, 16, 16], "the hole of the torus stays empty"
    b, _ = both(bm, tri, (-3, 5, 2), (15, 20, 30))
    assert np.array_equal(b[:, :, 3:], a[2:17, 5:25, :27]), "the same voxels, seen from another origin"


def test_a_slice_of_a_larger_array_and_keep(bm):
    rng = np.random.default_rng(2)
    big = np.where(rng.random((12, 14, 40)) < 0.1, rng.integers(1, 256, size=(12, 14, 40)), 0).astype(np.uint8)
    tri = model.icosphere((12.2, 5.1, 4.8), 4.4, 2)
    for keep in (False, True):
        arr = big.copy()
        view = arr[1:11, 2:13, 3:36]
        old = view.copy()
        out, rec = bm.host_voxelize(tri, (0, 0, 0), out=view, keep=keep)
        want, wrec = model.model_voxelize(tri, (0, 0, 0), view.shape, 3, keep, old)
        assert np.array_equal(view, want) and rec == wrec
        mask = np.ones(big.shape, bool)
        mask[1:11, 2:13, 3:36] = False
        assert np.array_equal(arr[mask], big[mask]), "the bytes around the volume stay"
        assert ((view[old > 0] > 0).all() and (view & 0xFE == old & 0xFE).all()) if keep else view.max() == 1


def test_rejected_and_degenerate_triangles_are_counted_and_change_nothing(bm):
    good = model.box_mesh((2, 2, 2), (7, 8, 9))
    base, _ = bm.host_voxelize(good, (0, 0, 0), (12, 12, 12))
    bad = np.array([[[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [-np.inf, 0, 0], [0, 1, 0]], [[4194305.0, 0, 0], [1, 0, 0], [0, 1, 0]],  # NaN, infinite, |v 256| > 2^30
                    [[16385, 0, 0], [16384.5, 1, 0], [16384.5, 0, 1]],    # |q| > 2^22
                    [[0, 0, 0], [2048.25, 0, 0], [0, 1, 0]],              # longer than 2048 voxels
                    [[3e38, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)    # the product overflows
    flat = np.array([[[1, 1, 1], [2, 2, 2], [3, 3, 3]], [[4, 4, 4], [4, 4, 4], [9, 1, 1]], [[5, 5, 5], [5, 5, 5], [5, 5, 5]],
                     [[1.001, 1, 1], [1.0, 1, 1], [1, 1.001, 1]]], np.float32)   # collinear, two equal vertices, a point, and one that snaps to a point
    got, r = both(bm, np.concatenate((bad, good, flat)), (0, 0, 0), (12, 12, 12))
    assert r["rejected"] == len(bad) and r["degenerate"] == len(flat) and np.array_equal(got, base)
    got, r = both(bm, bad, (0, 0, 0), (5, 5, 5))
    assert not got.any() and r["rejected"] == len(bad)
    # the snap is about the volume's origin: the same far triangle is fine from a volume next to it
    far = np.array([[[16385, 0, 0], [16384.5, 1, 0], [16384.5, 0, 1]]], np.float32)
    got, r = both(bm, far, (16380, 0, 0), (4, 4, 8), "surface")
    assert r["rejected"] == 0 and got.any()


def test_an_open_mesh_is_reported(bm):
    tri = model.open_hemisphere((16, 16, 16), 12, 2)
    got, r = both(bm, tri, (0, 0, 0), (32, 32, 32), "solid")
    assert r["open_columns"] > 100
    _, r = both(bm, tri, (0, 0, 0), (32, 32, 32), "surface")
    assert r["open_columns"] == 0, "surface alone counts no crossings"


def test_every_refusal(bm):
    from brickmap_amd import _lib
    L = bm.load()
    tri = np.ascontiguousarray(model.box_mesh((1, 1, 1), (5, 5, 5)))
    vol = np.full((8, 8, 8), 7, np.uint8)

    def call(extent=(8, 8, 8), row=0, sl=0, mode=3, flags=0, n=len(tri), t=tri.ctypes.data, v=vol.ctypes.data):
        par = _lib.bm_voxelize_params()
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.mode, par.flags = row, sl, mode, flags
        return L.bm_host_voxelize(C.byref(par), n, C.c_void_p(t), C.c_void_p(v), None)

    for kw in (dict(extent=(0, 8, 8)), dict(extent=(8, -1, 8)), dict(extent=(8, 8, 16385)), dict(row=7), dict(row=-8), dict(sl=63), dict(sl=-1), dict(mode=0),
               dict(mode=4), dict(mode=7), dict(flags=2), dict(flags=0x80000001), dict(n=-1), dict(n=(1 << 30) + 1), dict(t=0), dict(v=0)):
        assert call(**kw) == EINVAL, kw
        assert (vol == 7).all()
    assert L.bm_host_voxelize(None, 0, None, C.c_void_p(vol.ctypes.data), None) == EINVAL
    size = C.c_size_t(0)
    par = _lib.bm_voxelize_params()
    assert L.bm_voxelize_workspace_bytes(C.byref(par), 1, C.byref(size)) == EINVAL, "extents of 0"
    assert bm.voxelize_workspace_bytes((8, 8, 33), 300) == 2 * 8 * 8 * 2 * 4 + (2 * 300 + 2 * 3) * 8
    assert call(row=8, sl=64) == 0 and call(n=0, t=0) == 0 and not vol.any()
    with pytest.raises(ValueError):
        bm.host_voxelize(tri, (0, 0, 0), (8, 8, 8), mode="hollow")
    assert bm.VOXELIZE_RESULT_DTYPE == model.RESULT_DTYPE and bm.VOXELIZE_RESULT_DTYPE.itemsize == 16


# ---------------------------------------------------------------- the model against what the rules are meant to compute
@pytest.mark.parametrize("seed", range(6))
def test_surface_rule_equals_exact_clipping(seed):
    """random quarter-voxel triangles (every second one with vertices on the voxel grid) against Sutherland-Hodgman in rationals"""
    tri = model.quarter_triangles(100 + seed, 5, -2, 8)
    if seed % 2:
        tri = np.round(tri)
    shape = (5, 6, 6)
    want = model.clipping_truth(tri, (0, 0, 0), shape)
    got, _ = model.model_voxelize(tri, (0, 0, 0), shape, model.SURFACE)
    assert np.array_equal(got, want), np.argwhere(got != want)
    assert want.any()


@pytest.mark.parametrize("center", [(10.0, 10.5, 10.0), (10.3, 9.9, 10.2)])
def test_parity_along_x_equals_parity_along_y_and_z_off_the_surface(center):
    for tri in (model.icosphere(center, 7.7, 2), model.torus(center, 6.0, 2.5, 16, 10)):
        q, rejected = model.snap(tri, (0, 0, 0))
        assert not rejected.any()
        extent = (21, 20, 22)
        x, ox = model.solid_volume(list(q), extent, 0)
        y, oy = model.solid_volume(list(q), extent, 1)
        z, oz = model.solid_volume(list(q), extent, 2)
        surface, _ = model.model_voxelize(tri, (0, 0, 0), extent[::-1], model.SURFACE)
        free = surface == 0
        assert ox == oy == oz == 0 and x[free].any()
        assert np.array_equal(x[free], y[free]) and np.array_equal(x[free], z[free])


# ---------------------------------------------------------------- the stand-alone program: the host routine linked alone
SRCS = [os.path.join(ROOT, "tests", "voxelize_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "voxelize_host.cpp")]


def _run(exe, rounds):
    r = subprocess.run([str(exe), str(rounds)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_voxelize_check_program(tmp_path):
    exe = tmp_path / "voxelize_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe)] + SRCS)
    n = _run(exe, 60)
    assert n["triangles"] > 30 and n["voxels"] > 4000 and n["rows"] > 1000 and n["refused"] == 12


def test_voxelize_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "voxelize_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + SRCS)
    n = _run(exe, 12)
    assert n["refused"] == 12 and n["voxels"] > 4000
