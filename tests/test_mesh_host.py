"""bm_host_mesh_quads and bm_host_mesh_triangles (csrc/mesh_host.cpp: plain loops over the rules of csrc/mesh.h) against the numpy model of
the surface-extraction contract (tests/_mesh_model.py), byte for byte; and, independent of the model's greedy loop, against what a mesh of
a surface has to be: painted back, the quads give every face once; tiles meshed with a halo give the whole without walls; the triangles,
voxelized again, give the volume back -- CPU only.  And tests/mesh_check.cpp, a program with its own main that links the host routine
alone, built plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _mesh_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001


def random_volume(seed, shape, density):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def both(bm, vol, lo=(0, 0, 0), halo=False, unit=False):
    want, rec = model.model_mesh_quads(vol, lo, halo, unit)
    got, r = bm.host_mesh_quads(vol, lo, halo=halo, unit=unit)
    assert got.dtype == bm.QUAD_DTYPE and r == rec, (r, rec)
    assert got.tobytes() == want.tobytes(), f"{vol.shape} at {lo} halo {halo} unit {unit}: first difference at {np.argmax(got != want) if len(got) == len(want) else (len(got), len(want))}"
    return got, r


# ---------------------------------------------------------------- the host routine against the model
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("extent", [(1, 1, 1), (8, 8, 8), (9, 8, 8), (17, 10, 9)])
def test_random_volumes(bm, extent, density):
    """extents are (nx, ny, nz); every combination of the two flags that the extents allow"""
    vol = random_volume(1, extent[::-1], density)
    if extent == (1, 1, 1):
        vol[:] = density < 0.9
    for halo in ((False, True) if min(extent) >= 3 else (False,)):
        for unit in (False, True):
            got, r = both(bm, vol, halo=halo, unit=unit)
            if unit:
                assert r["quads"] == r["faces"]
    assert bm.host_mesh_quads(np.ones((1, 1, 1), np.uint8))[1]["quads"] == 6


@pytest.mark.parametrize("lo", [(3, -5, 6), (-8, -16, 0)])
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_negative_origins_pin_floor_division_and_ragged_first_cells(bm, lo, density):
    vol = random_volume(2, (9, 10, 17), density)
    got, _ = both(bm, vol, lo)
    both(bm, vol, lo, halo=True)
    both(bm, vol, lo, unit=True)
    # no quad crosses a world cell boundary
    d, w, h = got["shape"] & 15, (got["shape"] >> 4) & 15, (got["shape"] >> 8) & 15
    for axis, name in enumerate("xyz"):
        ua, va = zip(*[model.IN_SLICE[k >> 1] for k in d])
        size = np.where(np.array(ua) == axis, w, np.where(np.array(va) == axis, h, 1))
        assert ((got[name] // 8) == ((got[name] + size - 1) // 8)).all()
    assert (got["x"] // 8).min() == lo[0] // 8


def test_empty_full_and_checkerboard(bm):
    got, r = both(bm, np.zeros((9, 10, 17), np.uint8))
    assert len(got) == 0 and tuple(r.tolist()) == (0, 0)
    got, r = both(bm, np.ones((16, 16, 16), np.uint8))
    assert len(got) == 24 and ((got["shape"] >> 4) == 0x88).all() and r["faces"] == 6 * 16 * 16
    got, r = both(bm, np.ones((16, 16, 16), np.uint8), lo=(4, 0, 0))
    assert len(got) == 2 * 4 + 4 * 6, "three cells along x and two along y and z: the two faces across in 2 x 2 pieces, the four sides in 3 x 2"
    z, y, x = np.indices((16, 16, 16))
    got, r = both(bm, ((x + y + z) & 1).astype(np.uint8))
    assert len(got) == 8 * 1536 and r["faces"] == len(got), "1536 unit quads per full cell"


def test_any_non_zero_byte_is_solid(bm):
    bits = random_volume(3, (9, 10, 17), 0.4)
    vol = bits * np.random.default_rng(4).choice(np.array([2, 255], np.uint8), size=bits.shape)
    assert set(np.unique(vol)) == {0, 2, 255}
    assert both(bm, vol)[0].tobytes() == bm.host_mesh_quads(bits)[0].tobytes()
    assert bm.host_mesh_quads(bits.astype(bool))[0].tobytes() == bm.host_mesh_quads(bits)[0].tobytes()


def test_a_slice_of_a_larger_array(bm):
    big = random_volume(5, (12, 14, 40), 0.5)
    view = big[1:11, 2:13, 3:36]
    assert not view.flags["C_CONTIGUOUS"]
    for halo in (False, True):
        got, _ = both(bm, view, (-2, 3, 1), halo=halo)
        assert got.tobytes() == bm.host_mesh_quads(np.ascontiguousarray(view), (-2, 3, 1), halo=halo)[0].tobytes()


# ---------------------------------------------------------------- independent of the model's greedy loop
@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("density", [0.15, 0.5, 0.9])
def test_painted_back_the_quads_give_every_face_once(bm, density, unit, halo):
    vol, lo = random_volume(6, (10, 9, 19), density), (5, -3, -11)
    quads, rec = bm.host_mesh_quads(vol, lo, halo=halo, unit=unit)
    painted = model.paint(quads, lo, vol.shape)
    solid = np.pad(vol != 0, 1)
    inner = (slice(1, -1),) * 3
    faces = 0
    for d, (axis, step) in enumerate(model.DIRECTIONS):
        want = solid[inner] & ~np.roll(solid, -step, axis=2 - axis)[inner]
        if halo:
            keep = np.zeros(vol.shape, bool)
            keep[inner] = True
            want &= keep
        assert painted[d].max() <= 1, "a face appears twice"
        assert np.array_equal(painted[d].astype(bool), want), "a face is missed, or one is invented"
        faces += int(want.sum())
    w, h = (quads["shape"] >> 4) & 15, (quads["shape"] >> 8) & 15
    assert rec["faces"] == faces == int((w * h).sum()) and rec["quads"] == len(quads)
    assert (w >= 1).all() and (h >= 1).all() and (w <= 8).all() and (h <= 8).all() and ((quads["shape"] & 15) < 6).all() and (quads["shape"] >> 12 == 0).all()


def test_halo_tiles_give_the_whole_without_walls(bm):
    """32^3 as eight tiles whose meshed boxes are 16^3 (15 at the volume's border, which is context only), at origins that are multiples
    of 8: the tiles' cells are the whole's cells, so their quads are, as a set, those of the whole volume meshed with a halo -- and with
    unit faces those of the closed whole volume whose voxel is not on the outer border."""
    vol = random_volume(7, (32, 32, 32), 0.5)
    for unit in (False, True):
        tiles = []
        for z in (0, 16):
            for y in (0, 16):
                for x in (0, 16):
                    lo = (max(x - 1, 0), max(y - 1, 0), max(z - 1, 0))
                    hi = (min(x + 17, 32), min(y + 17, 32), min(z + 17, 32))
                    tiles.append(bm.host_mesh_quads(vol[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]], lo, halo=True, unit=unit)[0])
        got = np.concatenate(tiles)
        assert len(np.unique(got)) == len(got)
        whole = bm.host_mesh_quads(vol, halo=True, unit=unit)[0]
        assert np.array_equal(np.sort(got, order=["z", "y", "x", "shape"]), np.sort(whole, order=["z", "y", "x", "shape"]))
        if unit:
            closed = bm.host_mesh_quads(vol, unit=True)[0]
            inside = np.ones(len(closed), bool)
            for name in "xyz":
                inside &= (closed[name] >= 1) & (closed[name] <= 30)
            assert np.array_equal(np.sort(got, order=["z", "y", "x", "shape"]), np.sort(closed[inside], order=["z", "y", "x", "shape"]))
    # a tile at an origin that is no multiple of 8 has other cells: the same faces, other quads
    a = bm.host_mesh_quads(vol[:18, :18, :18], halo=True)[0]
    b = bm.host_mesh_quads(vol[:18, :18, :18], (3, 0, 0), halo=True)[0]
    assert len(a) != len(b) and all(np.array_equal(p, q) for p, q in zip(model.paint(a, (0, 0, 0), (18, 18, 18)), model.paint(b, (3, 0, 0), (18, 18, 18))))


# ---------------------------------------------------------------- triangles and the round trip
def test_triangles_equal_the_model_and_face_outwards(bm):
    vol, lo = random_volume(8, (9, 12, 17), 0.5), (-8, 3, 1 << 20)
    quads, _ = bm.host_mesh_quads(vol, lo)
    tri = bm.host_mesh_triangles(quads)
    assert tri.dtype == np.float32 and tri.shape == (2 * len(quads), 3, 3) and tri.tobytes() == model.model_triangles(quads).tobytes()
    n = np.cross(tri[:, 1].astype(np.float64) - tri[:, 0], tri[:, 2].astype(np.float64) - tri[:, 0])
    d = np.repeat(quads["shape"] & 15, 2)
    for k, (axis, step) in enumerate(model.DIRECTIONS):
        mine = n[d == k]
        assert (mine[:, axis] * step > 0).all() and not np.delete(mine, axis, axis=1).any()
    w, h = (quads["shape"] >> 4) & 15, (quads["shape"] >> 8) & 15
    assert np.array_equal(np.abs(n).sum(axis=1).reshape(-1, 2).sum(axis=1) / 2, (w * h).astype(np.float64))
    assert bm.host_mesh_triangles(quads[:0]).shape == (0, 3, 3)
    odd = np.array([(1, 2, 3, 6 | 1 << 4 | 1 << 8), (1, 2, 3, 15 | 8 << 4 | 8 << 8)], bm.QUAD_DTYPE)
    assert not bm.host_mesh_triangles(odd).any(), "a direction above 5: zeros"


@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("shape,density", [((9, 12, 17), 0.15), ((9, 12, 17), 0.5), ((9, 12, 17), 0.9), ((10, 9, 11), 0.15), ((10, 9, 11), 0.5), ((10, 9, 11), 0.9),
                                           ((8, 8, 8), 0.15), ((8, 8, 8), 0.5), ((8, 8, 8), 0.9), ((8, 8, 8), "checkerboard")])
def test_the_mesh_voxelizes_back_to_the_volume(bm, shape, density, unit):
    """shapes are (nz, ny, nx).  Centres lie half a voxel from every quad, so the parity fill has no ties to break."""
    if density == "checkerboard":
        z, y, x = np.indices(shape)
        vol = ((x + y + z) & 1).astype(np.uint8)
    else:
        vol = random_volume(9, shape, density)
    for lo in ((0, 0, 0), (3, -5, 6)):
        quads, _ = bm.host_mesh_quads(vol, lo, unit=unit)
        back, rec = bm.host_voxelize(bm.host_mesh_triangles(quads), lo, shape, "solid")
        assert np.array_equal(back, vol) and rec["open_columns"] == 0 and rec["degenerate"] == 0 and rec["rejected"] == 0


# ---------------------------------------------------------------- refusals
def test_every_refusal(bm):
    from brickmap_amd import _lib
    L = bm.load()
    vol = np.ones((8, 8, 8), np.uint8)
    out = np.full(64, -1, np.int32).view(np.int32)
    quads = np.zeros(64, bm.QUAD_DTYPE)
    quads["shape"] = 0xFFFFFFFF
    res = _lib.bm_mesh_result(77, 77)

    def call(extent=(8, 8, 8), lo=(0, 0, 0), row=0, sl=0, flags=0, reserved=0, v=vol.ctypes.data, q=quads.ctypes.data, cap=64, r=C.byref(res)):
        par = _lib.bm_mesh_params()
        par.lo[:] = list(lo)
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.flags, par.reserved = row, sl, flags, reserved
        return L.bm_host_mesh_quads(C.byref(par), C.c_void_p(v), C.c_void_p(q), cap, r)

    for kw in (dict(extent=(0, 8, 8)), dict(extent=(8, -1, 8)), dict(extent=(8, 8, 16385)), dict(extent=(8, 2, 8), flags=1), dict(extent=(16384, 16384, 8)), dict(row=7),
               dict(row=-8), dict(sl=63), dict(sl=-1), dict(flags=4), dict(flags=0x80000001), dict(reserved=1), dict(v=0), dict(r=None), dict(q=0, cap=1),
               dict(lo=((1 << 23) - 7, 0, 0)), dict(lo=(0, 0, -(1 << 23) - 1))):
        assert call(**kw) == EINVAL, kw
        assert (quads["shape"] == 0xFFFFFFFF).all() and (res.quads, res.faces) == (77, 77), "nothing is written"
    assert L.bm_host_mesh_quads(None, C.c_void_p(vol.ctypes.data), None, 0, C.byref(res)) == EINVAL
    assert call(row=8, sl=64) == 0 and (res.quads, res.faces) == (6, 384) and (quads["shape"][6:] == 0xFFFFFFFF).all()
    assert call(q=0, cap=0) == 0 and call(extent=(8, 3, 8), flags=1) == 0 and call(lo=((1 << 23) - 8, -(1 << 23), 0)) == 0
    size = C.c_size_t(0)
    par = _lib.bm_mesh_params()
    assert L.bm_mesh_workspace_bytes(C.byref(par), C.byref(size)) == EINVAL, "extents of 0"
    assert bm.mesh_workspace_bytes((40, 80, 80)) == 500 * 4 + 3 * 8, "500 cells, two scan blocks and the total"
    assert bm.mesh_workspace_bytes((8, 8, 8)) == 16 + 16 and bm.mesh_workspace_bytes((8, 8, 8), lo=(1, 0, 0)) == 16 + 16
    assert bm.mesh_workspace_bytes((10, 10, 10), halo=True, lo=(-1, -1, -1)) == 16 + 16, "the halo is no cell of its own"
    assert bm.mesh_workspace_bytes((10, 10, 10), lo=(-1, -1, -1)) == 27 * 4 + 4 + 16
    assert L.bm_host_mesh_triangles(None, 1, None) == EINVAL and L.bm_host_mesh_triangles(None, -1, None) == EINVAL
    with pytest.raises(ValueError):
        bm.host_mesh_quads(np.ones((8, 8, 8), np.int32))
    assert bm.QUAD_DTYPE == model.QUAD_DTYPE and bm.QUAD_DTYPE.itemsize == 16 and bm.MESH_RESULT_DTYPE == model.RESULT_DTYPE and bm.MESH_RESULT_DTYPE.itemsize == 16


# ---------------------------------------------------------------- the stand-alone program: the host routine linked alone
SRCS = [os.path.join(ROOT, "tests", "mesh_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "mesh_host.cpp")]


def _run(exe, rounds):
    r = subprocess.run([str(exe), str(rounds)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_mesh_check_program(tmp_path):
    exe = tmp_path / "mesh_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe)] + SRCS)
    n = _run(exe, 60)
    assert n["masks"] == 2 * 3 * 65536 + 200000 and n["cells"] > 500 and n["dropped"] > 10 and n["quads"] > 50000 and n["triangles"] > 1000 and n["refused"] == 17


def test_mesh_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "mesh_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + SRCS)
    n = _run(exe, 12)
    assert n["refused"] == 17 and n["quads"] > 5000
