"""bm_host_water_field and bm_host_water_mask (csrc/water_host.cpp: a plain priority flood over the rules of csrc/water.h) against the numpy
model of the spill-level contract (tests/_water_model.py: height by height, by shifting), byte for byte -- CPU only.  And
tests/water_check.cpp, a program with its own main that links the host routine alone and runs the kernels' in-tile sweeps and round
scheme lane by lane, built plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _water_cases as cases
import _water_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
NONE = model.NONE


@pytest.fixture(scope="module")
def water():
    from brickmap_amd import water
    return water


def both(water, vol, drains=None, open=cases.SIDES, sea=0):
    want, rec = model.model_water_field(vol, drains, open, sea)
    got, r = water.host_water_field(vol, drains, open, sea)
    assert got.dtype == np.int32 and got.shape == vol.shape
    assert got.tobytes() == want.tobytes(), f"{vol.shape}: first difference at {np.argmax(got.ravel() != want.ravel())}"
    assert r == rec, (r, rec)
    z = np.arange(vol.shape[0])[:, None, None]
    assert (got >= z).all() and (got[vol != 0] == NONE).all()
    for depth in (1, 2, 5):
        assert water.host_water_mask(got, depth).tobytes() == model.model_water_mask(want, depth).tobytes()
    return got, r


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_host_equals_the_model(water, case):
    both(water, *case[1:])


def test_what_the_shapes_say(water):
    got, rec = both(water, np.zeros((1, 1, 1), np.uint8))
    assert got.item() == 0 and (int(rec["wet"]), int(rec["closed"]), int(rec["deepest"])) == (0, 0, 0), "an outlet, dry"
    got, rec = both(water, np.ones((1, 1, 1), np.uint8))
    assert got.item() == NONE and int(rec["closed"]) == 0
    got, rec = both(water, cases.bowl())
    assert (got[2:5, 4:8, 4:8] == 5).all() and int(rec["wet"]) == 48 and (int(rec["deepest"]), int(rec["deepest_at"])) == (3, (2 * 12 + 4) * 12 + 4)
    assert (got[5:] == np.arange(5, 8)[:, None, None]).all(), "the air above the plateau is dry"
    assert water.host_water_mask(got, 3).sum() == 16 and water.host_water_mask(got, 4).sum() == 0
    got, rec = both(water, cases.u_tube())
    assert (got[1:10, 2, 2] == 10).all() and (got[1:10, 2, 8] == 10).all() and (got[10:13, 2, 8] == [10, 11, 12]).all(), "both arms stand at the left rim"
    got, rec = both(water, cases.pit_with_tunnel())
    assert int(rec["wet"]) == 0 and (got[2, 5, :8] == 2).all()
    got, rec = both(water, cases.air_bell())
    assert int(rec["wet"]) == 0 and int(rec["closed"]) == 0 and got[7, 3, 5] == 7
    got, rec = both(water, cases.closed_cave())
    assert int(rec["closed"]) == 13 and (got[0:2, 1:3, 1:4] == NONE).all() and int(rec["wet"]) == 48
    got, rec = both(water, cases.bowl(), [(5, 5, 2)])
    assert int(rec["wet"]) == 0 and int(rec["drains_rejected"]) == 0 and (got[2:5, 4:8, 4:8] == np.arange(2, 5)[:, None, None]).all(), "the drain empties it"
    got, rec = both(water, cases.bowl(), [(-1, 0, 0), (12, 0, 0), (0, 12, 0), (0, 0, 8), (0, 0, 0), (5, 5, 2), (5, 5, 2)])
    assert int(rec["drains_rejected"]) == 5 and int(rec["wet"]) == 0
    got, rec = both(water, cases.bowl(), None, ())
    assert (got == NONE).all() and int(rec["closed"]) == int((cases.bowl() == 0).sum()) and int(rec["wet"]) == 0, "nothing is an outlet"
    got, rec = both(water, cases.bowl(), [(5, 5, 3)], ())
    assert (got[3:, 5, 5] == np.arange(3, 8)).all() and got[2, 5, 5] == 3 and int(rec["wet"]) == 16, "below the drain the pit stays full"
    got, rec = both(water, cases.bowl(), None, cases.SIDES, 8)
    assert (got[cases.bowl() == 0] == 8).all() and int(rec["deepest"]) == 6
    got, rec = both(water, cases.bowl(), None, cases.SIDES, 4)
    assert (got[2:5, 4:8, 4:8] == 5).all() and (got[5:] == np.arange(5, 8)[:, None, None]).all(), "a sea below the rim changes nothing here"
    got, rec = both(water, cases.bowl(), None, cases.SIDES, 6)
    assert (got[2:6][cases.bowl()[2:6] == 0] == 6).all() and (got[6:] == np.arange(6, 8)[:, None, None]).all()


def test_late_levels_and_long_corridors(water):
    got, rec = both(water, cases.late_detour(), None, ("-x",))
    assert (got[1:11, 3, 38] == np.arange(1, 11)).all(), "the low way drains the shaft"
    got, rec = both(water, cases.serpentine(), None, ("-x",))
    assert int(rec["wet"]) == 0 and int(rec["closed"]) == 0


@pytest.mark.parametrize("case", cases.RANDOM, ids=[c[0] for c in cases.RANDOM])
def test_random_volumes_hold_every_kind_of_voxel(water, case):
    got, rec = both(water, *case[1:])
    wet, dry, _ = model.counts(got)
    assert wet >= 100 and dry >= 100 and int(rec["closed"]) >= 50, (wet, dry, int(rec["closed"]))
    assert wet == int(rec["wet"])


def test_a_slice_of_a_larger_array(water):
    big = cases.random_volume(5, 0.55, (12, 14, 40)) * 7
    view = big[1:11, 2:13, 3:36]
    assert not view.flags["C_CONTIGUOUS"]
    got, rec = both(water, view, [(4, 4, 4)], cases.SIDES, 2)
    tight, rec2 = water.host_water_field(np.ascontiguousarray(view), [(4, 4, 4)], cases.SIDES, 2)
    assert got.tobytes() == tight.tobytes() and rec == rec2
    assert water.host_water_field(view.astype(bool))[0].tobytes() == water.host_water_field(view)[0].tobytes()


# ---------------------------------------------------------------- refusals
def test_every_refusal(water):
    from brickmap_amd import _lib
    L = _lib.load()
    vol = np.zeros((8, 8, 8), np.uint8)
    field = np.full((8, 8, 8), -7, np.int32)
    drains = np.zeros((2, 3), np.int32)
    res = _lib.bm_water_result(77, 77, 77, 77, 77)

    def message():
        return (L.bm_last_error_string() or b"").decode()

    def call(extent=(8, 8, 8), row=0, sl=0, flags=15, reserved=0, sea=0, v=vol.ctypes.data, s=drains.ctypes.data, n=2, f=field.ctypes.data, r=C.byref(res)):
        par = _lib.bm_water_params()
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.flags, par.reserved, par.sea_level = row, sl, flags, reserved, sea
        return L.bm_host_water_field(C.byref(par), C.c_void_p(v), C.c_void_p(s), n, C.c_void_p(f), r)

    refused = [(dict(extent=(0, 8, 8)), "an extent below 1 or above 16384"), (dict(extent=(8, -1, 8)), "an extent below 1 or above 16384"),
               (dict(extent=(8, 8, 16385)), "an extent below 1 or above 16384"), (dict(extent=(16384, 16384, 8)), "more than 2^31 - 2 voxels"),
               (dict(row=7), "row_pitch below the extent along x"), (dict(row=-8), "negative pitch"), (dict(sl=63), "slice_pitch below row_pitch * the extent along y"),
               (dict(sl=-1), "negative pitch"), (dict(flags=64), "unknown flag"), (dict(flags=0x80000000), "unknown flag"), (dict(reserved=1), "reserved is not 0"),
               (dict(sea=9), "sea_level above the extent along z"), (dict(v=0), "null volume, drains, field or result"), (dict(f=0), "null volume, drains, field or result"),
               (dict(r=None), "null volume, drains, field or result"), (dict(s=0), "null volume, drains, field or result"), (dict(n=-1), "a negative number of drains")]
    for kw, why in refused:
        assert call(**kw) == EINVAL, kw
        assert message() == "bm_host_water_field: " + why, (kw, message())
        assert (field == -7).all() and (res.wet, res.deepest, res.drains_rejected, res.deepest_at, res.closed) == (77, 77, 77, 77, 77), "nothing is written"
    assert call(flags=64, reserved=1, extent=(0, 8, 8)) == EINVAL and message() == "bm_host_water_field: unknown flag", "the order of bm_travel_field"
    assert L.bm_host_water_field(None, C.c_void_p(vol.ctypes.data), C.c_void_p(drains.ctypes.data), 2, C.c_void_p(field.ctypes.data), C.byref(res)) == EINVAL
    assert call(s=0, n=0, flags=0) == 0 and (field == NONE).all() and (res.wet, res.deepest, res.drains_rejected, res.deepest_at, res.closed) == (0, 0, 0, 0, 512)
    assert call(row=8, sl=64, sea=8, flags=63) == 0 and (field == 8).all() and (res.wet, res.deepest, res.deepest_at, res.closed) == (512, 8, 0, 0)

    mask = np.full((8, 8, 8), 9, np.uint8)

    def mask_call(extent=(8, 8, 8), f=field.ctypes.data, depth=1, m=mask.ctypes.data):
        return L.bm_host_water_mask((C.c_int32 * 3)(*extent) if extent else None, C.c_void_p(f), depth, C.c_void_p(m))

    for kw in (dict(extent=None), dict(extent=(0, 8, 8)), dict(extent=(8, 8, 16385)), dict(extent=(16384, 16384, 8)), dict(f=0), dict(m=0), dict(depth=0)):
        assert mask_call(**kw) == EINVAL, kw
        assert (mask == 9).all(), "nothing is written"
    assert mask_call(depth=8) == 0 and (mask[0] == 1).all() and (mask[1:] == 0).all()

    size = C.c_size_t(0)
    par = _lib.bm_water_params()
    assert L.bm_water_workspace_bytes(C.byref(par), C.byref(size)) == EINVAL, "extents of 0"
    par.extent[:] = [8, 8, 8]
    assert L.bm_water_workspace_bytes(C.byref(par), None) == EINVAL and L.bm_water_workspace_bytes(None, C.byref(size)) == EINVAL
    par.flags = 64
    assert L.bm_water_workspace_bytes(C.byref(par), C.byref(size)) == EINVAL
    par.flags, par.sea_level = 63, 9
    assert L.bm_water_workspace_bytes(C.byref(par), C.byref(size)) == EINVAL
    assert water.water_workspace_bytes((8, 8, 8)) == 64 + 3 * 16 + 64, "one tile: its brick, a stamp and two list entries each rounded up to 16, and the tail"
    assert water.water_workspace_bytes((9, 8, 8)) == 2 * 64 + 3 * 16 + 64 and water.water_workspace_bytes((17, 17, 17)) == 27 * 64 + 3 * 112 + 64
    assert water.water_workspace_bytes((7, 16384, 16384)) == (1 << 22) * 64 + 3 * (1 << 24) + 64
    from brickmap_amd import volumes
    assert all(water.water_workspace_bytes(s) == volumes.travel_workspace_bytes(s) for s in ((1, 1, 1), (19, 20, 24), (64, 64, 64)))
    with pytest.raises(ValueError):
        water.host_water_field(np.zeros((8, 8, 8), np.int32))
    with pytest.raises(ValueError):
        water.host_water_field(vol, [(1, 2)])
    with pytest.raises(ValueError):
        water.host_water_field(vol, open=("up",))
    with pytest.raises(ValueError):
        water.host_water_field(vol, sea_level=-1)
    with pytest.raises(ValueError):
        water.host_water_mask(np.zeros((2, 2, 2), np.float32))
    with pytest.raises(ValueError):
        water.host_water_mask(np.zeros((2, 2, 2), np.int32), 0)
    assert water.WATER_NONE == NONE == _lib.BM_WATER_NONE and water.WATER_RESULT_DTYPE == model.RESULT_DTYPE and water.WATER_RESULT_DTYPE.itemsize == 32
    assert C.sizeof(_lib.bm_water_params) == 40 and C.sizeof(_lib.bm_water_result) == 32


# ---------------------------------------------------------------- the stand-alone program: the host routine linked alone
SRCS = [os.path.join(ROOT, "tests", "water_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "water_host.cpp")]
WANT = {"rows": 4096, "tiles": 10000, "volumes": 40, "refused": 14, "failures": 0}


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def _check(n):
    assert {k: n[k] for k in WANT} == WANT, n
    assert 100 < n["snake_sweeps"] < 512, "the serpentine tile needs many sweeps, and fewer than the bound"
    assert 0 < n["most_sweeps"] < 512, "the in-tile sweeps stay below their bound"
    assert n["rounds_over"] == 0, "no volume needed more rounds than the cap"
    assert n["refalls"] > 0, "some tile's values fell in more than one round"


def test_water_check_program(tmp_path):
    exe = tmp_path / "water_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe)] + SRCS)
    _check(_run(exe))


def test_water_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "water_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + SRCS)
    _check(_run(exe))
