"""bm_host_foot_room, bm_host_foot_field and bm_host_foot_paths (csrc/foot_host.cpp: plain loops over the rules of csrc/foot.h) against the
numpy model of the contract (tests/_foot_model.py: a downward column loop, a plain queue search, the path rule as a loop), byte for byte
-- CPU only.  And tests/foot_check.cpp, a program with its own main that links the host routines alone and runs the kernels' level
scheme on the host with every front in a random order, built plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _foot_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
NAMES = model.NAMES
NONE = model.NONE


@pytest.fixture(scope="module")
def foot(bm):
    from brickmap_amd import foot
    return foot


def agent(c):
    return dict(height=c.height, climb=c.climb, drop=c.drop, toward=c.toward)


def host(foot, c):
    room = foot.host_foot_room(c.volume, c.floor)
    field, rec = foot.host_foot_field(room, c.seeds, max_steps=c.max_steps, **agent(c))
    return room, field, rec


def value(field, p):
    return int(field[p[2], p[1], p[0]])


def test_the_case_list_is_complete():
    assert sorted(model.cases()) == sorted(NAMES) and len(NAMES) == 20 + 72


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_the_model(foot, name):
    c = model.cases()[name]
    room, field, rec = host(foot, c)
    m_room = model.model_room_fast(c.volume, c.floor)
    assert room.dtype == np.uint8 and room.shape == c.volume.shape and room.tobytes() == m_room.tobytes(), f"first difference at {np.argmax(room.ravel() != m_room.ravel())}"
    if c.volume.size <= 4096:
        assert model.model_room(c.volume, c.floor).tobytes() == m_room.tobytes(), "the model's two room loops disagree"
    m_field, m_rec = model.model_field(m_room, c.seeds, max_steps=c.max_steps, **agent(c))
    assert field.dtype == np.int32 and field.tobytes() == m_field.tobytes(), f"first difference at {np.argmax(field.ravel() != m_field.ravel())}"
    assert rec.tobytes() == m_rec.tobytes(), (rec, m_rec)
    # paths: from the farthest voxel in full and cut short, from the first seed, from a voxel without a value and from outside
    far = model.voxel_of(rec["farthest_at"], field.shape)
    starts = [far, c.seeds[0] if c.seeds else (0, 0, 0), (0, 0, field.shape[0] - 1), (-1, 0, 0), (0, field.shape[1], 0)]
    full = int(rec["farthest"]) + 1 if int(rec["reached"]) else 1
    for capacity in sorted({full, min(3, full), 1}):
        path, lengths = foot.host_foot_paths(room, field, starts, capacity, **agent(c))
        m_path, m_lengths = model.model_paths(m_room, m_field, starts, capacity, **agent(c))
        assert path.tobytes() == m_path.tobytes() and lengths.tobytes() == m_lengths.tobytes(), (capacity, lengths, m_lengths)
        assert int(lengths[0]) == (full if int(rec["reached"]) else 0) and lengths[3] == 0 and lengths[4] == 0 and (lengths >= 0).all()
    if name.startswith("random"):
        # the condition of the issue, so that a case cannot pass by reaching nothing
        assert int(rec["reached"]) * 4 >= int(rec["standable"]) and int(rec["farthest"]) >= 25, rec


def test_what_the_named_cases_show(foot):
    cases = model.cases()
    got = {name: host(foot, cases[name]) for name in NAMES if not name.startswith("random")}
    rec = lambda name: {k: int(got[name][2][k]) for k in got[name][2].dtype.names}
    assert rec("one voxel") == dict(reached=1, farthest=0, seeds_rejected=0, farthest_at=0, standable=1)
    assert rec("one voxel, no floor") == dict(reached=0, farthest=NONE, seeds_rejected=1, farthest_at=0, standable=0)
    room = got["room saturates"][0]
    assert room[139, 0, 0] == 127 and room[1, 0, 0] == 0x80 | 127 and int((room & 0x7F).max()) == 127, "the cap is met and not exceeded"
    assert room[139, 0, 1] == 0 and room[138, 0, 1] == 1 and room[12, 0, 1] == 127 and room[11, 0, 1] == 127 and room[1, 0, 1] == 0x80 | 127
    f1, f2 = got["step of one, step of two: climb 1"][1], got["step of one, step of two: climb 2"][1]
    assert value(f1, (2, 0, 2)) == 2 and value(f1, (4, 0, 4)) == NONE and value(f2, (4, 0, 4)) == 4 and value(f2, (5, 0, 4)) == 5
    top, bottom = (2, 0, 4), (3, 0, 1)
    assert value(got["ledge of three: seeded on top"][1], bottom) == 3
    assert value(got["ledge of three: seeded at the bottom"][1], top) == NONE
    assert value(got["ledge of three: toward"][1], top) == 3 and value(got["ledge of three: toward"][1], (0, 0, 4)) == 5
    assert value(got["ledge of three: drop 2 from the top"][1], bottom) == NONE and value(got["ledge of three: drop 2 from the bottom"][1], top) == NONE
    assert rec("lintel: height 1")["reached"] == 7 and rec("lintel: height 2")["reached"] == 3 and rec("lintel: height 2")["standable"] == 6 + 1   # (the lintel's top is a stand too)
    assert rec("head bump")["reached"] == 2 and rec("head bump")["standable"] == 4 + 1, "the lower voxel has R = h: no step up"
    room, field, _ = got["two storeys"]
    assert value(field, (1, 0, 1)) == 1 and value(field, (1, 0, 3)) == 1 and value(field, (2, 0, 1)) == 2, "both storeys get the level"
    path, lengths = foot.host_foot_paths(room, field, [(2, 0, 1)], 3, **agent(cases["two storeys"]))
    assert lengths.tolist() == [3] and path[0].tolist() == [[2, 0, 1], [1, 0, 1], [0, 0, 1]], "the path takes the lower one: z ascends"
    assert rec("wide front") == dict(reached=96 * 96, farthest=96, seeds_rejected=0, farthest_at=96 * 96, standable=96 * 96)
    assert rec("serpentine")["farthest"] == 299 and rec("serpentine, cut in the middle")["farthest"] == 150 and rec("serpentine, cut in the middle")["reached"] == 151
    assert rec("seeds")["seeds_rejected"] == 7 and rec("seeds")["reached"] == 18 and rec("no seeds")["reached"] == 0 and rec("no seeds")["farthest"] == NONE
    assert not cases["pitched"].volume.flags["C_CONTIGUOUS"]


def test_a_field_spoiled_by_hand_ends_the_walk(foot):
    c = model.cases()["serpentine"]
    room, field, rec = host(foot, c)
    start = model.voxel_of(rec["farthest_at"], field.shape)
    path, lengths = foot.host_foot_paths(room, field, [start], 400, **agent(c))
    assert lengths.tolist() == [300] and path[0, 299].tolist() == [0, 0, 1] and (path[0, 300:] == -1).all()
    spoiled = field.copy()
    x, y, z = path[0, 10].tolist()
    spoiled[z, y, x] += 1
    path2, lengths2 = foot.host_foot_paths(room, spoiled, [start], 400, **agent(c))
    assert lengths2.tolist() == [-1] and np.array_equal(path2[0, :10], path[0, :10]) and (path2[0, 10:] == -1).all()
    # a value that fits but whose move is not legal ends the walk as well: the wall beside the corridor
    m_path, m_lengths = model.model_paths(room, spoiled, [start], 400, **agent(c))
    assert m_lengths.tolist() == [-1] and m_path.tobytes() == path2.tobytes()


def test_ground(foot):
    c = model.cases()["seeds"]
    room = foot.host_foot_room(c.volume)
    assert foot.ground(room, [(4, 1, 5), (4, 1, 2), (4, 1, 1), (0, 0, 0), (9, 0, 0)], 2) == [(4, 1, 3), None, None, None, None]
    assert foot.ground(room, [(4, 1, 2), (0, 0, 5)], 1) == [(4, 1, 1), (0, 0, 1)]


def test_every_refusal(bm, foot):
    from brickmap_amd import _lib
    L = bm.load()
    volume = np.zeros((2, 3, 4), np.uint8)
    room, field, res = np.full((2, 3, 4), 7, np.uint8), np.full((2, 3, 4), 7, np.int32), _lib.bm_foot_result()
    seeds, path, lengths = np.zeros((1, 3), np.int32), np.full((1, 2, 3), 7, np.int32), np.full(1, 7, np.int32)

    def params(**kw):
        p = _lib.bm_foot_params()
        p.extent[:] = kw.pop("extent", (4, 3, 2))
        p.height, p.climb, p.drop = 2, 1, 3
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def calls(p, v=volume.ctypes.data, r=room.ctypes.data, f=field.ctypes.data, s=seeds.ctypes.data, n=1, res_p=C.byref(res), capacity=2, pa=path.ctypes.data,
              le=lengths.ctypes.data):
        p = C.byref(p) if p is not None else None
        return (L.bm_host_foot_room(p, C.c_void_p(v), C.c_void_p(r)), L.bm_host_foot_field(p, C.c_void_p(r), C.c_void_p(s), n, C.c_void_p(f), res_p),
                L.bm_host_foot_paths(p, C.c_void_p(r), C.c_void_p(f), C.c_void_p(s), n, capacity, C.c_void_p(pa), C.c_void_p(le)))

    bad = [dict(height=0), dict(height=33), dict(climb=-1), dict(climb=33), dict(drop=-1), dict(drop=65), dict(flags=4), dict(flags=0x80000000), dict(reserved=1),
           dict(reserved2=1), dict(extent=(0, 3, 2)), dict(extent=(4, 16385, 2)), dict(extent=(16384, 16384, 8)), dict(row_pitch=3), dict(row_pitch=-1),
           dict(slice_pitch=11), dict(slice_pitch=1 << 46)]
    for kw in bad:
        assert calls(params(**kw)) == (EINVAL,) * 3, kw
        assert b"bm_host_foot_paths" in L.bm_last_error_string()
    assert calls(None) == (EINVAL,) * 3
    p, vp = C.byref(params()), C.c_void_p
    v, r, f, sd, pa, le = (a.ctypes.data for a in (volume, room, field, seeds, path, lengths))
    assert L.bm_host_foot_room(p, None, vp(r)) == EINVAL and L.bm_host_foot_room(p, vp(v), None) == EINVAL
    for kw in (dict(r=None), dict(f=None), dict(s=None), dict(n=-1), dict(res_p=None)):
        a = dict(dict(r=r, s=sd, n=1, f=f, res_p=C.byref(res)), **kw)
        assert L.bm_host_foot_field(p, vp(a["r"]), vp(a["s"]), a["n"], vp(a["f"]), a["res_p"]) == EINVAL, kw
    for kw in (dict(r=None), dict(f=None), dict(s=None), dict(n=-1), dict(capacity=0), dict(pa=None), dict(le=None)):
        a = dict(dict(r=r, f=f, s=sd, n=1, capacity=2, pa=pa, le=le), **kw)
        assert L.bm_host_foot_paths(p, vp(a["r"]), vp(a["f"]), vp(a["s"]), a["n"], a["capacity"], vp(a["pa"]), vp(a["le"])) == EINVAL, kw
    assert (room == 7).all() and (field == 7).all() and (path == 7).all() and (lengths == 7).all(), "a refused call writes nothing"
    assert calls(params(flags=3, max_steps=5, row_pitch=4, slice_pitch=12)) == (0, 0, 0)
    assert calls(params(), s=None, n=0, pa=None, le=None)[1:] == (0, 0)   # without seeds or starts the pointers may be null
    size = C.c_size_t(0)
    assert L.bm_foot_workspace_bytes(C.byref(params(height=0)), C.byref(size)) == EINVAL and L.bm_foot_workspace_bytes(None, C.byref(size)) == EINVAL
    assert L.bm_foot_workspace_bytes(C.byref(params()), None) == EINVAL
    assert L.bm_foot_workspace_bytes(C.byref(params(extent=(5, 3, 7))), C.byref(size)) == 0 and size.value == 4 * 4 * 15 + 64   # ceil(7 / 2) entries per column
    assert foot.foot_workspace_bytes((7, 3, 5)) == size.value
    for kw in (dict(height=0), dict(climb=33), dict(drop=65), dict(max_steps=-1)):
        with pytest.raises(ValueError):
            foot.host_foot_field(np.zeros((2, 2, 2), np.uint8), [], **kw)


def test_the_params_begin_with_the_travel_params_and_the_record_dtype():
    from brickmap_amd import _lib
    assert _lib.FOOT_RESULT_DTYPE == model.RESULT_DTYPE and _lib.FOOT_RESULT_DTYPE.itemsize == 32 == C.sizeof(_lib.bm_foot_result)
    assert C.sizeof(_lib.bm_foot_params) == C.sizeof(_lib.bm_travel_params) + 16
    for name, _ in _lib.bm_travel_params._fields_:
        assert getattr(_lib.bm_foot_params, name).offset == getattr(_lib.bm_travel_params, name).offset, name
    assert _lib.BM_FOOT_NONE == NONE


def test_the_module_adds_no_name_to_the_package():
    import brickmap_amd
    from brickmap_amd import foot, host
    for name in ("foot_room", "foot_field", "find_walk", "FootField", "host_foot_room", "host_foot_field", "host_foot_paths", "foot_workspace_bytes", "FOOT_RESULT_DTYPE",
                 "FOOT_NONE", "foot_field_times"):
        assert not hasattr(host, name) and not hasattr(brickmap_amd, name), name
        assert hasattr(foot, name), name


# ---------------------------------------------------------------- the check program
SRCS = [os.path.join(ROOT, "tests", "foot_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "foot_host.cpp")]
WANT = {"volumes": 200, "refused": 14, "failures": 0}


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split() for line in r.stdout.strip().splitlines() if len(line.split()) == 2)
    assert {k: int(got[k]) for k in WANT} == WANT, r.stdout + r.stderr


def test_foot_check_program(tmp_path):
    exe = tmp_path / "foot_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe)] + SRCS)
    _run(exe)


def test_foot_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "foot_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + SRCS)
    _run(exe)
