"""bm_host_settle (csrc/settle_host.cpp: plain loops over the rules of csrc/settle.h) against the numpy model of the settling contract
(tests/_settle_model.py: the contacts by plain column loops, relaxed until nothing changes), byte for byte -- CPU only.  And
tests/settle_check.cpp, a program with its own main that links the host routine alone and runs the kernels' round scheme on the host with
reads that see either the round's start or a value lowered in the same round, built plain and under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _settle_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
NAMES = model.NAMES


def test_the_case_list_is_complete(bm):
    assert sorted(model.cases(bm)) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_the_model(bm, name):
    from brickmap_amd import settle
    labels, records, chosen, want = model.cases(bm)[name]
    out, drops, rec = settle.host_settle(labels, records, chosen)
    m_out, m_drops, m_rec = model.model_settle(labels, records, chosen)
    assert out.dtype == np.uint8 and out.shape == labels.shape and drops.dtype == np.int32
    assert out.tobytes() == m_out.tobytes(), f"first difference at {np.argmax(out.ravel() != m_out.ravel())}"
    assert drops.tobytes() == m_drops.tobytes()
    assert rec.tobytes() == m_rec.tobytes(), (rec, m_rec)
    if want is not None:
        assert drops[chosen != 0].tolist() == want
    # nothing is lost, nothing is made, and what was not chosen stays where it was
    assert int((out != 0).sum()) == int((labels != 0).sum())
    assert int((out == 2).sum()) == int(rec["moved_voxels"]) and (drops[chosen == 0] == 0).all()
    if name == "two interlocked pieces":
        assert out.tobytes() == model.INTERLOCKED_OUT.tobytes()
    if name in ("n = 0", "chosen all zero"):
        assert np.array_equal(out, (labels != 0).astype(np.uint8)) and not drops.any() and int(rec["contacts"]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_settling_the_result_again_moves_nothing(bm, name):
    """every piece of the case that touches neither the floor nor a side face is chosen (a piece left hanging would fall in the second
    run); the result is relabelled and the same choice made again: all drops are 0"""
    from brickmap_amd import settle
    labels = model.cases(bm)[name][0]
    records = model.table_of(labels)
    out, _, _ = settle.host_settle(labels, records, model.loose(records))
    again, table = model.label_and_table(bm, out != 0)
    _, drops, rec = settle.host_settle(again, table, model.loose(table))
    assert not drops.any() and int(rec["moved_voxels"]) == 0 and int(rec["largest_drop"]) == 0


def test_a_chosen_record_without_voxels_falls_nowhere(bm):
    from brickmap_amd import settle
    labels = np.zeros((4, 1, 2), np.int32)
    labels[2, 0, 0] = 3
    records = np.zeros(2, model.COMPONENT_DTYPE)
    records["label"] = (3, 8)
    out, drops, rec = settle.host_settle(labels, records, [1, 1])
    assert drops.tolist() == [2, 0] and out[0, 0, 0] == 2 and int(rec["chosen_pieces"]) == 2 and int(rec["moved_pieces"]) == 1


def test_every_refusal(bm):
    from brickmap_amd import _lib
    L = bm.load()
    labels = np.zeros((2, 3, 4), np.int32)
    records = np.zeros(1, model.COMPONENT_DTYPE)
    chosen, out, drops, res = np.zeros(1, np.uint8), np.full((2, 3, 4), 7, np.uint8), np.full(1, 7, np.int32), _lib.bm_settle_result()

    def call(extent=(4, 3, 2), labels_p=labels.ctypes.data, records_p=records.ctypes.data, n=1, chosen_p=chosen.ctypes.data, out_p=out.ctypes.data,
             drops_p=drops.ctypes.data, res_p=C.byref(res)):
        ext = (C.c_int32 * 3)(*extent) if extent is not None else None
        return L.bm_host_settle(ext, C.c_void_p(labels_p), C.c_void_p(records_p), n, C.c_void_p(chosen_p), C.c_void_p(out_p), C.c_void_p(drops_p), res_p)

    assert call() == 0 and not out.any() and not drops.any()
    out[:], drops[:] = 7, 7
    bad = [dict(extent=None), dict(extent=(0, 3, 2)), dict(extent=(4, 16385, 2)), dict(extent=(16384, 16384, 8)), dict(n=-1), dict(labels_p=None), dict(out_p=None),
           dict(res_p=None), dict(records_p=None), dict(chosen_p=None), dict(drops_p=None)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert b"bm_host_settle" in L.bm_last_error_string()
    assert (out == 7).all() and (drops == 7).all(), "a refused call writes nothing"
    assert call(n=0, records_p=None, chosen_p=None, drops_p=None) == 0   # without records the three pointers may be null
    size = C.c_size_t(0)
    assert L.bm_settle_workspace_bytes((C.c_int32 * 3)(0, 1, 1), 1, C.byref(size)) == EINVAL
    assert L.bm_settle_workspace_bytes((C.c_int32 * 3)(4, 3, 2), -1, C.byref(size)) == EINVAL
    assert L.bm_settle_workspace_bytes((C.c_int32 * 3)(4, 3, 2), 1, None) == EINVAL
    assert L.bm_settle_workspace_bytes((C.c_int32 * 3)(130, 3, 6), 5, C.byref(size)) == 0 and size.value == 32 + 32 + 72   # 5 records, 7 groups, the tail


def test_the_record_dtype():
    from brickmap_amd import _lib
    assert _lib.SETTLE_RESULT_DTYPE == model.RESULT_DTYPE and _lib.SETTLE_RESULT_DTYPE.itemsize == 32 == C.sizeof(_lib.bm_settle_result)


def test_the_module_adds_no_name_to_the_package():
    import brickmap_amd
    from brickmap_amd import host
    for name in ("settle_workspace_bytes", "host_settle", "settle_floating", "Settled", "SETTLE_RESULT_DTYPE"):
        assert not hasattr(host, name) and not hasattr(brickmap_amd, name), name


# ---------------------------------------------------------------- the check program
SRCS = [os.path.join(ROOT, "tests", "settle_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "settle_host.cpp")]
WANT = {"volumes": 200, "refused": 6, "failures": 0}


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split() for line in r.stdout.strip().splitlines() if len(line.split()) == 2)
    assert {k: int(got[k]) for k in WANT} == WANT, r.stdout + r.stderr


def test_settle_check_program(tmp_path):
    exe = tmp_path / "settle_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe)] + SRCS)
    _run(exe)


def test_settle_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "settle_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + SRCS)
    _run(exe)
