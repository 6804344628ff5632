"""bm_host_reproject (csrc/reproject_host.cpp: plain loops over the rules of csrc/reproject.h) against the numpy model of the
specification (tests/_reproject_model.py), bit for bit, on a synthetic world with hand-made hit records and camera pairs -- CPU only.
And tests/reproject_check.cpp, a program with its own main that links the host routine alone, built plain and under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _reproject_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [c.name for c in model.cases()]
EINVAL = 10001


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def camera(bm, cam):
    return bm.Camera(position=cam.position, direction=cam.direction, up=cam.up)


def run(bm, c, max_history=32.0, prev_image="case", prev_keys="case"):
    prev_image = c.prev_image if isinstance(prev_image, str) else prev_image
    prev_keys = c.prev_keys if isinstance(prev_keys, str) else prev_keys
    prev = None if prev_image is None else model.history(prev_image, prev_keys)
    return bm.host_reproject(c.accum, c.hits, camera(bm, c.cur), camera(bm, c.prev), prev, max_history=max_history)


@pytest.mark.parametrize("name", CASES)
def test_host_routine_equals_the_model_bit_for_bit(bm, name):
    c = model.case(name)
    got = run(bm, c)
    image, key = model.expected(name)
    assert got.image.shape == image.shape and got.keys.shape == key.shape
    assert np.array_equal(got.keys, key), f"{name}: {np.count_nonzero(got.keys != key)} keys differ"
    assert np.array_equal(bits(got.image), bits(image)), f"{name}: {np.count_nonzero(bits(got.image) != bits(image))} words differ"


def test_the_cases_cover_the_paths():
    """what the camera pairs are for: most pixels take history where the camera moved a little, a moved camera uncovers surfaces (a tap
    with another key), and nothing takes history where the previous camera cannot have seen the point"""
    for w, h in model.SIZES:
        took = {}
        for name, _, _ in model.camera_pairs():
            c = model.case(f"{name}_{w}x{h}")
            image, key = model.expected(c.name)
            took[name] = (image[..., 3] > c.accum[..., 3]).mean()
            assert np.isfinite(image).all()
            assert (key == model.SPECIAL).any() and (key != model.SPECIAL).mean() > 0.5, "misses above the horizon, surfaces below"
        for name in ("identical", "sideways", "forward", "yaw"):
            assert took[name] > 0.4, (name, took[name])
        assert took["from_above"] > 0.02  # the floor between the towers, seen from both cameras
        for name in ("turned_round", "far_jump", "degenerate"):
            assert took[name] == 0, (name, took[name])
        # ... and some pixels of a surface start again: uncovered, off the previous image, or over history pixels without samples
        c = model.case(f"sideways_{w}x{h}")
        assert took["sideways"] < (model.expected(c.name)[1] != model.SPECIAL).mean()


def test_no_history_copies(bm):
    for name in ("sideways_33x17", "yaw_257x65"):
        c = model.case(name)
        got = run(bm, c, prev_image=None)
        assert np.array_equal(bits(got.image), bits(c.accum))
        assert np.array_equal(got.keys, model.keys(c.accum, c.hits))
        # ... also without a previous camera
        got = bm.host_reproject(c.accum, c.hits, camera(bm, c.cur), None, None)
        assert np.array_equal(bits(got.image), bits(c.accum)) and np.array_equal(got.keys, model.keys(c.accum, c.hits))


def test_previous_keys_that_all_differ_copy(bm):
    for name in ("identical_64x64", "sideways_257x65"):
        c = model.case(name)
        cur_keys = model.keys(c.accum, c.hits)
        other = np.full_like(c.prev_keys, np.uint32(int(cur_keys[cur_keys != model.SPECIAL].max()) + 8))
        got = run(bm, c, prev_keys=other)
        assert np.array_equal(bits(got.image), bits(c.accum))
        assert np.array_equal(got.keys, cur_keys)


@pytest.mark.parametrize("max_history", (1.0, 4.0, 32.0))
def test_history_is_capped(bm, max_history):
    for name in ("identical_64x64", "sideways_33x17", "forward_257x65"):
        c = model.case(name)
        got = run(bm, c, max_history=max_history)
        image, key = model.reproject(c.cur, c.prev, c.accum, c.hits, c.prev_image, c.prev_keys, max_history)
        assert np.array_equal(bits(got.image), bits(image)) and np.array_equal(got.keys, key)
        assert (got.image[..., 3] <= np.float32(max_history) + c.accum[..., 3]).all()
        assert (got.image[..., 3] == np.float32(max_history) + c.accum[..., 3]).any(), "no pixel reached the cap"


def test_a_chain_of_three_frames(bm):
    """each output is the next frame's history: the camera walks sideways, every frame has noise of its own"""
    w, h = 64, 64
    start = model.camera_pairs()[0][1]
    rng = np.random.default_rng(5)
    prev_cam, hist, want = None, None, (None, None)
    for frame in range(3):
        cam = model._moved(start, (0.5 * frame, 0.1 * frame, 0.0))
        accum = model._noisy(rng, h, w, (rng.integers(0, 12, (h, w)) > 0).astype(np.float32))
        hits = model.cast(cam, w, h)
        hist = bm.host_reproject(accum, hits, camera(bm, cam), camera(bm, prev_cam) if prev_cam else None, hist, max_history=1.5)
        want = model.reproject(cam, prev_cam, accum, hits, want[0], want[1], 1.5)
        assert np.array_equal(bits(hist.image), bits(want[0])) and np.array_equal(hist.keys, want[1]), f"frame {frame}"
        prev_cam = cam
    assert hist.image[..., 3].max() == np.float32(2.5)  # 1.5 of the history and the frame's own sample


def test_refusals(bm):
    L = bm.load()
    from brickmap_amd._lib import bm_reproject_params
    accum = np.ones((2, 2, 4), np.float32)
    hits = np.zeros(4, model.HIT_DTYPE)
    hits["distance"], hits["level"] = 10, 2
    hits["normal"][:, 2] = 1
    prev = np.ones(20, np.float32)
    out = np.full(20, -7, np.float32)
    cam = bm.Camera().to_c()

    def call(w=2, h=2, mh=32.0, flags=0, reserved=0, c=cam, cp=cam, a=accum.ctypes.data, hh=hits.ctypes.data, p=prev.ctypes.data, o=out.ctypes.data, par=True):
        pp = bm_reproject_params(w, h, mh, flags, reserved)
        return L.bm_host_reproject(C.byref(pp) if par else None, C.byref(c) if c is not None else None, C.byref(cp) if cp is not None else None, a, hh, p, o)

    for kw in (dict(w=0), dict(h=0), dict(w=-3), dict(w=65536), dict(h=65536), dict(mh=0.5), dict(mh=0.0), dict(mh=-1.0), dict(mh=float("inf")),
               dict(mh=float("nan")), dict(flags=1), dict(reserved=1), dict(c=None), dict(a=None), dict(hh=None), dict(o=None), dict(par=False),
               dict(cp=None)):
        assert call(**kw) == EINVAL, kw
        assert b"bm_host_reproject" in L.bm_last_error_string()
    assert np.all(out == -7), "a refused call wrote its output"
    assert call() == 0 and call(mh=1.0) == 0 and call(p=None, cp=None) == 0 and call(p=None) == 0
    n = C.c_size_t(0)
    assert L.bm_history_bytes(1920, 1080, C.byref(n)) == 0 and n.value == 1920 * 1080 * 20 and bm.history_bytes(3, 5) == 300
    assert L.bm_history_bytes(0, 1080, C.byref(n)) == EINVAL and L.bm_history_bytes(4, 65536, C.byref(n)) == EINVAL and L.bm_history_bytes(4, 4, None) == EINVAL


# ---- the stand-alone program: the host routine linked alone, run plain and under the sanitizers
SRCS = [os.path.join(ROOT, "tests", "reproject_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "reproject_host.cpp")]


def _run(exe, images):
    r = subprocess.run([str(exe), str(images)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_reproject_check_program(tmp_path):
    exe = tmp_path / "reproject_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe)] + SRCS)
    n = _run(exe, 40)
    assert n["images"] == 40 and n["pixels"] > 10_000 and n["special"] > 100 and n["history"] > 3_000 and n["refused"] >= 8


def test_reproject_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "reproject_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe)] + SRCS)
    n = _run(exe, 12)
    assert n["images"] == 12 and n["history"] > 500
