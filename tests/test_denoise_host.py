"""bm_host_denoise (csrc/denoise_host.cpp: plain loops over the rules of csrc/denoise.h) against the numpy model of the specification
(tests/_denoise_model.py), bit for bit, on synthetic images with hand-made hit records -- CPU only.  And tests/denoise_check.cpp, a program
with its own main that links the host filter alone, built plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _denoise_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [c[0] for c in model.cases()]
ITERATIONS = (0, 1, 5, 6)  # 6: the last pass has step 32, beyond every image but one


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("name", CASES)
def test_host_filter_equals_the_model_bit_for_bit(bm, name, iterations):
    _, accum, hits = next(c for c in model.cases() if c[0] == name)
    got = bm.host_denoise(accum, hits, iterations=iterations, sigma_l=4.0)
    want = model.expected(name, iterations)
    assert got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), f"{name}: {np.count_nonzero(bits(got) != bits(want))} words differ"
    assert np.isfinite(got).all()


def test_other_sigma(bm):
    _, accum, hits = next(c for c in model.cases() if c[0] == "scene_70x37")
    for sigma in (0.5, 37.0):
        assert np.array_equal(bits(bm.host_denoise(accum, hits, iterations=3, sigma_l=sigma)), bits(model.denoise(accum, hits, 3, sigma)))


def test_keys_of_shared_planes_and_directions():
    """levels 0, 1, 2 whose entry faces lie in one plane get one key; the six directions of one voxel get six keys; and the plane is that of
    the ENTRY face: a positive normal (the ray came from the positive side) means the cell's high face"""
    accum = np.ones((1, 9, 4), np.float32)
    hits = model.make_hits(1, 9)
    for i, (lvl, size) in enumerate(((0, 8), (1, 4), (2, 1))):
        hits["normal"][i], hits["voxel"][i], hits["level"][i] = (0, 0, 1), (8 * i, 3, 64 - size), lvl          # high faces at z = 64
        hits["normal"][3 + i], hits["voxel"][3 + i], hits["level"][3 + i] = (0, 0, -1), (8 * i, 3, 64), lvl    # low faces at z = 64
    hits["normal"][6], hits["voxel"][6], hits["level"][6] = (0, 1, 0), (0, 63, 0), 2   # y = 64, not z = 64
    hits["normal"][7], hits["voxel"][7], hits["level"][7] = (0, 0, 1), (0, 0, 64), 2   # high face of voxel 64: z = 65
    hits["normal"][8], hits["voxel"][8], hits["level"][8] = (0, 0, 0), (0, 0, 63), 2   # started inside a voxel: special
    k = model.keys(accum, hits)[0]
    assert k[0] == k[1] == k[2] == 64 * 8 + 2 * 2 + 1
    assert k[3] == k[4] == k[5] == 64 * 8 + 2 * 2 + 0
    assert k[6] == 64 * 8 + 1 * 2 + 1 and k[7] == 65 * 8 + 2 * 2 + 1 and k[8] == model.SPECIAL
    six = model.make_hits(1, 6)
    six["normal"] = model.NORMALS
    assert len(set(model.keys(np.ones((1, 6, 4), np.float32), six)[0].tolist())) == 6


def test_shared_plane_is_filtered_as_one_surface(bm):
    """... and the library agrees: three pixels of levels 0, 1, 2 on one plane are averaged, a fourth on the plane's other side is not"""
    accum = np.array([[[1, 1, 1, 1], [2, 2, 2, 1], [4, 4, 4, 1], [64, 64, 64, 1]]], np.float32)
    hits = model.make_hits(1, 4)
    for i, (lvl, size) in enumerate(((0, 8), (1, 4), (2, 1))):
        hits["voxel"][i], hits["level"][i] = (8 * i, 3, 64 - size), lvl
    hits["normal"][3], hits["voxel"][3] = (0, 0, -1), (5, 3, 64)
    out = bm.host_denoise(accum, hits, iterations=1)
    assert np.array_equal(bits(out), bits(model.denoise(accum, hits, 1)))
    assert np.all(out[0, 3, :3] == 64) and np.all(out[0, :3, :3] > 1) and np.all(out[0, :3, :3] < 4)


@pytest.mark.parametrize("iterations", (0, 5))
def test_special_pixels_and_lone_pixels_keep_their_value(bm, iterations):
    for name in ("scene_70x37", "scene_129x3"):
        _, accum, hits = next(c for c in model.cases() if c[0] == name)
        out = bm.host_denoise(accum, hits, iterations=iterations)
        special = model.keys(accum, hits) == model.SPECIAL
        assert special.sum() > 10
        c = np.stack(model.radiance(accum) + [np.ones(accum.shape[:2], np.float32)], axis=-1)
        assert np.array_equal(bits(out[special]), bits(c[special]))
        # the pixel whose key no other pixel carries: its radiance (1.5, 1, 0.5) survives every pass exactly
        assert np.array_equal(out[-1, -1], np.array([1.5, 1.0, 0.5, 1.0], np.float32))
        if iterations == 0:
            assert np.array_equal(bits(out), bits(c))


def test_constant_image_stays_constant(bm):
    _, accum, hits = next(c for c in model.cases() if c[0] == "constant_17x12")
    out = bm.host_denoise(accum, hits, iterations=5)
    assert np.all(out == np.array([0.75, 0.5, 0.25, 1], np.float32))


def test_filter_reduces_noise(bm):
    """not a quality bar, only that it filters: on one surface of exponential noise the deviation from the mean shrinks"""
    _, accum, hits = next(c for c in model.cases() if c[0] == "noisy_40x33")
    c = accum[..., :3] / accum[..., 3:]
    out = bm.host_denoise(accum, hits, iterations=5)[..., :3]
    assert out.std() < 0.5 * c.std()


def test_refusals(bm):
    L = bm.load()
    from brickmap_amd._lib import bm_denoise_params
    accum = np.ones((2, 2, 4), np.float32)
    hits = model.make_hits(2, 2)
    out = np.zeros_like(accum)

    def call(w=2, h=2, it=5, sigma=4.0, flags=0, reserved=0, a=accum.ctypes.data, hh=hits.ctypes.data, o=out.ctypes.data, par=True):
        p = bm_denoise_params(w, h, it, sigma, flags, reserved)
        return L.bm_host_denoise(C.byref(p) if par else None, a, hh, o)

    assert call() == 0
    EINVAL = 10001
    for kw in (dict(it=-1), dict(it=9), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("inf")), dict(sigma=float("nan")),
               dict(w=0), dict(h=0), dict(w=-3), dict(w=65536), dict(h=65536), dict(flags=1), dict(reserved=1),
               dict(a=None), dict(hh=None), dict(o=None), dict(par=False)):
        assert call(**kw) == EINVAL, kw
        assert b"bm_host_denoise" in L.bm_last_error_string()
    assert call(it=8) == 0 and call(it=0) == 0
    n = C.c_size_t(0)
    assert L.bm_denoise_workspace_bytes(1920, 1080, C.byref(n)) == 0 and n.value == 1920 * 1080 * 36
    assert L.bm_denoise_workspace_bytes(0, 1080, C.byref(n)) == EINVAL and L.bm_denoise_workspace_bytes(4, 4, None) == EINVAL


# ---- the stand-alone program: the host filter linked alone, run plain and under the sanitizers
SRCS = [os.path.join(ROOT, "tests", "denoise_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "denoise_host.cpp")]


def _run(exe, images):
    r = subprocess.run([str(exe), str(images)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_denoise_check_program(tmp_path):
    exe = tmp_path / "denoise_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe)] + SRCS)
    n = _run(exe, 40)
    assert n["images"] == 40 and n["pixels"] > 10_000 and n["special"] > 100 and n["filtered"] > 5_000 and n["refused"] >= 8


def test_denoise_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "denoise_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe)] + SRCS)
    n = _run(exe, 12)
    assert n["images"] == 12 and n["filtered"] > 1_000
