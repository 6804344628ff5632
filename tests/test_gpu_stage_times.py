"""The measuring doors on the MI355X -- Scene.voxelize_times, mesh_quads_times, denoise_times (bm_debug_*_times: the operator with a
hipEvent between its stages, csrc/device_ops.cpp through launch_staged of csrc/hip_owned.h) and Scene.last_label_ms: each runs the
launches of its plain call, so its results equal that call's byte for byte, and gives one finite, non-negative duration per stage.  The
durations themselves come from events and depend on the machine: they are compared with nothing."""
import ctypes as C
import math

import numpy as np
import pytest

import _voxelize_model as vmodel

pytestmark = pytest.mark.gpu
ESTATE = 10002


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def scene(bm, torch_cuda):
    """a small loaded scene: a floor of 8 voxels and a random block on it"""
    vox = np.zeros((128, 128, 128), np.uint8)
    vox[:8] = 1
    vox[8:40, :40, :40] = np.random.default_rng(5).random((32, 40, 40)) < 0.2
    s = bm.Scene.from_voxels(vox)
    yield s
    s.close()


def durations(ms, n):
    return len(ms) == n and all(math.isfinite(t) and t >= 0.0 for t in ms)


def test_voxelize_times(bm, torch_cuda, scene):
    """a closed box across the word edge of rows of 33 voxels, in a volume of 33 x 9 x 10 (nx, ny, nz)"""
    torch = torch_cuda
    tri = torch.from_numpy(np.ascontiguousarray(vmodel.box_mesh((1.25, 1.5, 1.75), (32.5, 7.5, 8.25)), np.float32).reshape(-1, 3, 3)).cuda()
    shape = (10, 9, 33)
    for mode in ("surface", "solid", "solid+surface"):
        plain, res = scene.voxelize(tri, (0, 0, 0), shape, mode=mode)
        timed, res_t, ms = scene.voxelize_times(tri, (0, 0, 0), shape, mode=mode)
        assert plain.cpu().numpy().any() and tuple(timed.shape) == shape
        assert timed.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), mode
        assert res_t.record == res.record and res.open_columns == 0, mode
        assert durations(ms, 5), ms


def test_mesh_quads_times(bm, torch_cuda, scene):
    """a solid box in a volume of 17 x 9 x 8 (nx, ny, nz): the counting call and the emitting call, or the emitting call alone"""
    torch = torch_cuda
    vol = torch.zeros((8, 9, 17), dtype=torch.uint8, device="cuda")
    vol[1:7, 2:8, 3:15] = 1
    plain = scene.mesh_quads(vol)
    assert plain.count > 0
    for capacity in (None, 64, plain.count - 1):
        want = scene.mesh_quads(vol, capacity=capacity)
        got, ms = scene.mesh_quads_times(vol, capacity=capacity)
        assert got.record == want.record == plain.record, capacity
        assert len(got.records) == (plain.count if capacity is None else min(plain.count, capacity))
        assert got.records.tobytes() == want.records.tobytes() == plain.records[:len(got.records)].tobytes(), capacity
        assert durations(ms, 3), ms


@pytest.mark.parametrize("iterations", (0, 2))
def test_denoise_times(bm, torch_cuda, scene, iterations):
    """16 x 16; bm_debug_denoise_times defines 2 + iterations durations: without a pass one kernel runs, and the second entry is 0"""
    torch = torch_cuda
    from brickmap_amd._lib import bm_denoise_params
    L = bm.load()
    w = h = 16
    rng = np.random.default_rng(7)
    accum = torch.from_numpy(np.concatenate((rng.random((h, w, 3), np.float32), np.ones((h, w, 1), np.float32)), axis=2)).cuda()
    hits = scene.pixel_hits(bm.Camera(position=(64.0, 20.0, 100.0), horizontal_angle=0.8, vertical_angle=-0.5).update(), w, h).packed
    plain = scene.denoise(accum, hits, w, h, iterations=iterations)
    timed, ms = scene.denoise_times(accum, hits, w, h, iterations=iterations)
    assert timed.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    assert durations(ms, 2 + iterations), ms
    # the C call, on an array that holds something else: every one of the 2 + iterations entries is written
    out = torch.empty_like(accum)
    ws = torch.empty(bm.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    raw = (C.c_float * (3 + iterations))(*([-1.0] * (3 + iterations)))
    par = bm_denoise_params(w, h, iterations, 4.0, 0, 0)
    assert L.bm_debug_denoise_times(scene.gpuScene, C.byref(par), C.c_void_p(accum.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(out.data_ptr()),
                                    C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream), raw) == 0
    ms = [float(v) for v in raw]
    assert durations(ms[:2 + iterations], 2 + iterations) and ms[2 + iterations] == -1.0, ms
    if iterations == 0:
        assert ms[1] == 0.0, "one kernel: the rest is 0"
    assert out.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()


def test_last_label_ms(bm, torch_cuda, scene):
    """BM_ESTATE unless the last label_region launched its kernels: on a fresh scene, after an empty box, after a box outside the world"""
    L = bm.load()

    def last(s):
        t = [C.c_float(-1.0) for _ in range(3)]
        code = L.bm_scene_last_label_ms(s.gpuScene, *[C.byref(v) for v in t])
        return code, [float(v.value) for v in t]

    fresh = bm.Scene(128, 128, device=0)
    assert last(fresh)[0] == ESTATE and b"launched nothing" in L.bm_last_error_string()
    fresh.close()
    assert last(scene)[0] == ESTATE
    for refused in (((8, 8, 4), (24, 24, 4)), ((200, 200, 200), (216, 216, 216))):   # an empty box; a box wholly outside the world
        _, count = scene.label_region((8, 8, 4), (24, 24, 20))   # 16^3 across the floor's top
        assert int(count.item()) >= 1
        code, ms = last(scene)
        assert code == 0 and durations(ms, 3), ms
        labels, count = scene.label_region(*refused)
        assert int(count.item()) == 0 and not labels.cpu().numpy().any()
        assert last(scene) == (ESTATE, [-1.0, -1.0, -1.0]) and b"launched nothing" in L.bm_last_error_string()
