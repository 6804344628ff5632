"""Host half of the ray queries (no GPU): the packed record layouts, bm_camera_pixel_rays against a float32 numpy restatement of the
frames' primary ray (lens radius 0, no jitter), and argument refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

EINVAL = 10001


def test_record_layouts(bm):
    from brickmap_amd import _lib
    assert C.sizeof(_lib.bm_ray) == 32 and C.sizeof(_lib.bm_ray_hit) == 32
    assert bm.RAY_DTYPE.itemsize == 32 and bm.RAY_HIT_DTYPE.itemsize == 32
    for ct, dt in ((_lib.bm_ray, bm.RAY_DTYPE), (_lib.bm_ray_hit, bm.RAY_HIT_DTYPE)):
        assert [n for n, _ in ct._fields_] == list(dt.names)
        for name, _ in ct._fields_:
            assert getattr(ct, name).offset == dt.fields[name][1], name
    rays = bm.pack_rays([[1, 2, 3]], [[0, 0, -1]])
    assert rays["tmax"][0] == np.inf and rays["reserved"][0] == 0
    words = rays.view(np.float32)
    assert list(words[:7]) == [1, 2, 3, 0, 0, -1, np.inf]


def _f(x):
    return np.float32(x)


def _normalize(v):
    return v * (_f(1.0) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def _cross(x, y):
    return np.array([x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]], np.float32)


def reference_pixel_rays(cam, W, H, px, py):
    """launch_kernels' camera basis and primary_ray's direction (traverse.h) in float32, jitter replaced by the pixel position"""
    d = np.array(cam.direction, np.float32)
    up = np.array(cam.up, np.float32)
    aspect = _f(W) / _f(H)
    right = (_normalize(_cross(d, up)) * _f(1.5)) * aspect
    upv = _normalize(_cross(right, d)) * _f(1.5)
    out = np.zeros((len(px), 3), np.float32)
    for i in range(len(px)):
        ppx, ppy = _f(px[i]) - _f(1.0), _f(py[i]) - _f(1.0)
        ni = (ppx / _f(W)) - _f(0.5)
        nj = ((_f(H) - ppy) / _f(H)) - _f(0.5)
        out[i] = _normalize((d + right * ni) + upv * nj)
    return out


@pytest.mark.parametrize("view", [((128, 32, 204.8), 0.8, -0.5, 64, 48), ((10, 500, 300), 2.5, -1.2, 1920, 1080), ((700, 20, 50), -0.3, 0.4, 333, 77)])
def test_pixel_rays_match_the_primary_ray_formula(bm, view):
    pos, h, v, W, H = view
    cam = bm.Camera(position=pos, horizontal_angle=h, vertical_angle=v).update()
    rng = np.random.default_rng(7)
    xs = np.concatenate([np.arange(W, dtype=np.float32)[:: max(1, W // 16)] + np.float32(0.5), rng.uniform(0, W, 40).astype(np.float32), [0, W]]).astype(np.float32)
    ys = np.concatenate([np.arange(H, dtype=np.float32)[:: max(1, H // 16)] + np.float32(0.5), rng.uniform(0, H, 40).astype(np.float32), [0, H]]).astype(np.float32)
    px, py = np.meshgrid(xs, ys)
    px, py = px.ravel(), py.ravel()
    rays = bm.camera_pixel_rays(cam, W, H, px, py)
    want = reference_pixel_rays(cam, W, H, px, py)
    assert np.array_equal(rays["direction"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(rays["origin"], np.tile(np.array(pos, np.float32), (len(px), 1)))
    assert np.all(rays["tmax"] == np.inf) and np.all(rays["reserved"] == 0)


def test_pixel_rays_ignore_the_lens(bm):
    cam = bm.Camera(position=(50, 60, 70), horizontal_angle=1.0, vertical_angle=-0.2).update()
    a = bm.camera_pixel_rays(cam, 64, 64, [3.5, 40.25], [7.5, 2.0])
    cam.lensRadius, cam.focalDistance = 0.5, 3.0
    b = bm.camera_pixel_rays(cam, 64, 64, [3.5, 40.25], [7.5, 2.0])
    assert a.tobytes() == b.tobytes()


def test_refusals_without_a_device(bm):
    from brickmap_amd import _lib
    L = _lib.load()
    cam = bm.Camera().update().to_c()
    px = np.zeros(4, np.float32)
    out = np.zeros(4, bm.RAY_DTYPE)
    assert L.bm_camera_pixel_rays(None, 8, 8, 4, px.ctypes.data, px.ctypes.data, out.ctypes.data) == EINVAL
    assert L.bm_camera_pixel_rays(C.byref(cam), 0, 8, 4, px.ctypes.data, px.ctypes.data, out.ctypes.data) == EINVAL
    assert L.bm_camera_pixel_rays(C.byref(cam), 8, -1, 4, px.ctypes.data, px.ctypes.data, out.ctypes.data) == EINVAL
    assert L.bm_camera_pixel_rays(C.byref(cam), 8, 8, -1, px.ctypes.data, px.ctypes.data, out.ctypes.data) == EINVAL
    assert L.bm_camera_pixel_rays(C.byref(cam), 8, 8, 4, None, px.ctypes.data, out.ctypes.data) == EINVAL
    assert L.bm_camera_pixel_rays(C.byref(cam), 8, 8, 4, px.ctypes.data, px.ctypes.data, None) == EINVAL
    assert L.bm_camera_pixel_rays(C.byref(cam), 8, 8, 0, None, None, None) == 0  # nothing to do
    assert L.bm_scene_cast_rays(None, 1, out.ctypes.data, out.ctypes.data, 0, None, None) == EINVAL
    assert b"null scene" in L.bm_last_error_string()
