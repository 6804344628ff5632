"""Temporal accumulation on the MI355X (bm_reproject, csrc/reproject.hip): equal to the numpy model of the specification bit for bit on
every camera pair and size of tests/_reproject_model.py; inputs unwritten; a NULL history copies; another stream; refusals launch nothing;
and end to end on the 256^3 world, eight 1-spp frames of a camera that walks sideways through TemporalAccumulator -- every frame equal to
the model, the last one closer to the 256-spp frame than its own 1-spp frame is; the history image goes through denoise and resolve."""
import ctypes as C

import numpy as np
import pytest

import _reproject_model as model

pytestmark = pytest.mark.gpu

EINVAL = 10001
CASES = [c.name for c in model.cases()]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def scene256(bm, torch_cuda):
    return bm.Scene(256, 256, device=0).generate().preload_all()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def camera(bm, cam):
    return bm.Camera(position=cam.position, direction=cam.direction, up=cam.up)


def upload(bm, torch, c, with_history=True):
    w, h = c.accum.shape[1], c.accum.shape[0]
    accum = torch.from_numpy(c.accum).cuda()
    hits = torch.from_numpy(c.hits.view(np.float32).reshape(h * w, 8).copy()).cuda()
    prev = bm.History(torch.from_numpy(model.history(c.prev_image, c.prev_keys)).cuda(), w, h) if with_history else None
    return accum, hits, prev, w, h


def keys_of(history):
    return history.keys.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_model_bit_for_bit(bm, scene256, torch_cuda, name):
    c = model.case(name)
    accum, hits, prev, w, h = upload(bm, torch_cuda, c)
    out = scene256.reproject(accum, hits, camera(bm, c.cur), camera(bm, c.prev), prev, w, h)
    image, key = model.expected(name)
    got = out.image.cpu().numpy()
    assert got.shape == image.shape
    assert np.array_equal(keys_of(out), key), f"{name}: {np.count_nonzero(keys_of(out) != key)} keys differ"
    assert np.array_equal(bits(got), bits(image)), f"{name}: {np.count_nonzero(bits(got) != bits(image))} words differ"
    assert np.array_equal(bits(accum.cpu().numpy()), bits(c.accum)), "accum was written"
    assert np.array_equal(hits.cpu().numpy().view(np.uint32), c.hits.view(np.uint32).reshape(h * w, 8)), "hits were written"
    assert np.array_equal(bits(prev.buffer.cpu().numpy()), bits(model.history(c.prev_image, c.prev_keys))), "the previous history was written"


def test_other_caps(bm, scene256, torch_cuda):
    c = model.case("sideways_257x65")
    accum, hits, prev, w, h = upload(bm, torch_cuda, c)
    for max_history in (1.0, 4.0):
        out = scene256.reproject(accum, hits, camera(bm, c.cur), camera(bm, c.prev), prev, w, h, max_history=max_history)
        image, _ = model.reproject(c.cur, c.prev, c.accum, c.hits, c.prev_image, c.prev_keys, max_history)
        assert np.array_equal(bits(out.image.cpu().numpy()), bits(image))


def test_null_history_copies(bm, scene256, torch_cuda):
    c = model.case("sideways_257x65")
    accum, hits, _, w, h = upload(bm, torch_cuda, c, with_history=False)
    for prev_camera in (camera(bm, c.prev), None):
        out = scene256.reproject(accum, hits, camera(bm, c.cur), prev_camera, None, w, h)
        assert np.array_equal(bits(out.image.cpu().numpy()), bits(c.accum))
        assert np.array_equal(keys_of(out), model.keys(c.accum, c.hits))


def test_another_stream_and_a_given_output(bm, scene256, torch_cuda):
    torch = torch_cuda
    c = model.case("yaw_257x65")
    accum, hits, prev, w, h = upload(bm, torch, c)
    mine = bm.History(torch.zeros(5 * w * h, device="cuda"), w, h)
    side = torch.cuda.Stream()
    out = scene256.reproject(accum, hits, camera(bm, c.cur), camera(bm, c.prev), prev, w, h, out=mine, stream=side.cuda_stream)
    assert out is mine
    side.synchronize()
    image, key = model.expected(c.name)
    assert np.array_equal(bits(out.image.cpu().numpy()), bits(image)) and np.array_equal(keys_of(out), key)


def test_refusals_launch_nothing(bm, scene256, torch_cuda):
    torch = torch_cuda
    from brickmap_amd._lib import bm_reproject_params
    L = bm.load()
    w, h = 20, 10
    n = w * h
    assert bm.history_bytes(w, h) == 20 * n
    accum = torch.ones((h, w, 4), device="cuda")
    hits = torch.zeros((n, 8), device="cuda")
    prev = torch.ones(5 * n + 16, device="cuda")
    out = torch.full((5 * n + 16,), -7.0, device="cuda")
    cam = bm.Camera().to_c()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ww=w, hh=h, mh=32.0, flags=0, reserved=0, c=cam, cp=cam, a=accum.data_ptr(), hp=hits.data_ptr(), p=prev.data_ptr(), o=out.data_ptr(), par=True):
        pp = bm_reproject_params(ww, hh, mh, flags, reserved)
        return L.bm_reproject(scene256.gpuScene, C.byref(pp) if par else None, C.byref(c) if c is not None else None, C.byref(cp) if cp is not None else None,
                              C.c_void_p(a), C.c_void_p(hp), C.c_void_p(p), C.c_void_p(o), stream)

    size, cap, zero, null, aligned, overlaps = (b"width and height must be 1 ... 65535", b"max_history must be finite and at least 1", b"flags and reserved must be 0",
                                                b"null", b"aligned", b"overlaps")
    for kw, fragment in ((dict(ww=0), size), (dict(hh=0), size), (dict(ww=65536), size), (dict(hh=65536), size), (dict(mh=0.5), cap), (dict(mh=-2.0), cap),
                         (dict(mh=float("inf")), cap), (dict(mh=float("nan")), cap), (dict(flags=1), zero), (dict(reserved=7), zero),
                         (dict(c=None), null), (dict(a=None), null), (dict(hp=None), null), (dict(o=None), null), (dict(par=False), null),
                         (dict(cp=None), b"a previous history needs the camera it was made with"),
                         (dict(o=out.data_ptr() + 4), aligned), (dict(a=accum.data_ptr() + 8), aligned), (dict(hp=hits.data_ptr() + 4), aligned), (dict(p=prev.data_ptr() + 4), aligned),
                         # history_out overlapping the previous history (the same, and its last 16 bytes), accum and hits
                         (dict(p=out.data_ptr()), overlaps), (dict(p=out.data_ptr() + 20 * n - 16), overlaps), (dict(p=out.data_ptr() - 20 * n + 16), overlaps),
                         (dict(a=out.data_ptr() + 16 * n), overlaps), (dict(hp=out.data_ptr() + 16), overlaps)):
        assert call(**kw) == EINVAL, kw
        msg = L.bm_last_error_string()
        assert msg.startswith(b"bm_reproject: ") and fragment in msg, (kw, msg)  # which refusal fired
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote its output"
    assert call() == 0 and call(p=None, cp=None) == 0
    torch.cuda.synchronize()
    assert bool((out[:4 * n] == 1.0).all()) and bool((out[5 * n:] == -7.0).all())


def sideways(bm, cam, step):
    d = np.asarray(cam.direction, np.float64)
    side = np.cross(d, (0.0, 0.0, 1.0))
    side /= np.linalg.norm(side)
    return bm.Camera(position=tuple(float(p + step * s) for p, s in zip(cam.position, side)), direction=cam.direction, up=cam.up)


def as_model_camera(cam):
    return model.Cam(tuple(cam.position), tuple(cam.direction), tuple(cam.up))


def test_moving_camera_end_to_end(bm, scene256, torch_cuda):
    """128 x 72 on the preloaded 256^3 world, 8 frames: the camera starts at the view of test_denoised_frame_is_closer_to_the_converged_frame
    and moves half a voxel sideways per frame; every frame is 1 spp with samples of its own into a zeroed buffer, fed through
    TemporalAccumulator.  Every frame's history equals the model applied to the downloaded inputs, bit for bit.  Over the pixels of the
    last frame that took history -- at least a quarter of the image -- the RMSE of rgb / n against 256 spp of the last view (other samples)
    is below the 1-spp frame's.  (The measured ratio is in profiles/reproject_quality.txt; no ratio is asserted.)"""
    torch = torch_cuda
    w, h, frames = 128, 72, 8
    start = bm.Camera(position=(128, 32, 204.8), horizontal_angle=0.8, vertical_angle=-0.5).update()
    temporal = bm.TemporalAccumulator(scene256, w, h)
    prev_cam, prev_image, prev_keys = None, None, None
    for k in range(frames):
        cam = sideways(bm, start, 0.5 * k)
        one = torch.zeros((h, w, 4), device="cuda")
        scene256.render(cam, bm.FrameParams(w, h, spp=1, sample_base=k), one)
        hits = scene256.pixel_hits(cam, w, h)
        image = temporal.add(cam, one, hits)
        torch.cuda.synchronize()
        a1 = one.cpu().numpy()
        rec = hits.packed.cpu().numpy().view(model.HIT_DTYPE).reshape(-1)
        got, got_keys = image.cpu().numpy(), keys_of(temporal.history)
        want, want_keys = model.reproject(as_model_camera(cam), as_model_camera(prev_cam) if prev_cam else None, a1, rec, prev_image, prev_keys, 32.0)
        assert np.array_equal(got_keys, want_keys), f"frame {k}: keys"
        assert np.array_equal(bits(got), bits(want)), f"frame {k}: {np.count_nonzero(bits(got) != bits(want))} words differ"
        prev_cam, prev_image, prev_keys = cam, got, got_keys
    ref = torch.zeros((h, w, 4), device="cuda")
    scene256.render(cam, bm.FrameParams(w, h, spp=256, sample_base=1000), ref)
    torch.cuda.synchronize()
    a256 = ref.cpu().numpy()
    took = got[..., 3] > a1[..., 3]
    assert took.mean() >= 0.25, f"only {took.mean():.2f} of the pixels took history: choose another path"
    assert np.isfinite(got).all()
    with np.errstate(all="ignore"):
        c1, ch, c256 = a1[..., :3] / a1[..., 3:], got[..., :3] / got[..., 3:], np.where(a256[..., 3:] > 0, a256[..., :3] / a256[..., 3:], 0)
    rmse = lambda a: float(np.sqrt(np.mean((a[took].astype(np.float64) - c256[took]) ** 2)))
    before, after = rmse(c1), rmse(ch)
    print(f"pixels with history {took.mean():.3f}, mean samples {got[..., 3][took].mean():.2f}, RMSE against 256 spp: 1 spp {before:.4f}, "
          f"reprojected {after:.4f}, ratio {after / before:.3f}")
    assert after < before
    # reset() forgets: the next frame is the frame alone
    temporal.reset()
    again = temporal.add(cam, one, hits)
    assert np.array_equal(bits(again.cpu().numpy()), bits(a1))


def test_history_image_through_denoise_and_resolve(bm, scene256, torch_cuda):
    torch = torch_cuda
    w, h = 96, 40
    start = bm.Camera(position=(20, 20, 200), horizontal_angle=0.7, vertical_angle=-0.7).update()
    temporal = bm.TemporalAccumulator(scene256, w, h, max_history=8.0)
    for k in range(3):
        cam = sideways(bm, start, 0.5 * k)
        accum = torch.zeros((h, w, 4), device="cuda")
        scene256.render(cam, bm.FrameParams(w, h, spp=1, sample_base=k), accum)
        image = temporal.add(cam, accum)  # the guides are made inside
    assert float(image[..., 3].max()) > 2.0
    img = scene256.resolve(scene256.denoise(image, scene256.pixel_hits(cam, w, h), w, h))
    torch.cuda.synchronize()
    assert tuple(img.shape) == (h, w, 4) and bool(torch.isfinite(img).all()) and bool((img[..., 3] == 1).all())
