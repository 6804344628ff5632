"""The a-trous filter on the MI355X (bm_denoise, csrc/denoise.hip): equal to the numpy model of the specification bit for bit -- tile edges
inside the image in both axes, every pass count that changes which kernel writes the result, `out` aliasing `accum`, another stream, a
workspace used twice; the device's pixel rays equal the host's; refusals launch nothing; and end to end on the 256^3 world a denoised
1-spp frame is closer to the 256-spp frame than the 1-spp frame is."""
import ctypes as C

import numpy as np
import pytest

import _denoise_model as model

pytestmark = pytest.mark.gpu

EINVAL = 10001
# beside the shared synthetic cases: images that the 64 x 16 tiles of the LDS kernels do not divide, with several tiles along both axes
GPU_SIZES = {"gpu_64x64": (64, 64, 201), "gpu_257x65": (65, 257, 202)}  # name: (height, width, seed)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def scene256(bm, torch_cuda):
    return bm.Scene(256, 256, device=0).generate().preload_all()


_cache = {}


def case(name):
    if name in GPU_SIZES:
        if name not in _cache:
            h, w, seed = GPU_SIZES[name]
            _cache[name] = model.scene_case(seed, h, w)
        return _cache[name]
    return next(c for c in model.cases() if c[0] == name)[1:]


def want(name, iterations):
    key = (name, iterations)
    if key not in _cache:
        accum, hits = case(name)
        _cache[key] = model.expected(name, iterations) if name not in GPU_SIZES else model.denoise(accum, hits, iterations, 4.0)
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def upload(torch, accum, hits):
    h, w = accum.shape[:2]
    return (torch.from_numpy(accum).cuda(), torch.from_numpy(hits.view(np.float32).reshape(h * w, 8).copy()).cuda(), w, h)


NAMES = [c[0] for c in model.cases()] + list(GPU_SIZES)


@pytest.mark.parametrize("iterations", (5, 8))
@pytest.mark.parametrize("name", NAMES)
def test_device_filter_equals_the_model_bit_for_bit(scene256, torch_cuda, name, iterations):
    accum, hits = case(name)
    d_accum, d_hits, w, h = upload(torch_cuda, accum, hits)
    out = scene256.denoise(d_accum, d_hits, w, h, iterations=iterations)
    got = out.cpu().numpy()
    exp = want(name, iterations)
    assert got.shape == exp.shape
    assert np.array_equal(bits(got), bits(exp)), f"{name}: {np.count_nonzero(bits(got) != bits(exp))} words differ"
    assert np.array_equal(bits(d_accum.cpu().numpy()), bits(accum)), "the input was written"


@pytest.mark.parametrize("iterations", (0, 1, 2, 3, 4))
def test_every_pass_count_writes_the_result(scene256, torch_cuda, iterations):
    """the last pass writes `out`: with 0 passes that is the prepare kernel, with 1 or 2 an LDS pass, from 3 on a pass that reads global memory"""
    name = "gpu_257x65"
    d_accum, d_hits, w, h = upload(torch_cuda, *case(name))
    got = scene256.denoise(d_accum, d_hits, w, h, iterations=iterations).cpu().numpy()
    assert np.array_equal(bits(got), bits(want(name, iterations)))


def test_out_may_be_accum_and_another_stream(scene256, torch_cuda):
    torch = torch_cuda
    name = "gpu_257x65"
    d_accum, d_hits, w, h = upload(torch, *case(name))
    side = torch.cuda.Stream()
    out = scene256.denoise(d_accum, d_hits, w, h, iterations=5, out=d_accum, stream=side.cuda_stream)
    assert out.data_ptr() == d_accum.data_ptr()
    side.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want(name, 5)))


def test_one_workspace_two_calls_and_the_timing_door(bm, scene256, torch_cuda):
    """bm_denoise on the caller's workspace: two different images in a row through one workspace (no state survives a call), then the
    measuring door, which runs the same launches"""
    torch = torch_cuda
    from brickmap_amd._lib import bm_denoise_params
    L = bm.load()
    big, small = "gpu_257x65", "gpu_64x64"
    ws = torch.empty(bm.denoise_workspace_bytes(257, 65), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for name in (big, small, big):
        d_accum, d_hits, w, h = upload(torch, *case(name))
        out = torch.empty_like(d_accum)
        par = bm_denoise_params(w, h, 5, 4.0, 0, 0)
        assert L.bm_denoise(scene256.gpuScene, C.byref(par), C.c_void_p(d_accum.data_ptr()), C.c_void_p(d_hits.data_ptr()), C.c_void_p(out.data_ptr()),
                            C.c_void_p(ws.data_ptr()), ws.numel(), stream) == 0
        outs.append((name, out, d_accum, d_hits))
    torch.cuda.synchronize()
    for name, out, _, _ in outs:
        assert np.array_equal(bits(out.cpu().numpy()), bits(want(name, 5))), name
    d_accum, d_hits, w, h = upload(torch, *case(big))
    out, ms = scene256.denoise_times(d_accum, d_hits, w, h, iterations=5)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want(big, 5)))
    assert len(ms) == 7 and all(t > 0 for t in ms)


def test_refusals_launch_nothing(bm, scene256, torch_cuda):
    torch = torch_cuda
    from brickmap_amd._lib import bm_denoise_params
    L = bm.load()
    w, h = 20, 10
    accum = torch.ones((h, w, 4), device="cuda")
    hits = torch.zeros((h * w, 8), device="cuda")
    out = torch.full((h, w, 4), -7.0, device="cuda")
    need = bm.denoise_workspace_bytes(w, h)
    assert need == w * h * 36
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(it=5, sigma=4.0, ww=w, hh=h, flags=0, reserved=0, a=accum.data_ptr(), hp=hits.data_ptr(), o=out.data_ptr(), wsp=ws.data_ptr(), wsb=need, par=True):
        p = bm_denoise_params(ww, hh, it, sigma, flags, reserved)
        return L.bm_denoise(scene256.gpuScene, C.byref(p) if par else None, C.c_void_p(a), C.c_void_p(hp), C.c_void_p(o), C.c_void_p(wsp), wsb, stream)

    its, sigma, size, zero, null, small = (b"iterations must be 0 ... 8", b"sigma_l must be finite and positive", b"width and height must be 1 ... 65535",
                                          b"flags and reserved must be 0", b"null", b"smaller than")
    for kw, fragment in ((dict(it=-1), its), (dict(it=9), its), (dict(sigma=0.0), sigma), (dict(sigma=-4.0), sigma), (dict(sigma=float("inf")), sigma),
                         (dict(sigma=float("nan")), sigma), (dict(ww=0), size), (dict(hh=0), size), (dict(ww=65536), size), (dict(hh=65536), size),
                         (dict(flags=1), zero), (dict(reserved=7), zero),
                         (dict(a=None), null), (dict(hp=None), null), (dict(o=None), null), (dict(wsp=None), null), (dict(wsb=need - 1), small), (dict(wsb=0), small),
                         (dict(par=False), null), (dict(wsp=ws.data_ptr() + 4), b"aligned"), (dict(o=ws.data_ptr()), b"overlaps")):
        assert call(**kw) == EINVAL, kw
        msg = L.bm_last_error_string()
        assert msg.startswith(b"bm_denoise: ") and fragment in msg, (kw, msg)  # which refusal fired
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote its output"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[..., 3] == 1.0).all())


VIEWS = [((128, 32, 204.8), 0.8, -0.5), ((20, 20, 200), 0.7, -0.7), ((230, 200, 120), -2.4, -0.35)]


def test_device_pixel_rays_equal_the_host_rays(bm, scene256, torch_cuda):
    w, h = 33, 17
    px, py = np.meshgrid(np.arange(w, dtype=np.float32) + np.float32(0.5), np.arange(h, dtype=np.float32) + np.float32(0.5))
    cams = [bm.Camera(position=p, horizontal_angle=a, vertical_angle=v).update() for p, a, v in VIEWS]
    cams.append(bm.Camera(position=(100.5, 60.25, 300.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)))  # axis-aligned: straight down
    for cam in cams:
        host = bm.camera_pixel_rays(cam, w, h, px.ravel(), py.ravel())
        dev = scene256.pixel_rays(cam, w, h).cpu().numpy()
        assert dev.shape == (w * h, 8)
        assert np.array_equal(dev.view(np.uint32), host.view(np.uint32).reshape(w * h, 8)), "device pixel rays differ from bm_camera_pixel_rays"
    L = bm.load()
    c = cams[0].to_c()
    buf = torch_cuda.empty((4, 8), device="cuda")
    for ww, hh, ptr in ((0, 2, buf.data_ptr()), (2, 65536, buf.data_ptr()), (2, 2, None), (2, 2, buf.data_ptr() + 4)):
        assert L.bm_camera_pixel_rays_device(scene256.gpuScene, C.byref(c), ww, hh, C.c_void_p(ptr), None) == EINVAL


def radiance(accum):
    return np.stack(model.radiance(accum), axis=-1)


def test_denoised_frame_is_closer_to_the_converged_frame(bm, scene256, torch_cuda):
    """128 x 72 on the preloaded 256^3 world: a 1-spp frame, its guides from pixel_hits, and a 256-spp frame of the same view (other
    samples).  Over the filtered pixels the denoised frame's RMSE against the 256-spp frame is below the 1-spp frame's; special pixels
    are rgb / n bit for bit.  (The measured ratio is in profiles/denoise_quality.txt; no ratio is asserted.)"""
    torch = torch_cuda
    w, h = 128, 72
    cam = bm.Camera(position=(128, 32, 204.8), horizontal_angle=0.8, vertical_angle=-0.5).update()
    one = torch.zeros((h, w, 4), device="cuda")
    ref = torch.zeros((h, w, 4), device="cuda")
    scene256.render(cam, bm.FrameParams(w, h, spp=1), one)
    scene256.render(cam, bm.FrameParams(w, h, spp=256, sample_base=1), ref)
    hits = scene256.pixel_hits(cam, w, h)
    assert hits.packed.shape == (w * h, 8)
    out = scene256.denoise(one, hits, w, h)
    torch.cuda.synchronize()
    a1, a256, den = one.cpu().numpy(), ref.cpu().numpy(), out.cpu().numpy()
    rec = hits.packed.cpu().numpy().view(model.HIT_DTYPE).reshape(-1)
    special = model.keys(a1, rec) == model.SPECIAL
    assert (~special).mean() >= 0.25, f"only {(~special).mean():.2f} of the pixels are filtered: choose another view"
    c1, c256 = radiance(a1), radiance(a256)
    assert np.array_equal(bits(den[special][:, :3]), bits(c1[special])) and np.all(den[..., 3] == 1)
    assert np.isfinite(den).all()
    rmse = lambda a: float(np.sqrt(np.mean((a[~special].astype(np.float64) - c256[~special]) ** 2)))
    before, after = rmse(c1), rmse(den[..., :3])
    print(f"filtered pixels {(~special).mean():.3f}, RMSE against 256 spp: 1 spp {before:.4f}, denoised {after:.4f}, ratio {after / before:.3f}")
    assert after < before
    # ... and it is the filter of the specification that ran
    assert np.array_equal(bits(den), bits(model.denoise(a1, rec, 5, 4.0)))


def test_denoise_then_resolve(bm, scene256, torch_cuda):
    torch = torch_cuda
    w, h = 96, 40
    cam = bm.Camera(position=(20, 20, 200), horizontal_angle=0.7, vertical_angle=-0.7).update()
    accum = torch.zeros((h, w, 4), device="cuda")
    scene256.render(cam, bm.FrameParams(w, h, spp=1), accum)
    img = scene256.resolve(scene256.denoise(accum, scene256.pixel_hits(cam, w, h), w, h))
    torch.cuda.synchronize()
    assert tuple(img.shape) == (h, w, 4) and bool(torch.isfinite(img).all()) and bool((img[..., 3] == 1).all())
