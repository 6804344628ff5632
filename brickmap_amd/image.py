"""What happens to an accumulation buffer after the frames: the a-trous filter (bm_denoise), temporal accumulation for a moving camera
(bm_reproject) with its `History` and `TemporalAccumulator`, their host-only doors, and the Scene methods that issue them."""
import ctypes as C
from dataclasses import replace

import numpy as np

from . import _lib
from ._handoff import Handoff
from ._lib import check, size_call, stage_call
from .queries import RayHits


def denoise_workspace_bytes(width, height):
    """bm_denoise_workspace_bytes: device memory bm_denoise needs beside its images (36 bytes per pixel)."""
    return size_call("bm_denoise_workspace_bytes", int(width), int(height))


def _host_frame(accum, hits, width, height):
    """(accum, hits, width, height, pixels) of a host door: contiguous arrays of one frame; width / height default to accum's shape"""
    accum = np.ascontiguousarray(accum, np.float32)
    if width is None or height is None:
        assert accum.ndim == 3 and accum.shape[2] == 4, "accum: [height, width, 4], or pass width and height"
        height, width = accum.shape[:2]
    hits = np.ascontiguousarray(hits)
    n = max(int(width), 0) * max(int(height), 0)
    assert accum.size == 4 * n and hits.nbytes == 32 * n, "accum: 4 floats per pixel; hits: one 32-byte record per pixel"
    return accum, hits, width, height, n


def _device_frame(accum, hits, width, height):
    """(packed hits, pixels) of a call on the device, after the checks of its frame: accum and the hit records of width x height pixels"""
    import torch
    hits = hits.packed if isinstance(hits, RayHits) else hits
    n = int(width) * int(height)
    assert accum.is_cuda and accum.dtype == torch.float32 and accum.is_contiguous() and accum.numel() == 4 * n, "accum: float32 [height, width, 4] on the GPU"
    assert hits.is_cuda and hits.dtype == torch.float32 and hits.is_contiguous() and hits.numel() == 8 * n, "hits: the packed records, float32 [height * width, 8]"
    return hits, n


def host_denoise(accum, hits, width=None, height=None, iterations=5, sigma_l=4.0, flags=0, reserved=0):
    """bm_host_denoise (host only, no device): the a-trous filter of Scene.denoise as plain loops.  accum: float32 [height, width, 4]
    (R, G, B, n); hits: a RAY_HIT_DTYPE array of height * width records (or float32 [height * width, 8]).  width / height default to
    accum's shape.  Returns float32 [height, width, 4] = (c, 1)."""
    accum, hits, width, height, n = _host_frame(accum, hits, width, height)
    out = np.zeros((max(int(height), 0), max(int(width), 0), 4), np.float32)
    par = _lib.bm_denoise_params(int(width), int(height), int(iterations), float(sigma_l), int(flags), int(reserved))
    check(_lib.load().bm_host_denoise(C.byref(par), accum.ctypes.data, hits.ctypes.data, out.ctypes.data))
    return out


def history_bytes(width, height):
    """bm_history_bytes: bytes of a history of Scene.reproject -- a float4 image, then the surface keys (20 bytes per pixel)."""
    return size_call("bm_history_bytes", int(width), int(height))


class History:
    """A history of Scene.reproject / host_reproject: `buffer`, 5 * height * width 32-bit words (a float32 torch CUDA tensor or numpy
    array), and two views of it -- `image`, float32 [height, width, 4] = (R, G, B, n), an accumulation buffer that Scene.denoise and
    Scene.resolve take unchanged, and `keys`, the surface keys [height, width] (torch: int32 bits; numpy: uint32)."""

    def __init__(self, buffer, width, height):
        n = int(width) * int(height)
        assert buffer.ndim == 1 and buffer.shape[0] == 5 * n, "a history: 5 float32 words per pixel"
        self.buffer, self.width, self.height = buffer, int(width), int(height)
        self.image = buffer[:4 * n].reshape(int(height), int(width), 4)
        if isinstance(buffer, np.ndarray):
            self.keys = buffer[4 * n:].view(np.uint32).reshape(int(height), int(width))
        else:
            import torch
            self.keys = buffer[4 * n:].view(torch.int32).reshape(int(height), int(width))


def host_reproject(accum, hits, camera, prev_camera=None, history_prev=None, width=None, height=None, max_history=32.0, flags=0, reserved=0):
    """bm_host_reproject (host only, no device): the temporal accumulation of Scene.reproject as plain loops.  accum: float32 [height,
    width, 4] (R, G, B, n) of the frame of `camera`; hits: a RAY_HIT_DTYPE array of height * width records; history_prev: the History
    (numpy) of the frame of `prev_camera`, or None.  width / height default to accum's shape.  Returns a History (numpy)."""
    accum, hits, width, height, n = _host_frame(accum, hits, width, height)
    prev = None
    if history_prev is not None:
        prev = np.ascontiguousarray(history_prev.buffer if isinstance(history_prev, History) else history_prev, np.float32)
        assert prev.size == 5 * n, "history_prev: 5 words per pixel"
    out = History(np.zeros(5 * n, np.float32), max(int(width), 0), max(int(height), 0))
    par = _lib.bm_reproject_params(int(width), int(height), float(max_history), int(flags), int(reserved))
    c, cp = camera.to_c(), (prev_camera.to_c() if prev_camera is not None else None)
    check(_lib.load().bm_host_reproject(C.byref(par), C.byref(c), C.byref(cp) if cp is not None else None, accum.ctypes.data, hits.ctypes.data,
                                        prev.ctypes.data if prev is not None else None, out.buffer.ctypes.data))
    return out


class _ImageMethods:
    """Scene's methods on accumulation buffers.  The scene only names the GPU."""

    def _denoise(self, accum, hits, width, height, iterations, sigma_l, out, stream, times):
        import torch
        hits, n = _device_frame(accum, hits, width, height)
        h = Handoff(accum, stream)
        with h.on_target():
            if out is None:
                out = torch.empty_like(accum)
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == 4 * n, "out: like accum"
            ws = torch.empty(denoise_workspace_bytes(width, height), dtype=torch.uint8, device=accum.device)
        h.reads(accum, hits, out)
        par = _lib.bm_denoise_params(int(width), int(height), int(iterations), float(sigma_l), 0, 0)
        args = (self.gpuScene, C.byref(par), C.c_void_p(accum.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                C.c_void_p(h.handle))
        return out, stage_call(self._L.bm_denoise, self._L.bm_debug_denoise_times, args, 2 + max(int(iterations), 0) if times else None)

    def denoise(self, accum, hits, width, height, iterations=5, sigma_l=4.0, out=None, stream=None):
        """bm_denoise: the edge-avoiding a-trous filter of an accumulation buffer `accum` (float32 [height, width, 4]: R, G, B,
        n), guided by `hits` (Scene.pixel_hits, or its .packed tensor).  Returns (c, 1) per pixel -- what Scene.resolve takes -- in `out`
        (None = a new tensor; may be accum itself).  The workspace comes from torch's pool on the stream the filter runs on: `stream` (a raw
        HIP stream handle; None = torch's current stream), which first waits for the work queued on the current stream.  The host does not wait."""
        return self._denoise(accum, hits, width, height, iterations, sigma_l, out, stream, False)[0]

    def denoise_times(self, accum, hits, width, height, iterations=5, sigma_l=4.0, out=None, stream=None):
        """bm_debug_denoise_times: Scene.denoise with a hipEvent between its kernels; waits.  Returns (out, [ms of prepare, the variance pass,
        every a-trous pass])."""
        return self._denoise(accum, hits, width, height, iterations, sigma_l, out, stream, True)

    def reproject(self, accum, hits, camera, prev_camera, history_prev, width, height, max_history=32.0, out=None, stream=None):
        """bm_reproject: temporal accumulation for a moving camera.  `accum` (float32 [height, width, 4]: R, G, B, n) is the
        frame just rendered with `camera`, `hits` its guides (Scene.pixel_hits, or its .packed tensor); `history_prev` is the History of the
        frame before, rendered with `prev_camera`, or None (no history: the result is accum and its keys).  Returns the new History -- `out`,
        or a new one; never history_prev itself: the taps read neighbours, so two histories take turns.  Its .image is an accumulation buffer
        of up to max_history + the frame's own samples per pixel, which Scene.denoise and Scene.resolve take.  Stream handling as in
        Scene.denoise; the host does not wait."""
        import torch
        hits, n = _device_frame(accum, hits, width, height)
        assert history_prev is None or (history_prev.buffer.is_cuda and history_prev.buffer.numel() == 5 * n), "history_prev: a History of this size on the GPU"
        h = Handoff(accum, stream)
        with h.on_target():
            if out is None:
                out = History(torch.empty(5 * n, dtype=torch.float32, device=accum.device), width, height)
        assert out.buffer.is_cuda and out.buffer.dtype == torch.float32 and out.buffer.numel() == 5 * n, "out: a History of this size on the GPU"
        h.reads(accum, hits, out.buffer, *((history_prev.buffer,) if history_prev is not None else ()))
        par = _lib.bm_reproject_params(int(width), int(height), float(max_history), 0, 0)
        c, cp = camera.to_c(), (prev_camera.to_c() if prev_camera is not None else None)
        check(self._L.bm_reproject(self.gpuScene, C.byref(par), C.byref(c), C.byref(cp) if cp is not None else None, C.c_void_p(accum.data_ptr()),
                                   C.c_void_p(hits.data_ptr()), C.c_void_p(history_prev.buffer.data_ptr()) if history_prev is not None else None,
                                   C.c_void_p(out.buffer.data_ptr()), C.c_void_p(h.handle)))
        return out


class TemporalAccumulator:
    """Temporal accumulation over the frames of a moving camera: owns two histories, which take turns, and the previous camera.
    add(camera, accum, hits=None) reprojects the history of the frame before into the frame just rendered (`accum`, 1 spp or a few into a
    zeroed buffer; hits: its guides, made with Scene.pixel_hits when not given) and returns the new history's image -- an accumulation
    buffer of up to max_history + the frame's own samples per pixel, for Scene.denoise and Scene.resolve; it stays valid until the
    add after the next.  reset() forgets the history: after a moved sun or an edit, which change the light without changing a key."""

    def __init__(self, scene, width, height, max_history=32.0):
        self.scene, self.width, self.height, self.max_history = scene, int(width), int(height), float(max_history)
        self._histories = [None, None]
        self._turn = 0
        self._camera = None  # of the newest history; None = no history

    def reset(self):
        self._camera = None

    @property
    def history(self):
        """the newest History, or None"""
        return self._histories[self._turn ^ 1] if self._camera is not None else None

    def add(self, camera, accum, hits=None):
        if hits is None:
            hits = self.scene.pixel_hits(camera, self.width, self.height)
        out = self.scene.reproject(accum, hits, camera, self._camera, self.history, self.width, self.height, self.max_history,
                                   out=self._histories[self._turn])
        self._histories[self._turn] = out
        self._turn ^= 1
        self._camera = replace(camera)
        return out.image
