"""Queries against a live scene: batched rays and picking (bm_scene_cast_rays), volume counts and sweeps (bm_scene_query_volumes), their
packed records, and the Scene methods that issue them (`_QueryMethods`)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._handoff import Handoff
from ._lib import BM_EDIT_BOX, BM_EDIT_SPHERE, BM_QUERY_LOD, BM_QUERY_NO_REQUESTS, BM_VOLUME_ANY, RAY_DTYPE, RAY_HIT_DTYPE, VOLUME_DTYPE, VOLUME_RESULT_DTYPE, check


# ---- ray queries (bm_scene_cast_rays): packed records, 32 bytes each
@dataclass
class RayHits:
    """Results of Scene.cast_rays, one row per ray, in the input's kind (torch CUDA tensors or numpy arrays): distance (+inf on a miss),
    normal (entry face), voxel (int32 x 3, -1 on a miss), level (-1 miss, 0 brick LoD, 1 2^3 LoD, 2 voxel, 3 brick not resident).
    `packed`: the bm_ray_hit records themselves (torch: float32 [n, 8] on the device; numpy: RAY_HIT_DTYPE)."""
    distance: object
    normal: object
    voxel: object
    level: object
    packed: object = None

    def __len__(self):
        return len(self.distance)


@dataclass
class RayHit:
    """One hit of Scene.pick: distance, normal (3 floats), voxel (3 ints), level."""
    distance: float
    normal: tuple
    voxel: tuple
    level: int


def camera_pixel_rays(camera, width, height, px, py):
    """bm_camera_pixel_rays (host only): rays of `camera` through continuous pixel positions (px[i], py[i]) of a width x height frame --
    the frames' primary rays without jitter and lens; (x + 0.5, y + 0.5) is pixel (x, y)'s centre.  Returns a RAY_DTYPE array."""
    px = np.ascontiguousarray(np.asarray(px, np.float32).reshape(-1))
    py = np.ascontiguousarray(np.asarray(py, np.float32).reshape(-1))
    assert px.shape == py.shape, "px and py: one value per ray"
    out = np.zeros(len(px), RAY_DTYPE)
    c = camera.to_c()
    check(_lib.load().bm_camera_pixel_rays(C.byref(c), int(width), int(height), len(px), px.ctypes.data, py.ctypes.data, out.ctypes.data))
    return out


def pack_rays(origins, directions, tmax=None):
    """numpy RAY_DTYPE records from N x 3 origins and directions (tmax: None = unbounded, a scalar, or one per ray)."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    assert len(o) == len(d), "one direction per origin"
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["origin"], rays["direction"] = o, d
    rays["tmax"] = np.inf if tmax is None else np.asarray(tmax, np.float32)
    return rays


# ---- volume queries (bm_scene_query_volumes): packed records, 48 bytes in, 40 bytes out
@dataclass
class VolumeResults:
    """Results of Scene.query_volumes, one row per record, in the input's kind (torch CUDA tensors or numpy arrays): solid (voxels counted;
    torch: int64), lo / hi (tight half-open bounds, int32 x 3, -1 when solid == 0), unresolved (brick cells that are not resident), status
    (1 = malformed record; both int32 in torch).  `packed`: the bm_volume_result records themselves (torch: uint8 [n, 40] on the device;
    numpy: VOLUME_RESULT_DTYPE)."""
    solid: object
    lo: object
    hi: object
    unresolved: object
    status: object
    packed: object = None

    def __len__(self):
        return len(self.solid)


def volume_box(lo, hi):
    """bm_volume records (a VOLUME_DTYPE array) of boxes lo <= v < hi: lo and hi are (x, y, z), or N x 3 for N boxes."""
    lo, hi = np.asarray(lo, np.int32).reshape(-1, 3), np.asarray(hi, np.int32).reshape(-1, 3)
    assert len(lo) == len(hi), "one hi per lo"
    out = np.zeros(len(lo), VOLUME_DTYPE)
    out["shape"], out["lo"], out["hi"] = BM_EDIT_BOX, lo, hi
    return out


def volume_sphere(center, radius):
    """bm_volume records of spheres sum((v - center)^2) <= radius^2: center is (x, y, z) or N x 3, radius a scalar or one per sphere."""
    center = np.asarray(center, np.int32).reshape(-1, 3)
    out = np.zeros(len(center), VOLUME_DTYPE)
    out["shape"], out["center"], out["radius"] = BM_EDIT_SPHERE, center, np.asarray(radius, np.int32)
    return out


def probe_streams(count, device=0):
    """bm_probe_streams: `count` HIP streams (raw handles, ints) that demonstrably run side by side on `device` -- HIP maps streams
    onto a few hardware queues, and streams that share one do not overlap.  release_streams() gives them back."""
    arr = (C.c_void_p * int(count))()
    check(_lib.load().bm_probe_streams(int(device), int(count), arr))
    return [int(h) for h in arr]


def release_streams(handles):
    _lib.load().bm_release_streams(len(handles), (C.c_void_p * len(handles))(*handles))


class _QueryMethods:
    """Scene's ray and volume queries: issued like a frame -- after every edit and upload issued before --, asynchronous to the host."""

    # ---- ray queries (bm_scene_cast_rays)
    def cast_rays_raw(self, n, rays_ptr, hits_ptr, flags=0, lod_origin=None, stream=None):
        """bm_scene_cast_rays on device pointers (ints): n bm_ray records in, n bm_ray_hit records out."""
        lo = None if lod_origin is None else (C.c_float * 3)(*[float(v) for v in lod_origin])
        check(self._L.bm_scene_cast_rays(self.gpuScene, int(n), C.c_void_p(rays_ptr), C.c_void_p(hits_ptr), int(flags), lo, self._stream(stream)))

    def cast_rays(self, origins, directions=None, tmax=None, lod_origin=None, request=True, stream=None):
        """First hit of each ray.  origins / directions: N x 3 torch CUDA tensors or numpy arrays; or, with directions=None, the packed
        bm_ray records themselves -- a float32 [N, 8] CUDA tensor (used as it is, no copy) or a RAY_DTYPE array.  tmax: None (unbounded),
        a scalar or one per ray.  lod_origin: None = exact (every brick at voxel level), else resolve with the frames' LoD rule around
        this point.  request=False: bricks that are not resident are reported (level 3) but not requested.  stream: a raw HIP stream handle
        (None = torch's current stream); the query runs there, behind the work already queued on the current stream.  Torch input: the
        result is on the device, ready in stream order on `stream`, and the host does not wait; numpy input: the call waits and returns
        numpy arrays."""
        import torch
        flags = (BM_QUERY_LOD if lod_origin is not None else 0) | (0 if request else BM_QUERY_NO_REQUESTS)
        dev = origins.device if isinstance(origins, torch.Tensor) else torch.device("cuda", self.device)
        h = Handoff(dev, stream)
        with h.on_target():  # everything the query touches is made on the stream it runs on: the packed rays and the hits come from its pool
            if isinstance(origins, torch.Tensor):
                if directions is None:
                    rays = origins
                    assert rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8 and rays.is_contiguous(), "packed rays: float32 [N, 8]"
                    inputs = [rays]
                else:
                    n = origins.shape[0]
                    t = torch.full((n, 1), float("inf"), dtype=torch.float32, device=dev) if tmax is None else \
                        torch.as_tensor(tmax, dtype=torch.float32, device=dev).reshape(-1, 1).expand(n, 1)
                    inputs = [origins, directions] + ([t] if isinstance(tmax, torch.Tensor) else [])
                    rays = torch.cat([origins.to(torch.float32).reshape(n, 3), directions.to(torch.float32).reshape(n, 3), t,
                                      torch.zeros((n, 1), dtype=torch.float32, device=dev)], dim=1).contiguous()
                assert rays.is_cuda, "torch rays must be on the GPU"
                h.reads(*inputs)
                n = rays.shape[0]
                hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
                self.cast_rays_raw(n, rays.data_ptr(), hits.data_ptr(), flags, lod_origin, h.handle)
                return RayHits(hits[:, 0], hits[:, 1:4], hits[:, 4:7].view(torch.int32), hits[:, 7].view(torch.int32), hits)
            rays = origins if directions is None else pack_rays(origins, directions, tmax)
            rays = np.ascontiguousarray(rays)
            assert rays.dtype == RAY_DTYPE, "packed rays: a RAY_DTYPE array"
            n = len(rays)
            out = np.zeros(n, RAY_HIT_DTYPE)
            if n:
                d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8)).to(dev)
                d_hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
                self.cast_rays_raw(n, d_rays.data_ptr(), d_hits.data_ptr(), flags, lod_origin, h.handle)
                h.target.synchronize()
                out = d_hits.cpu().numpy().view(RAY_HIT_DTYPE).reshape(n)
            return RayHits(out["distance"], out["normal"], out["voxel"], out["level"], out)

    def pixel_rays(self, camera, width, height, stream=None):
        """bm_camera_pixel_rays_device: the pixel-centre rays of a width x height frame of `camera`, written on the device -- a float32
        [height * width, 8] CUDA tensor of packed bm_ray records, ray y * width + x through pixel (x, y), bit for bit what
        camera_pixel_rays gives for (x + 0.5, y + 0.5).  Ready in stream order on `stream` (None = torch's current stream)."""
        import torch
        dev = torch.device("cuda", self.device)
        h = Handoff(dev, stream)
        with h.on_target():
            rays = torch.empty((int(height) * int(width), 8), dtype=torch.float32, device=dev)
            c = camera.to_c()
            check(self._L.bm_camera_pixel_rays_device(self.gpuScene, C.byref(c), int(width), int(height), C.c_void_p(rays.data_ptr()), C.c_void_p(h.handle)))
        return rays

    def pixel_hits(self, camera, width, height, lod_origin="camera", stream=None):
        """The first hit of every pixel's centre ray -- the guides of Scene.denoise: rays made on the device (pixel_rays), then cast_rays.
        lod_origin: "camera" (default) = the frames' LoD rule around the camera position, so the guides see the geometry the frame sees;
        None = exact (every brick at voxel level); or a point.  Returns RayHits (torch); .packed is the [height * width, 8] record tensor."""
        if isinstance(lod_origin, str):
            assert lod_origin == "camera", "lod_origin: 'camera', None or a point"
            lod_origin = tuple(float(v) for v in camera.position)
        rays = self.pixel_rays(camera, width, height, stream=stream)
        return self.cast_rays(rays, lod_origin=lod_origin, stream=stream)

    def pick(self, camera, x, y, width, height, lod_origin=None):
        """The voxel under pixel (x, y) of a width x height frame of `camera`: one ray through the pixel's centre, one query, then the host
        waits.  Returns a RayHit, or None on a miss.  (A level-3 hit means the brick is not resident yet: service the load queue and pick again.)"""
        rays = camera_pixel_rays(camera, width, height, [x + 0.5], [y + 0.5])
        h = self.cast_rays(rays, lod_origin=lod_origin).packed[0]
        if int(h["level"]) < 0:
            return None
        return RayHit(float(h["distance"]), tuple(float(v) for v in h["normal"]), tuple(int(v) for v in h["voxel"]), int(h["level"]))

    # ---- volume queries (bm_scene_query_volumes): issued like a ray query
    def query_volumes_raw(self, n, volumes_ptr, results_ptr, flags=0, stream=None):
        """bm_scene_query_volumes on device pointers (ints): n bm_volume records in, n bm_volume_result records out."""
        check(self._L.bm_scene_query_volumes(self.gpuScene, int(n), C.c_void_p(volumes_ptr), C.c_void_p(results_ptr), int(flags), self._stream(stream)))

    def query_volumes(self, volumes, any=False, stream=None):
        """Solid voxels, their tight bounds and the unresolved brick cells of each box or sphere.  volumes: a VOLUME_DTYPE array
        (volume_box / volume_sphere; np.concatenate joins them), or the records as a contiguous uint8 CUDA tensor of 48 n bytes (used
        as it is, no copy).  any=True: the yes / no probe BM_VOLUME_ANY (solid 0 / 1, bounds -1).  stream: a raw HIP stream handle
        (None = torch's current stream); the query runs there, behind the work already queued on the current stream.  A tensor gives
        tensors on the device, ready in stream order on `stream`, and the host does not wait; an array makes the call wait and gives arrays."""
        import torch
        flags = BM_VOLUME_ANY if any else 0
        dev = volumes.device if isinstance(volumes, torch.Tensor) else torch.device("cuda", self.device)
        h = Handoff(dev, stream)
        with h.on_target():  # (what the query touches is made on the stream it runs on, as in cast_rays)
            if isinstance(volumes, torch.Tensor):
                assert volumes.is_cuda and volumes.dtype == torch.uint8 and volumes.is_contiguous() and volumes.numel() % 48 == 0, "packed volumes: contiguous uint8, 48 bytes per record, on the GPU"
                h.reads(volumes)
                n = volumes.numel() // 48
                res = torch.empty((n, 40), dtype=torch.uint8, device=dev)
                self.query_volumes_raw(n, volumes.data_ptr(), res.data_ptr(), flags, h.handle)
                return VolumeResults(res[:, 0:8].view(torch.int64).reshape(n), res[:, 8:20].view(torch.int32), res[:, 20:32].view(torch.int32),
                                     res[:, 32:36].view(torch.int32).reshape(n), res[:, 36:40].view(torch.int32).reshape(n), res)
            volumes = np.ascontiguousarray(volumes)
            assert volumes.dtype == VOLUME_DTYPE, "packed volumes: a VOLUME_DTYPE array"
            n = volumes.size
            out = np.zeros(n, VOLUME_RESULT_DTYPE)
            if n:
                d_vol = torch.from_numpy(volumes.reshape(n).view(np.uint8).reshape(n, 48)).to(dev)
                d_res = torch.empty((n, 40), dtype=torch.uint8, device=dev)
                self.query_volumes_raw(n, d_vol.data_ptr(), d_res.data_ptr(), flags, h.handle)
                h.target.synchronize()
                out = d_res.cpu().numpy().view(VOLUME_RESULT_DTYPE).reshape(n)
            return VolumeResults(out["solid"], out["lo"], out["hi"], out["unresolved"], out["status"], out)

    def count_box(self, lo, hi):
        """Solid voxels in the box lo <= v < hi (one query, then the host waits); in a streaming scene only resident bricks count."""
        return int(self.query_volumes(volume_box(lo, hi)).solid[0])

    def count_sphere(self, center, radius):
        """Solid voxels in the sphere sum((v - center)^2) <= radius^2 (one query, then the host waits)."""
        return int(self.query_volumes(volume_sphere(center, radius)).solid[0])

    def is_free(self, lo, hi):
        """True when no resident solid voxel lies in the box lo <= v < hi (the early-out probe BM_VOLUME_ANY)."""
        return int(self.query_volumes(volume_box(lo, hi), any=True).solid[0]) == 0

    def sweep_box(self, lo, hi, axis, sign, max_distance):
        """How far the box lo <= v < hi can move along sign * axis (axis 0 / 1 / 2 = x / y / z, sign +1 / -1): the largest d in
        [0, max_distance] such that the box moved by k voxels meets no solid voxel for every 1 <= k <= d.  One box query per sweep, over
        everything the moved boxes cover -- the box moved by one voxel, stretched by max_distance - 1 more along the direction; d follows
        from the bounds of the solid voxels found there, exactly: the nearest one beyond the leading face stops the box in front of it,
        and one inside the box moved by one voxel (a box that starts in something solid) gives 0.  All arguments are scalars / (x, y, z),
        or arrays of N (N x 3 for lo and hi).  Returns (d, unresolved): numpy arrays of N, or two ints for one box; unresolved counts the
        brick cells of the queried space that are not resident (a streaming scene)."""
        single = np.ndim(lo) == 1 and all(np.ndim(v) == 0 for v in (axis, sign, max_distance))
        lo, hi = np.asarray(lo, np.int64).reshape(-1, 3), np.asarray(hi, np.int64).reshape(-1, 3)
        n = max(len(lo), np.size(axis), np.size(sign), np.size(max_distance))
        lo, hi = np.broadcast_to(lo, (n, 3)), np.broadcast_to(hi, (n, 3))
        axis, sign, dist = (np.broadcast_to(np.asarray(v, np.int64), (n,)) for v in (axis, sign, max_distance))
        assert ((axis >= 0) & (axis <= 2)).all() and (np.abs(sign) == 1).all() and (dist >= 0).all(), "axis 0 ... 2, sign +1 / -1, max_distance >= 0"
        rows = np.arange(n)
        face_hi, face_lo = hi[rows, axis], lo[rows, axis]
        elo, ehi = lo.copy(), hi.copy()
        elo[rows, axis] = np.where(sign > 0, face_lo + 1, face_lo - dist)
        ehi[rows, axis] = np.where(sign > 0, face_hi + dist, face_hi - 1)
        ehi[dist == 0] = elo[dist == 0]  # nothing to ask
        lim = np.iinfo(np.int32)
        res = self.query_volumes(volume_box(np.clip(elo, lim.min, lim.max), np.clip(ehi, lim.min, lim.max)))
        hit = res.solid > 0
        d = np.where(hit, np.maximum(np.where(sign > 0, res.lo[rows, axis] - face_hi, face_lo - res.hi[rows, axis]), 0), dist)
        unresolved = res.unresolved.astype(np.int64)
        return (int(d[0]), int(unresolved[0])) if single else (d, unresolved)
