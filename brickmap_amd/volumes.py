"""The stateless operators on dense volumes [z, y, x] -- meshes -> voxels, voxels -> quads, distances, travel fields --, their host-only
doors, the one layout and the one set of argument checks they share, and the Scene methods that issue them (`_VolumeMethods`)."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import DISTANCE_RESULT_DTYPE, MESH_RESULT_DTYPE, QUAD_DTYPE, TRAVEL_RESULT_DTYPE, VOXELIZE_RESULT_DTYPE, bm_region, check, size_call, stage_call
from .world import region_of


# ---- result records: a filled struct on the host, or int64 words on the device that are read lazily
def record_of(struct):
    """a filled ctypes structure as a numpy record of its dtype (a 0-d array of its own)"""
    return np.frombuffer(bytes(struct), np.dtype(type(struct))).reshape(()).copy()


class DeviceRecord:
    """A result record that stands on the device as int64 words in the tensor named by `_record_in`: `record` copies it to the host once
    (a scalar of `_record_dtype`), which waits for the call that wrote it."""
    _record_in, _record_dtype, _record = "result", None, None

    @property
    def record(self):
        if self._record is None:
            self._record = getattr(self, self._record_in).cpu().numpy().view(self._record_dtype).reshape(())
        return self._record


# ---- the layout of a dense volume in a params struct, and the argument checks of the operators
def dense_layout(par, region):
    """Fill whichever of lo, extent, row_pitch and slice_pitch the params struct `par` has from a bm_region (region_of's): the one place
    where the layout of a dense volume enters a params struct.  Returns par."""
    if hasattr(par, "lo"):
        par.lo[:] = list(region.lo)
    par.extent[:] = [(h - l) % (1 << 32) for l, h in zip(region.lo, region.hi)]  # (hi is lo + extent in 32 bits, wrapped or not)
    par.row_pitch, par.slice_pitch = region.row_pitch, region.slice_pitch
    return par


def _workspace_bytes(name, par, shape, lo=(0, 0, 0), *args):
    """bm_<name>_workspace_bytes of a volume of shape (nz, ny, nx) at lo: only the box is laid out, the pitches stay 0"""
    box = bm_region()
    box.lo[:] = [int(v) for v in lo]
    box.hi[:] = [int(l) + int(n) for l, n in zip(lo, tuple(shape)[::-1])]
    return size_call(f"bm_{name}_workspace_bytes", C.byref(dense_layout(par, box)), *args)


def _device_volume(name, volume, params, *args):
    """(params struct, data pointer) of a volume on a GPU: raises for another device, what params(*args) refuses (dtype, layout), no voxel"""
    if not hasattr(volume, "is_cuda") or not volume.is_cuda:
        raise ValueError(f"{name}: volume must be a uint8 or bool tensor [z, y, x] on the scene's GPU")
    par, ptr, _ = params(*args)
    if min(volume.shape) == 0:
        raise ValueError(f"{name}: a volume with positive extents expected, got shape {tuple(volume.shape)}")
    return par, ptr


def _int32_out(name, out, shape):
    """the check of `out`, an int32 field of the volume's shape to fill on the device (None passes)"""
    import torch
    if out is not None and (not hasattr(out, "is_cuda") or not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous()):
        raise ValueError(f"{name}: out must be a contiguous int32 tensor of shape {shape} on the scene's GPU")


def _points(points, name):
    """an int32 numpy array [n, 3] of (x, y, z) from a list or an array ([3] is one point)"""
    a = np.asarray(points)
    if a.size == 0:
        return np.zeros((0, 3), np.int32)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name}: integer coordinates expected, got {a.dtype}")
    if a.ndim == 1 and a.shape[0] == 3:
        a = a.reshape(1, 3)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{name}: an array [n, 3] of (x, y, z) expected, got shape {a.shape}")
    return np.ascontiguousarray(a, np.int32)


def _device_points(name, what, points, dev):
    """a contiguous int32 tensor [n, 3] on `dev` from a list or an array (copied there on torch's current stream) or from such a tensor"""
    import torch
    if not (hasattr(points, "is_cuda") and points.is_cuda):
        points = torch.from_numpy(_points(points, name)).to(dev)
    if points.dtype != torch.int32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
        raise ValueError(f"{name}: {what} must be a contiguous int32 tensor [n, 3]")
    return points


def _nonempty_box(name, lo, hi):
    """(lo, hi) as lists of ints; raises for a box without a voxel"""
    lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    if any(h <= l for l, h in zip(lo, hi)):
        raise ValueError(f"{name}: an empty box ({lo} ... {hi})")
    return lo, hi


# ---- meshes -> voxels (bm_voxelize / bm_host_voxelize)
_VOXELIZE_MODES = {"surface": _lib.BM_VOXELIZE_SURFACE, "solid": _lib.BM_VOXELIZE_SOLID,
                   "solid+surface": _lib.BM_VOXELIZE_SURFACE | _lib.BM_VOXELIZE_SOLID, "surface+solid": _lib.BM_VOXELIZE_SURFACE | _lib.BM_VOXELIZE_SOLID}


def _voxelize_mode(mode):
    if isinstance(mode, str) and mode not in _VOXELIZE_MODES:
        raise ValueError(f"voxelize: mode 'surface', 'solid' or 'solid+surface' expected, got {mode!r}")
    return _VOXELIZE_MODES[mode] if isinstance(mode, str) else int(mode)


def _voxelize_params(lo, volume, mode, keep, name="out"):
    """(bm_voxelize_params, data pointer, is_cuda) of `volume` ([z, y, x], laid out as region_of takes it) with its voxel [0, 0, 0] at lo"""
    r, ptr, cuda = region_of(lo, volume, name)
    par = dense_layout(_lib.bm_voxelize_params(), r)
    par.mode = _voxelize_mode(mode)
    par.flags = _lib.BM_VOXELIZE_KEEP if keep else 0
    return par, ptr, cuda


def voxelize_workspace_bytes(shape, n, mode="solid+surface"):
    """bm_voxelize_workspace_bytes: device memory bm_voxelize needs beside its buffers for a volume of shape (nz, ny, nx) and n triangles."""
    par = _lib.bm_voxelize_params()
    par.mode = _voxelize_mode(mode)
    return _workspace_bytes("voxelize", par, shape, (0, 0, 0), int(n))


def host_voxelize(triangles, lo, shape=None, mode="solid+surface", keep=False, out=None):
    """bm_host_voxelize (host only, no device): the voxelization of Scene.voxelize as plain loops.  triangles: float32 [n, 3, 3] (xyz per
    vertex, world voxel units); lo = (x, y, z), the world voxel of the volume's first voxel; shape = (nz, ny, nx), or `out`: a uint8 array
    [z, y, x] to fill (a slice of a larger array works as long as x is contiguous).  keep: OR into what the volume holds.  Returns (volume, record): the uint8 volume and a VOXELIZE_RESULT_DTYPE record (rejected, degenerate,
    open_columns)."""
    tri = np.ascontiguousarray(triangles, dtype=np.float32)
    if tri.size % 9:
        raise ValueError(f"host_voxelize: triangles of shape [n, 3, 3] expected, got {tri.shape}")
    if out is None:
        out = np.zeros(tuple(int(v) for v in shape), np.uint8)
    par, ptr, cuda = _voxelize_params(lo, out, mode, keep)
    assert not cuda
    res = _lib.bm_voxelize_result()
    check(_lib.load().bm_host_voxelize(C.byref(par), tri.size // 9, C.c_void_p(tri.ctypes.data), C.c_void_p(ptr), C.byref(res)))
    return out, record_of(res)


class VoxelizeResult(DeviceRecord):
    """The bm_voxelize_result of a Scene.voxelize, read lazily: `packed` is the record on the device (two int64 words); rejected,
    degenerate, open_columns and record (a VOXELIZE_RESULT_DTYPE scalar) copy it to the host, which waits for the call."""
    _record_in, _record_dtype = "packed", VOXELIZE_RESULT_DTYPE

    def __init__(self, packed):
        self.packed = packed

    rejected = property(lambda self: int(self.record["rejected"]))
    degenerate = property(lambda self: int(self.record["degenerate"]))
    open_columns = property(lambda self: int(self.record["open_columns"]))


# ---- voxels -> quads (bm_mesh_quads / bm_host_mesh_quads)
def _mesh_params(lo, volume, halo, unit, name="volume"):
    """(bm_mesh_params, data pointer, is_cuda) of `volume` ([z, y, x], laid out as region_of takes it) with its voxel [0, 0, 0] at lo"""
    r, ptr, cuda = region_of(lo, volume, name)
    par = dense_layout(_lib.bm_mesh_params(), r)
    par.flags = (_lib.BM_MESH_HALO if halo else 0) | (_lib.BM_MESH_UNIT_FACES if unit else 0)
    return par, ptr, cuda


def mesh_workspace_bytes(shape, halo=False, lo=(0, 0, 0)):
    """bm_mesh_workspace_bytes: device memory bm_mesh_quads needs beside its buffers for a volume of shape (nz, ny, nx) whose first voxel is
    world voxel lo (the cells are the world's, so their number depends on lo modulo 8)."""
    par = _lib.bm_mesh_params()
    par.flags = _lib.BM_MESH_HALO if halo else 0
    return _workspace_bytes("mesh", par, shape, lo)


def host_mesh_quads(volume, lo=(0, 0, 0), halo=False, unit=False):
    """bm_host_mesh_quads (host only, no device): the surface of a dense volume [z, y, x] (uint8 or bool numpy array, non-zero = solid; a
    slice of a larger array works as long as x is contiguous) whose first voxel is world voxel lo = (x, y, z), as plain loops.  halo: the
    outermost shell of the volume is context only; unit: one quad per face.  Returns (quads, record): a QUAD_DTYPE array in the
    contract's order and a MESH_RESULT_DTYPE record (quads, faces)."""
    par, ptr, cuda = _mesh_params(lo, volume, halo, unit)
    assert not cuda
    L = _lib.load()
    res = _lib.bm_mesh_result()
    check(L.bm_host_mesh_quads(C.byref(par), C.c_void_p(ptr), None, 0, C.byref(res)))
    quads = np.zeros(int(res.quads), QUAD_DTYPE)
    if len(quads):
        check(L.bm_host_mesh_quads(C.byref(par), C.c_void_p(ptr), C.c_void_p(quads.ctypes.data), len(quads), C.byref(res)))
    return quads, record_of(res)


def host_mesh_triangles(quads):
    """bm_host_mesh_triangles (host only): the two triangles of every quad (a QUAD_DTYPE array) as float32 [2 n, 3, 3], counter-clockwise
    seen from outside: what host_voxelize and Scene.voxelize read."""
    quads = np.ascontiguousarray(np.asarray(quads, dtype=QUAD_DTYPE).reshape(-1))
    tri = np.zeros((2 * len(quads), 3, 3), np.float32)
    check(_lib.load().bm_host_mesh_triangles(C.c_void_p(quads.ctypes.data), len(quads), C.c_void_p(tri.ctypes.data)))
    return tri


class Quads(DeviceRecord):
    """The quads of a Scene.mesh_quads, read lazily: `packed` is the quad buffer on the device (an int32 tensor [capacity, 4]) and
    `result` the bm_mesh_result there (two int64 words); count, faces, record (a MESH_RESULT_DTYPE scalar) and records (a QUAD_DTYPE array
    of the min(count, capacity) quads written) copy to the host, which waits for the call.  triangles() stays on the device."""
    _record_dtype = MESH_RESULT_DTYPE

    def __init__(self, scene, packed, result, record=None):
        self.scene, self.packed, self.result = scene, packed, result
        self._record, self._records = record, None

    count = property(lambda self: int(self.record["quads"]))
    faces = property(lambda self: int(self.record["faces"]))

    def __len__(self):
        return min(self.count, int(self.packed.shape[0]))

    @property
    def records(self):
        if self._records is None:
            self._records = np.ascontiguousarray(self.packed[:len(self)].cpu().numpy()).view(QUAD_DTYPE).reshape(-1)
        return self._records

    def triangles(self, stream=None):
        """bm_mesh_triangles: a float32 tensor [2 n, 3, 3] on the scene's GPU for the n quads written, as Scene.voxelize takes it (reads
        the count: waits for the call that made the quads)."""
        import torch
        n = len(self)
        h = self.scene._handoff(self.packed, stream)
        with h.on_target():
            tri = torch.empty((2 * n, 3, 3), dtype=torch.float32, device=self.packed.device)
        if n:
            check(self.scene._L.bm_mesh_triangles(self.scene.gpuScene, C.c_void_p(self.packed.data_ptr()), n, C.c_void_p(tri.data_ptr()), C.c_void_p(h.handle)))
            h.reads(self.packed)
            h.join()
        return tri


# ---- voxels -> distances (bm_distance_field / bm_host_distance_field)
DISTANCE_NONE = _lib.BM_DISTANCE_NONE


def _distance_flags(to, outside):
    if to not in ("solid", "empty"):
        raise ValueError(f"distance_field: to 'solid' or 'empty' expected, got {to!r}")
    return (_lib.BM_DISTANCE_TO_EMPTY if to == "empty" else 0) | (_lib.BM_DISTANCE_OUTSIDE if outside else 0)


def _distance_params(volume, to, outside, name="volume"):
    """(bm_distance_params, data pointer, is_cuda) of `volume` ([z, y, x], laid out as region_of takes it)"""
    flags = _distance_flags(to, outside)
    r, ptr, cuda = region_of((0, 0, 0), volume, name)
    par = dense_layout(_lib.bm_distance_params(), r)
    par.flags = flags
    return par, ptr, cuda


def distance_workspace_bytes(shape):
    """bm_distance_workspace_bytes: device memory bm_distance_field needs beside its buffers for a volume of shape (nz, ny, nx)."""
    return _workspace_bytes("distance", _lib.bm_distance_params(), shape)


def host_distance_field(volume, to="solid", outside=False):
    """bm_host_distance_field (host only, no device): the exact squared Euclidean distance of every voxel of a dense volume [z, y, x]
    (uint8 or bool numpy array, non-zero = solid; a slice of a larger array works as long as x is contiguous) to the nearest source, as
    plain loops.  to="solid": the solid voxels are the sources; to="empty": the empty ones; outside=True: every voxel outside the volume
    is a source too.  Returns (field, record): an int32 array [z, y, x] (DISTANCE_NONE where there is no source) and a
    DISTANCE_RESULT_DTYPE record (sources, max_sq, max_at)."""
    par, ptr, cuda = _distance_params(volume, to, outside)
    assert not cuda
    if min(volume.shape) == 0:
        raise ValueError(f"host_distance_field: a volume with positive extents expected, got shape {tuple(volume.shape)}")
    field = np.zeros(tuple(volume.shape), np.int32)
    res = _lib.bm_distance_result()
    check(_lib.load().bm_host_distance_field(C.byref(par), C.c_void_p(ptr), C.c_void_p(field.ctypes.data), C.byref(res)))
    return field, record_of(res)


def host_distance_mask(field, limit_sq, above=False):
    """bm_host_distance_mask (host only): the uint8 volume field <= limit_sq (above=True: the opposite) of an int32 / uint32 field, in its
    shape; DISTANCE_NONE is above every limit."""
    field = np.ascontiguousarray(field)
    if field.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)):
        raise ValueError(f"host_distance_mask: an int32 or uint32 field expected, got {field.dtype}")
    out = np.zeros(field.shape, np.uint8)
    check(_lib.load().bm_host_distance_mask(field.size, C.c_void_p(field.ctypes.data), int(limit_sq), _lib.BM_DISTANCE_MASK_ABOVE if above else 0, C.c_void_p(out.ctypes.data)))
    return out


class DistanceField(DeviceRecord):
    """The field of a Scene.distance_field: `field` is the int32 tensor [z, y, x] on the device (DISTANCE_NONE where there is no source)
    and `result` the bm_distance_result there (four int64 words).  record (a DISTANCE_RESULT_DTYPE scalar) and largest() copy the result
    to the host, which waits for the call; mask() stays on the device."""
    _record_dtype = DISTANCE_RESULT_DTYPE

    def __init__(self, scene, field, result):
        self.scene, self.field, self.result = scene, field, result

    sources = property(lambda self: int(self.record["sources"]))

    def largest(self):
        """((x, y, z), radius_sq) of the largest ball of non-sources: the lowest-indexed voxel with the largest finite distance, in the
        volume's own coordinates; None when no distance is finite."""
        rec = self.record
        if int(rec["max_sq"]) == DISTANCE_NONE:
            return None
        nz, ny, nx = self.field.shape
        at = int(rec["max_at"])
        return (at % nx, at // nx % ny, at // (nx * ny)), int(rec["max_sq"])

    def mask(self, radius_sq, above=False, out=None, stream=None):
        """bm_distance_mask: a uint8 tensor of the field's shape, 1 where the distance is <= radius_sq (above=True: where it is not) --
        what write_region takes.  out: a contiguous uint8 tensor of that many voxels to fill (any base address).  The host does not wait."""
        import torch
        if not 0 <= int(radius_sq) <= 0xFFFFFFFF:
            raise ValueError(f"mask: radius_sq in 0 ... 2^32 - 1 expected, got {radius_sq}")
        h = self.scene._handoff(self.field, stream)
        with h.on_target():
            if out is None:
                out = torch.empty(tuple(self.field.shape), dtype=torch.uint8, device=self.field.device)
        if not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != self.field.numel():
            raise ValueError("mask: out must be a contiguous uint8 tensor of the field's size on the scene's GPU")
        h.reads(self.field, out)
        check(self.scene._L.bm_distance_mask(self.scene.gpuScene, self.field.numel(), C.c_void_p(self.field.data_ptr()), int(radius_sq),
                                             _lib.BM_DISTANCE_MASK_ABOVE if above else 0, C.c_void_p(out.data_ptr()), C.c_void_p(h.handle)))
        h.join()
        return out


# ---- voxels + seeds -> shortest face-step distances and paths (bm_travel_field / bm_host_travel_field)
TRAVEL_NONE = _lib.BM_TRAVEL_NONE


def _travel_params(volume, max_steps, name="volume"):
    """(bm_travel_params, data pointer, is_cuda) of `volume` ([z, y, x], laid out as region_of takes it)"""
    if not 0 <= int(max_steps) <= 0xFFFFFFFF:
        raise ValueError(f"travel_field: max_steps in 0 ... 2^32 - 1 expected (0 = no limit), got {max_steps}")
    r, ptr, cuda = region_of((0, 0, 0), volume, name)
    par = dense_layout(_lib.bm_travel_params(), r)
    par.max_steps = int(max_steps)
    return par, ptr, cuda


def travel_workspace_bytes(shape):
    """bm_travel_workspace_bytes: device memory bm_travel_field needs beside its buffers for a volume of shape (nz, ny, nx)."""
    return _workspace_bytes("travel", _lib.bm_travel_params(), shape)


def host_travel_field(volume, seeds, max_steps=0):
    """bm_host_travel_field (host only, no device): the least number of face steps from any accepted seed to every voxel of a dense volume
    [z, y, x] (uint8 or bool numpy array, non-zero = blocked; a slice of a larger array works as long as x is contiguous) through voxels
    that are not blocked, as a plain breadth-first search.  seeds: [n, 3] of (x, y, z); max_steps: 0 = no limit.  Returns (field, record):
    an int32 array [z, y, x] (TRAVEL_NONE where blocked, unreachable or beyond max_steps) and a TRAVEL_RESULT_DTYPE record."""
    par, ptr, cuda = _travel_params(volume, max_steps)
    assert not cuda
    if min(volume.shape) == 0:
        raise ValueError(f"host_travel_field: a volume with positive extents expected, got shape {tuple(volume.shape)}")
    pts = _points(seeds, "host_travel_field")
    field = np.zeros(tuple(volume.shape), np.int32)
    res = _lib.bm_travel_result()
    check(_lib.load().bm_host_travel_field(C.byref(par), C.c_void_p(ptr), C.c_void_p(pts.ctypes.data if len(pts) else None), len(pts), C.c_void_p(field.ctypes.data), C.byref(res)))
    return field, record_of(res)


def host_travel_paths(field, starts, capacity):
    """bm_host_travel_paths (host only): walks down an int32 / uint32 field [z, y, x] from every start ([n, 3] of (x, y, z)).  Returns
    (path, lengths): int32 [n, capacity, 3], of which the first min(length, capacity) voxels of every path are written (the rest is -1),
    and int32 [n]: T(start) + 1, 0 for a start outside the volume or without a finite value, -1 where the field is not a travel field."""
    field = np.ascontiguousarray(field)
    if field.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)) or field.ndim != 3:
        raise ValueError(f"host_travel_paths: an int32 or uint32 field [z, y, x] expected, got {field.dtype} {field.shape}")
    pts = _points(starts, "host_travel_paths")
    capacity = int(capacity)
    path = np.full((len(pts), max(capacity, 0), 3), -1, np.int32)
    lengths = np.zeros(len(pts), np.int32)
    extent = (C.c_int32 * 3)(field.shape[2], field.shape[1], field.shape[0])
    check(_lib.load().bm_host_travel_paths(extent, C.c_void_p(field.ctypes.data), C.c_void_p(pts.ctypes.data if len(pts) else None), len(pts), capacity,
                                           C.c_void_p(path.ctypes.data if path.size else None), C.c_void_p(lengths.ctypes.data if len(pts) else None)))
    return path, lengths


class TravelField(DeviceRecord):
    """The field of a Scene.travel_field: `field` is the int32 tensor [z, y, x] on the device (TRAVEL_NONE where blocked, unreachable or
    beyond max_steps) and `result` the bm_travel_result there (four int64 words).  The field stands when travel_field returns.  record (a
    TRAVEL_RESULT_DTYPE scalar) and path() copy to the host, which waits; paths() stays on the device."""
    _record_dtype = TRAVEL_RESULT_DTYPE

    def __init__(self, scene, field, result):
        self.scene, self.field, self.result = scene, field, result

    reached = property(lambda self: int(self.record["reached"]))

    def paths(self, starts, capacity, stream=None):
        """bm_travel_paths: from every start ([n, 3] of (x, y, z) in the volume's coordinates; a list, a numpy array or an int32 tensor on
        the scene's GPU) down the field.  Returns (path, lengths), int32 tensors [n, capacity, 3] and [n] on the device: the first
        min(length, capacity) voxels of every path, the start first (the rest is -1); lengths as in host_travel_paths.  The host does not
        wait."""
        import torch
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"paths: a capacity of at least 1 expected, got {capacity}")
        dev = self.field.device
        starts = _device_points("paths", "starts", starts, dev)
        n = int(starts.shape[0])
        h = self.scene._handoff(self.field, stream)
        with h.on_target():
            path = torch.full((n, capacity, 3), -1, dtype=torch.int32, device=dev)
            lengths = torch.zeros(n, dtype=torch.int32, device=dev)
        h.reads(self.field, starts, path, lengths)
        extent = (C.c_int32 * 3)(*tuple(self.field.shape)[::-1])
        check(self.scene._L.bm_travel_paths(self.scene.gpuScene, extent, C.c_void_p(self.field.data_ptr()), C.c_void_p(starts.data_ptr() if n else None), n, capacity,
                                            C.c_void_p(path.data_ptr() if n else None), C.c_void_p(lengths.data_ptr() if n else None), C.c_void_p(h.handle)))
        h.join()
        return path, lengths

    def path(self, start):
        """The whole path from `start` (x, y, z) down to a seed: an int32 numpy array [length, 3], the start first; None when the start is
        outside the volume or has no finite value.  Waits: the start's value is read first, and gives the capacity."""
        x, y, z = (int(v) for v in start)
        nz, ny, nx = self.field.shape
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
            return None
        t = int(self.field[z, y, x].item())
        if t == TRAVEL_NONE:
            return None
        path, lengths = self.paths([(x, y, z)], t + 1)
        if int(lengths[0].item()) != t + 1:
            raise RuntimeError("path: the field is not a travel field")
        return path[0].cpu().numpy()


class _VolumeMethods:
    """Scene's methods that issue the volume operators, and the calls that join them with read_region / write_region."""

    # ---- meshes -> voxels (bm_voxelize)
    def _triangles(self, triangles):
        """float32 [n, 3, 3] on the scene's GPU from such a tensor, or from (vertices [m, 3], faces [n, 3]) gathered with torch"""
        import torch
        if isinstance(triangles, (tuple, list)) and len(triangles) == 2:
            vertices, faces = triangles
            dev = torch.device("cuda", self.device)
            vertices = torch.as_tensor(vertices, dtype=torch.float32, device=dev)
            faces = torch.as_tensor(faces, device=dev).long()
            if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
                raise ValueError(f"voxelize: vertices [m, 3] and faces [n, 3] expected, got {tuple(vertices.shape)} and {tuple(faces.shape)}")
            return vertices[faces].contiguous()
        if not hasattr(triangles, "is_cuda"):
            raise ValueError(f"voxelize: a float32 tensor [n, 3, 3] on the scene's GPU, or (vertices, faces), expected, got {type(triangles).__name__}")
        if not triangles.is_cuda or triangles.device.index != self.device or triangles.dtype != torch.float32 or triangles.ndim != 3 or tuple(triangles.shape[1:]) != (3, 3):
            raise ValueError(f"voxelize: a float32 tensor [n, 3, 3] on cuda:{self.device} expected, got {triangles.dtype} {tuple(triangles.shape)} on {triangles.device}")
        return triangles.contiguous()

    def _voxelize(self, triangles, lo, shape, mode, keep, out, stream, times):
        import torch
        tri = self._triangles(triangles)
        dev = tri.device
        if out is None:
            if shape is None or len(shape) != 3 or min(int(v) for v in shape) < 1:
                raise ValueError(f"voxelize: shape (nz, ny, nx) with positive extents expected, got {shape}")
            if keep:
                raise ValueError("voxelize: keep needs the volume to keep (out)")
        elif not hasattr(out, "is_cuda") or not out.is_cuda:
            raise ValueError("voxelize: out must be a uint8 or bool tensor [z, y, x] on the scene's GPU")
        h = self._handoff(tri, stream)
        with h.on_target():
            if out is None:
                out = torch.empty(tuple(int(v) for v in shape), dtype=torch.uint8, device=dev)
            par, ptr, _ = _voxelize_params(lo, out, mode, keep)
            n = int(tri.shape[0])
            ws = torch.empty(voxelize_workspace_bytes(out.shape, n, par.mode), dtype=torch.uint8, device=dev)
            packed = torch.empty(2, dtype=torch.int64, device=dev)
        h.reads(tri, out)
        args = (self.gpuScene, C.byref(par), n, C.c_void_p(tri.data_ptr()), C.c_void_p(ptr), C.c_void_p(packed.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                C.c_void_p(h.handle))
        ms = stage_call(self._L.bm_voxelize, self._L.bm_debug_voxelize_times, args, 5 if times else None)
        h.join()
        return out, VoxelizeResult(packed), ms

    def voxelize(self, triangles, lo, shape=None, mode="solid+surface", keep=False, out=None, stream=None):
        """bm_voxelize: fill a dense volume [z, y, x] of bytes 0 / 1 whose first voxel is world voxel lo = (x, y, z) from a
        triangle mesh -- a float32 tensor [n, 3, 3] on the scene's GPU (xyz per vertex, world voxel units), or (vertices [m, 3], faces
        [n, 3]), gathered with torch.  mode: "surface" (every voxel whose cube meets a triangle), "solid" (every voxel whose centre lies
        inside the closed mesh) or "solid+surface".  shape = (nz, ny, nx) for a new uint8 tensor, or `out`: a uint8 / bool CUDA tensor to
        fill (strides as in write_region); keep=True ORs into what `out` holds.  Returns (volume, VoxelizeResult); the result's
        open_columns is 0 for a closed mesh.  Stream handling as in write_region; the workspace comes from torch's pool; the host does
        not wait."""
        return self._voxelize(triangles, lo, shape, mode, keep, out, stream, False)[:2]

    def voxelize_times(self, triangles, lo, shape=None, mode="solid+surface", keep=False, out=None, stream=None):
        """bm_debug_voxelize_times: Scene.voxelize with a hipEvent between its stages; waits.  Returns (volume, VoxelizeResult, [ms of
        zeroing the workspace, plan + scan, the surface items, the solid items, the dense pass])."""
        return self._voxelize(triangles, lo, shape, mode, keep, out, stream, True)

    def write_mesh(self, triangles, op="set", mode="solid+surface", stream=None):
        """Voxelize a mesh (as Scene.voxelize takes it) over its own bounds, clipped to the world, and write_region the result: op "set"
        adds the mesh to the scene, "clear" carves it out.  The bounds are taken with torch and read by the host: one synchronisation, and
        the one thing this call waits for.  Triangles with a non-finite coordinate do not count for the bounds.  Returns (lo, hi,
        VoxelizeResult) -- the box written, (x, y, z), hi exclusive -- or (None, None, None) when nothing of the mesh lies in the world."""
        import torch
        tri = self._triangles(triangles)
        if tri.shape[0] == 0:
            return None, None, None
        finite = torch.isfinite(tri).all(dim=2).all(dim=1)
        pts = tri[finite].reshape(-1, 3).double()
        if pts.shape[0] == 0:
            return None, None, None
        bounds = torch.stack((torch.floor(pts.amin(dim=0)) - 1, torch.floor(pts.amax(dim=0)) + 1)).cpu().numpy()  # the voxels a cube of which can touch
        world = (self.grid_size, self.grid_size, self.grid_height)
        lo = [int(max(bounds[0][k], 0)) for k in range(3)]
        hi = [int(min(bounds[1][k], world[k])) for k in range(3)]
        if any(h <= l for l, h in zip(lo, hi)):
            return None, None, None
        volume, res = self.voxelize(tri, lo, (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]), mode=mode, stream=stream)
        self.write_region(lo, volume, op=op, stream=stream)
        return tuple(lo), tuple(hi), res

    # ---- voxels -> quads (bm_mesh_quads)
    def _mesh_quads(self, volume, lo, halo, unit, capacity, stream, times):
        import torch
        par, ptr = _device_volume("mesh_quads", volume, _mesh_params, lo, volume, halo, unit)
        dev = volume.device
        h = self._handoff(volume, stream)
        with h.on_target():
            ws = torch.empty(mesh_workspace_bytes(volume.shape, halo, lo), dtype=torch.uint8, device=dev)
            result = torch.empty(2, dtype=torch.int64, device=dev)
        h.reads(volume)

        def call(packed, cap):
            args = (self.gpuScene, C.byref(par), C.c_void_p(ptr), C.c_void_p(packed.data_ptr() if packed is not None else 0), cap, C.c_void_p(result.data_ptr()),
                    C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(h.handle))
            return stage_call(self._L.bm_mesh_quads, self._L.bm_debug_mesh_times, args, 3 if times else None)

        record = ms = None
        if capacity is None:
            ms = call(None, 0)
            with h.on_target():
                record = result.cpu().numpy().view(MESH_RESULT_DTYPE).reshape(())   # waits for the counting call
            capacity = int(record["quads"])
        capacity = int(capacity)
        with h.on_target():
            packed = torch.empty((capacity, 4), dtype=torch.int32, device=dev)
        if capacity > 0 or record is None:
            ms = call(packed if capacity > 0 else None, capacity)
        h.join()
        return Quads(self, packed, result, record), ms

    def mesh_quads(self, volume, lo=(0, 0, 0), halo=False, unit=False, capacity=None, stream=None):
        """bm_mesh_quads: the surface of a dense volume [z, y, x] -- a uint8 or bool tensor on the scene's GPU, non-zero =
        solid, strides as in write_region -- whose first voxel is world voxel lo = (x, y, z), as quads merged greedily inside the world's
        8^3 cells.  halo=True: the volume's outermost shell is context only, so neighbouring tiles share no wall; unit=True: one quad per
        face.  capacity=None makes the counting call, reads the total, allocates and emits: that read is one synchronisation, and the one
        thing this call waits for.  With a capacity the first `capacity` quads are written and the host does not wait.  Returns a Quads.
        Stream handling as in write_region; the workspace comes from torch's pool."""
        return self._mesh_quads(volume, lo, halo, unit, capacity, stream, False)[0]

    def mesh_quads_times(self, volume, lo=(0, 0, 0), halo=False, unit=False, capacity=None, stream=None):
        """bm_debug_mesh_times: Scene.mesh_quads with a hipEvent between its stages; waits.  Returns (Quads, [ms of count, scan, emit]) of
        the emitting call."""
        return self._mesh_quads(volume, lo, halo, unit, capacity, stream, True)

    def extract_mesh(self, lo, hi, closed=True, unit=False, stream=None):
        """The surface of the voxels lo <= v < hi (x, y, z) of the live scene as a Quads.  closed=True: read_region(lo, hi, device=True),
        meshed without flags -- everything outside the box is empty and the surface is closed.  closed=False: the box lo - 1 ... hi + 1 is
        read and meshed with a halo -- faces only where a voxel of the box meets an empty voxel, inside the box or beside it, so
        neighbouring boxes share no wall.  Waits once, for the quad count (see mesh_quads)."""
        lo, hi = _nonempty_box("extract_mesh", lo, hi)
        if not closed:
            lo, hi = [v - 1 for v in lo], [v + 1 for v in hi]
        volume = self.read_region(lo, hi, device=True, stream=stream)
        return self.mesh_quads(volume, lo, halo=not closed, unit=unit, stream=stream)

    # ---- voxels -> distances (bm_distance_field)
    def _distance_field(self, volume, to, outside, out, stream, times):
        import torch
        par, ptr = _device_volume("distance_field", volume, _distance_params, volume, to, outside)
        dev, shape = volume.device, tuple(int(v) for v in volume.shape)
        _int32_out("distance_field", out, shape)
        h = self._handoff(volume, stream)
        with h.on_target():
            if out is None:
                out = torch.empty(shape, dtype=torch.int32, device=dev)
            ws = torch.empty(distance_workspace_bytes(shape), dtype=torch.uint8, device=dev)
            result = torch.empty(4, dtype=torch.int64, device=dev)
        h.reads(volume, out)
        args = (self.gpuScene, C.byref(par), C.c_void_p(ptr), C.c_void_p(out.data_ptr()), C.c_void_p(result.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                C.c_void_p(h.handle))
        ms = stage_call(self._L.bm_distance_field, self._L.bm_debug_distance_times, args, 3 if times else None)
        h.join()
        return DistanceField(self, out, result), ms

    def distance_field(self, volume, to="solid", outside=False, out=None, stream=None):
        """bm_distance_field: the exact squared Euclidean distance of every voxel of a dense volume [z, y, x] -- a uint8 or
        bool tensor on the scene's GPU, non-zero = solid, strides as in write_region -- to the nearest source: the nearest solid voxel
        (to="solid") or the nearest empty one (to="empty"); outside=True counts every voxel outside the volume as a source too.  out: a
        contiguous int32 tensor of the volume's shape to fill.  Returns a DistanceField: .field (int32 [z, y, x], DISTANCE_NONE where there
        is no source), .record, .largest() and .mask(radius_sq, above=False); only .record and .largest() wait.  Stream handling as in
        write_region; the workspace (8 bytes per voxel) comes from torch's pool."""
        return self._distance_field(volume, to, outside, out, stream, False)[0]

    def distance_field_times(self, volume, to="solid", outside=False, out=None, stream=None):
        """bm_debug_distance_times: Scene.distance_field with a hipEvent between its stages; waits.  Returns (DistanceField, [ms of the x
        pass, the y pass, the z pass with the finishing thread])."""
        return self._distance_field(volume, to, outside, out, stream, True)

    def clearance(self, lo, hi, stream=None):
        """How far every voxel of the box lo <= v < hi (x, y, z) of the live scene is from the nearest solid voxel of the box:
        read_region(lo, hi, device=True), then distance_field(to="solid").  .largest() is the centre (relative to lo) and the squared
        radius of the largest empty ball."""
        lo, hi = _nonempty_box("clearance", lo, hi)
        return self.distance_field(self.read_region(lo, hi, device=True, stream=stream), stream=stream)

    def _near(self, lo, hi, limit_sq, reach_sq, to, stream):
        """(volume, mask) of the box: the box enlarged by ceil(sqrt(reach_sq)) on every side is read, its distance to `to` is taken and
        masked at D <= limit_sq, and both are cut back to the box -- the margin covers every source that can matter inside it"""
        m = math.isqrt(reach_sq - 1) + 1  # ceil(sqrt(reach_sq))
        volume = self.read_region([v - m for v in lo], [v + m for v in hi], device=True, stream=stream)
        inner = (slice(m, -m),) * 3
        return volume[inner], self.distance_field(volume, to=to, stream=stream).mask(limit_sq, stream=stream)[inner]

    def _morph(self, name, lo, hi, radius_sq, to, op, stream):
        radius_sq = int(radius_sq)
        if radius_sq < 1 or radius_sq > 3 * 16383 * 16383:
            raise ValueError(f"{name}: radius_sq, an integer in 1 ... 3 * 16383^2, expected, got {radius_sq}")
        lo, hi = _nonempty_box(name, lo, hi)
        volume, mask = self._near(lo, hi, radius_sq, radius_sq, to, stream)
        changed = (mask != 0) & ((volume != 0) if op == "clear" else (volume == 0))
        self.write_region(lo, mask, op=op, stream=stream)
        return int(changed.sum().item())

    def grow(self, lo, hi, radius_sq, stream=None):
        """Dilate the live scene inside the box lo <= v < hi (x, y, z) with a Euclidean ball of squared radius radius_sq (an integer >= 1):
        every voxel of the box within that distance of a solid voxel becomes solid.  The box enlarged by ceil(sqrt(radius_sq)) on every
        side is read (read_region gives 0 outside the world), its distance to solid is taken, and the mask D <= radius_sq of the box is
        written with op "set".  Because the margin covers the radius, the result inside the box equals the morphological operation on
        the whole world restricted to the box; beyond the world's border counts as empty.  Returns the number of voxels changed (read
        with torch: the host waits)."""
        return self._morph("grow", lo, hi, radius_sq, "solid", "set", stream)

    def shrink(self, lo, hi, radius_sq, stream=None):
        """Erode the live scene inside the box lo <= v < hi with a Euclidean ball of squared radius radius_sq (an integer >= 1): every
        voxel of the box within that distance of an empty voxel becomes empty -- the distance to empty of the enlarged box, the mask
        D <= radius_sq, write_region with op "clear".  As for grow the margin covers the radius, and beyond the world's border counts as
        empty, so solid voxels at the border erode.  Returns the number of voxels changed."""
        return self._morph("shrink", lo, hi, radius_sq, "empty", "clear", stream)

    # ---- voxels + seeds -> shortest face-step distances (bm_travel_field)
    def _travel_field(self, volume, seeds, max_steps, out, stream, times, batch=0):
        import torch
        par, ptr = _device_volume("travel_field", volume, _travel_params, volume, max_steps)
        dev, shape = volume.device, tuple(int(v) for v in volume.shape)
        _int32_out("travel_field", out, shape)
        h = self._handoff(volume, stream)
        with h.on_target():
            seeds = _device_points("travel_field", "seeds", seeds, dev)
            if out is None:
                out = torch.empty(shape, dtype=torch.int32, device=dev)
            ws = torch.empty(travel_workspace_bytes(shape), dtype=torch.uint8, device=dev)
            result = torch.empty(4, dtype=torch.int64, device=dev)
        n = int(seeds.shape[0])
        h.reads(volume, seeds, out)
        args = (self.gpuScene, C.byref(par), C.c_void_p(ptr), C.c_void_p(seeds.data_ptr() if n else None), n, C.c_void_p(out.data_ptr()), C.c_void_p(result.data_ptr()),
                C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(h.handle))
        counts = (C.c_uint32 * 2)()
        ms = stage_call(self._L.bm_travel_field, self._L.bm_debug_travel_times, args, 3 if times else None, before=(int(batch),), after=(counts,))
        h.join()
        return TravelField(self, out, result), ((ms, int(counts[0]), int(counts[1])) if times else None)

    def travel_field(self, volume, seeds, max_steps=0, out=None, stream=None):
        """bm_travel_field: the least number of face steps from any accepted seed to every voxel of a dense volume
        [z, y, x] -- a uint8 or bool tensor on the scene's GPU, non-zero = blocked, strides as in write_region -- through voxels that are
        not blocked.  seeds: [n, 3] of (x, y, z) in the volume's coordinates (a list, a numpy array or an int32 tensor on the GPU); a seed
        outside the volume or on a blocked voxel is counted and ignored.  max_steps: 0 = no limit.  out: a contiguous int32 tensor of the
        volume's shape to fill.  Returns a TravelField: .field (int32 [z, y, x], TRAVEL_NONE where there is no value), .record,
        .paths(starts, capacity) and .path(start).  Unlike its siblings the call returns when the field stands: it waits on the stream
        between batches of rounds.  Stream handling as in write_region; the workspace (76 bytes per 8^3 tile) comes from torch's pool."""
        return self._travel_field(volume, seeds, max_steps, out, stream, False)[0]

    def travel_field_times(self, volume, seeds, max_steps=0, out=None, stream=None, batch=0):
        """bm_debug_travel_times: Scene.travel_field with a hipEvent between its stages and `batch` rounds between two looks of the host
        (0 = the default).  Returns (TravelField, ([ms of the set-up, the rounds, the finish], rounds, looks))."""
        return self._travel_field(volume, seeds, max_steps, out, stream, True, batch)

    def _blocked_box(self, name, lo, hi, clearance_sq, stream):
        lo, hi = _nonempty_box(name, lo, hi)
        clearance_sq = int(clearance_sq)
        if clearance_sq < 0 or clearance_sq > 3 * 16383 * 16383:
            raise ValueError(f"{name}: clearance_sq, an integer in 0 ... 3 * 16383^2, expected, got {clearance_sq}")
        if clearance_sq == 0:
            return self.read_region(lo, hi, device=True, stream=stream)
        return self._near(lo, hi, clearance_sq - 1, clearance_sq, "solid", stream)[1]

    def reach(self, lo, hi, seeds, clearance_sq=0, max_steps=0, stream=None):
        """How many face steps every voxel of the box lo <= v < hi (x, y, z) of the live scene is from the nearest of `seeds` ([n, 3] WORLD
        voxels) without leaving the box: read_region(lo, hi, device=True), then travel_field.  With clearance_sq >= 1 a voxel is blocked
        when a solid voxel lies closer than that squared distance -- where an agent of that squared radius does not fit: the distance to
        solid of the box enlarged by ceil(sqrt(clearance_sq)) (read_region gives 0 outside the world, as for grow), masked at
        clearance_sq - 1 and cut back to the box.  Returns a TravelField in the box's coordinates (voxel - lo)."""
        blocked = self._blocked_box("reach", lo, hi, clearance_sq, stream)
        pts = _points(seeds, "reach") - np.asarray([int(v) for v in lo], np.int32)
        return self.travel_field(blocked, pts, max_steps=max_steps, stream=stream)

    def find_path(self, start, goal, lo=None, hi=None, clearance_sq=0, max_steps=0, stream=None):
        """A shortest face-step path from world voxel `start` to world voxel `goal` inside the box lo <= v < hi (default: the bounding box
        of the two enlarged by 32 and clipped to the world): reach() seeded at the goal, then the walk down from the start.  Returns an
        int32 numpy array [length, 3] of world voxels, the start first and the goal last, or None when there is no path (within
        max_steps).  Ordered like a query: it sees every edit issued before.  The host waits."""
        start, goal = [int(v) for v in start], [int(v) for v in goal]
        world = (self.grid_size, self.grid_size, self.grid_height)
        if lo is None:
            lo = [max(min(s, g) - 32, 0) for s, g in zip(start, goal)]
        if hi is None:
            hi = [min(max(s, g) + 33, w) for s, g, w in zip(start, goal, world)]
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if any(h <= l for l, h in zip(lo, hi)):
            return None
        path = self.reach(lo, hi, [goal], clearance_sq, max_steps, stream).path([s - l for s, l in zip(start, lo)])
        return None if path is None else path + np.asarray(lo, np.int32)
