"""Where water stands (bm_water_field, bm_water_mask): exact spill levels and pools of a dense voxel volume [z, y, x], z
up.  Free functions on a scene; the package and brickmap_amd.host export none of them: `from brickmap_amd import water`."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import WATER_RESULT_DTYPE, check, stage_call
from .volumes import DeviceRecord, _device_points, _device_volume, _int32_out, _nonempty_box, _points, _workspace_bytes, dense_layout, record_of
from .world import region_of

WATER_NONE = _lib.BM_WATER_NONE
SIDES = ("-x", "+x", "-y", "+y")   # the default open faces: water runs off over the four sides of the box


def _flags(open):
    """the face bits of `open`: names out of -x, +x, -y, +y, -z, +z (or the bits themselves)"""
    if isinstance(open, (int, np.integer)):
        return int(open)
    if isinstance(open, str):
        open = (open,)
    bad = [f for f in open if f not in _lib.BM_WATER_FACES]
    if bad:
        raise ValueError(f"water: open faces out of {tuple(_lib.BM_WATER_FACES)} expected, got {bad}")
    return sum({_lib.BM_WATER_FACES[f] for f in open})


def _water_params(volume, open, sea_level, name="volume"):
    """(bm_water_params, data pointer, is_cuda) of `volume` ([z, y, x], laid out as region_of takes it)"""
    if not 0 <= int(sea_level) <= 0xFFFFFFFF:
        raise ValueError(f"water: sea_level in 0 ... nz expected (0 = none), got {sea_level}")
    r, ptr, cuda = region_of((0, 0, 0), volume, name)
    par = dense_layout(_lib.bm_water_params(), r)
    par.sea_level, par.flags = int(sea_level), _flags(open)
    return par, ptr, cuda


def _extent(shape):
    return (C.c_int32 * 3)(*[int(v) for v in tuple(shape)[::-1]])


def water_workspace_bytes(shape):
    """bm_water_workspace_bytes: device memory bm_water_field needs beside its buffers for a volume of shape (nz, ny, nx): what
    travel_workspace_bytes gives."""
    return _workspace_bytes("water", _lib.bm_water_params(), shape)


def host_water_field(volume, drains=None, open=SIDES, sea_level=0):
    """bm_host_water_field (host only, no device): the spill level of every voxel of a dense volume [z, y, x] (uint8 or bool numpy array,
    non-zero = solid, z up; a slice of a larger array works as long as x is contiguous), as a plain priority flood.  Outlets are the free
    voxels on the `open` faces of the box and the accepted drains ([n, 3] of (x, y, z)); sea_level: box-local z, 0 = none.  Returns
    (field, record): an int32 array [z, y, x] (WATER_NONE where solid or closed) and a WATER_RESULT_DTYPE record."""
    par, ptr, cuda = _water_params(volume, open, sea_level)
    assert not cuda
    if min(volume.shape) == 0:
        raise ValueError(f"host_water_field: a volume with positive extents expected, got shape {tuple(volume.shape)}")
    pts = _points([] if drains is None else drains, "host_water_field")
    field = np.zeros(tuple(volume.shape), np.int32)
    res = _lib.bm_water_result()
    check(_lib.load().bm_host_water_field(C.byref(par), C.c_void_p(ptr), C.c_void_p(pts.ctypes.data if len(pts) else None), len(pts), C.c_void_p(field.ctypes.data), C.byref(res)))
    return field, record_of(res)


def host_water_mask(field, min_depth=1):
    """bm_host_water_mask (host only): a uint8 array [z, y, x], 1 where the voxel of an int32 / uint32 field is wet and at least min_depth
    deep, otherwise 0."""
    field = np.ascontiguousarray(field)
    if field.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)) or field.ndim != 3 or min(field.shape) == 0:
        raise ValueError(f"host_water_mask: an int32 or uint32 field [z, y, x] with positive extents expected, got {field.dtype} {field.shape}")
    if not 1 <= int(min_depth) <= 0xFFFFFFFF:
        raise ValueError(f"host_water_mask: a min_depth of at least 1 expected, got {min_depth}")
    mask = np.zeros(field.shape, np.uint8)
    check(_lib.load().bm_host_water_mask(_extent(field.shape), C.c_void_p(field.ctypes.data), int(min_depth), C.c_void_p(mask.ctypes.data)))
    return mask


class WaterField(DeviceRecord):
    """The field of a water_field: `field` is the int32 tensor [z, y, x] on the device (WATER_NONE where solid or closed; dry where it
    equals the voxel's z, wet where it is larger) and `result` the bm_water_result there (four int64 words).  `lo` is the world voxel of
    the field's voxel [0, 0, 0] when it came from pools().  The field stands when water_field returns.  record (a WATER_RESULT_DTYPE
    scalar), wet, closed and deepest() copy to the host, which waits; mask() stays on the device."""
    _record_dtype = WATER_RESULT_DTYPE

    def __init__(self, scene, field, result, lo=(0, 0, 0)):
        self.scene, self.field, self.result, self.lo = scene, field, result, tuple(int(v) for v in lo)

    wet = property(lambda self: int(self.record["wet"]))
    closed = property(lambda self: int(self.record["closed"]))

    def deepest(self):
        """((x, y, z), depth) of the deepest wet voxel in the field's coordinates, the lowest linear index among equals; None when nothing
        is wet"""
        depth = int(self.record["deepest"])
        if depth == 0:
            return None
        nz, ny, nx = self.field.shape
        at = int(self.record["deepest_at"])
        return (at % nx, at // nx % ny, at // (nx * ny)), depth

    def mask(self, min_depth=1, out=None, stream=None):
        """bm_water_mask: a uint8 tensor of the field's shape, 1 where the voxel is wet and at least min_depth deep -- what write_region
        and mesh_quads take.  out: a contiguous uint8 tensor of that shape to fill.  The host does not wait."""
        import torch
        if not 1 <= int(min_depth) <= 0xFFFFFFFF:
            raise ValueError(f"mask: a min_depth of at least 1 expected, got {min_depth}")
        shape = tuple(int(v) for v in self.field.shape)
        if out is not None and (not hasattr(out, "is_cuda") or not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError(f"mask: out must be a contiguous uint8 tensor of shape {shape} on the scene's GPU")
        h = self.scene._handoff(self.field, stream)
        with h.on_target():
            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=self.field.device)
        h.reads(self.field, out)
        check(self.scene._L.bm_water_mask(self.scene.gpuScene, _extent(shape), C.c_void_p(self.field.data_ptr()), int(min_depth), C.c_void_p(out.data_ptr()), C.c_void_p(h.handle)))
        h.join()
        return out


def _water_field(scene, volume, drains, open, sea_level, out, stream, times, batch=0, lo=(0, 0, 0)):
    import torch
    par, ptr = _device_volume("water_field", volume, _water_params, volume, open, sea_level)
    dev, shape = volume.device, tuple(int(v) for v in volume.shape)
    _int32_out("water_field", out, shape)
    h = scene._handoff(volume, stream)
    with h.on_target():
        drains = _device_points("water_field", "drains", [] if drains is None else drains, dev)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=dev)
        ws = torch.empty(water_workspace_bytes(shape), dtype=torch.uint8, device=dev)
        result = torch.empty(4, dtype=torch.int64, device=dev)
    n = int(drains.shape[0])
    h.reads(volume, drains, out)
    args = (scene.gpuScene, C.byref(par), C.c_void_p(ptr), C.c_void_p(drains.data_ptr() if n else None), n, C.c_void_p(out.data_ptr()), C.c_void_p(result.data_ptr()),
            C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(h.handle))
    counts = (C.c_uint32 * 3)()
    ms = stage_call(scene._L.bm_water_field, scene._L.bm_debug_water_times, args, 3 if times else None, before=(int(batch),), after=(counts,))
    h.join()
    return WaterField(scene, out, result, lo), ((ms, int(counts[0]), int(counts[1]), int(counts[2])) if times else None)


def water_field(scene, volume, drains=None, open=SIDES, sea_level=0, out=None, stream=None):
    """bm_water_field: the spill level of every voxel of a dense volume [z, y, x] -- a uint8 or bool tensor on the scene's
    GPU, non-zero = solid, z up, strides as in write_region.  Outlets are the free voxels on the `open` faces of the box (names out of -x,
    +x, -y, +y, -z, +z) and the accepted drains ([n, 3] of (x, y, z) in the volume's coordinates: a list, a numpy array or an int32 tensor
    on the GPU; one outside the volume or on a solid voxel is counted and ignored).  sea_level: box-local z, 0 = none.  out: a contiguous
    int32 tensor of the volume's shape to fill.  Returns a WaterField: .field (int32 [z, y, x]), .record, .wet, .closed, .deepest() and
    .mask(min_depth).  Like Scene.travel_field the call returns when the field stands: it waits on the stream between batches of rounds.
    Stream handling as in write_region; the workspace (76 bytes per 8^3 tile) comes from torch's pool."""
    return _water_field(scene, volume, drains, open, sea_level, out, stream, False)[0]


def water_field_times(scene, volume, drains=None, open=SIDES, sea_level=0, out=None, stream=None, batch=0):
    """bm_debug_water_times: water_field with a hipEvent between its stages and `batch` rounds between two looks of the host (0 = the
    default).  Returns (WaterField, ([ms of the set-up, the rounds, the finish], rounds, looks, tile visits))."""
    return _water_field(scene, volume, drains, open, sea_level, out, stream, True, batch)


def pools(scene, lo, hi, drains=None, open=SIDES, sea_level=None, stream=None):
    """Where water stands in the box lo <= v < hi (x, y, z) of the live scene: read_region(lo, hi, device=True), then water_field.  drains
    ([n, 3]) and sea_level (None = none) are in WORLD voxels; the sea is clamped into the box.  Returns a WaterField in the box's
    coordinates (voxel - lo) that carries `lo`.  Ordered like a query: it sees every edit issued before."""
    lo, hi = _nonempty_box("pools", lo, hi)
    volume = scene.read_region(lo, hi, device=True, stream=stream)
    pts = _points([] if drains is None else drains, "pools") - np.asarray(lo, np.int32)
    sea = 0 if sea_level is None else min(max(int(sea_level) - lo[2], 0), hi[2] - lo[2])
    return _water_field(scene, volume, pts, open, sea, None, stream, False, lo=lo)[0]
