"""Ground navigation (bm_foot_room, bm_foot_field, bm_foot_paths): exact walk fields and paths for an agent that stands on
solid ground, is `height` voxels tall, climbs `climb` and drops `drop`.  Free functions on a scene; the package and brickmap_amd.host
export none of them: `from brickmap_amd import foot`."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FOOT_RESULT_DTYPE, check, size_call, stage_call
from .volumes import DeviceRecord, _device_points, _device_volume, _int32_out, _points, dense_layout, record_of
from .world import region_of

FOOT_NONE = _lib.BM_FOOT_NONE
SUPPORTED, ROOM = 0x80, 0x7F   # a room byte: bit 7 and the free voxels from this one upwards


def _agent(par, height, climb, drop, toward=False, floor=True, max_steps=0):
    """the agent's part of a bm_foot_params; what the library would refuse is raised here"""
    height, climb, drop, max_steps = int(height), int(climb), int(drop), int(max_steps)
    if not (1 <= height <= 32 and 0 <= climb <= 32 and 0 <= drop <= 64):
        raise ValueError(f"foot: height in 1 ... 32, climb in 0 ... 32 and drop in 0 ... 64 expected, got {height}, {climb}, {drop}")
    if not 0 <= max_steps <= 0xFFFFFFFF:
        raise ValueError(f"foot: max_steps in 0 ... 2^32 - 1 expected (0 = no limit), got {max_steps}")
    par.height, par.climb, par.drop, par.max_steps = height, climb, drop, max_steps
    par.flags = (_lib.BM_FOOT_TOWARD if toward else 0) | (0 if floor else _lib.BM_FOOT_NO_FLOOR)
    return par


def _volume_params(volume, name="volume"):
    """(bm_foot_params, data pointer, is_cuda) of a byte volume [z, y, x], laid out as region_of takes it"""
    r, ptr, cuda = region_of((0, 0, 0), volume, name)
    return dense_layout(_lib.bm_foot_params(), r), ptr, cuda


def _tight_params(shape):
    par = _lib.bm_foot_params()
    par.extent[:] = [int(v) for v in tuple(shape)[::-1]]
    return par


def _host_room(room, who):
    room = np.ascontiguousarray(room)
    if room.dtype != np.dtype(np.uint8) or room.ndim != 3 or min(room.shape) == 0:
        raise ValueError(f"{who}: a uint8 room volume [z, y, x] with positive extents expected, got {room.dtype} {room.shape}")
    return room


def foot_workspace_bytes(shape):
    """bm_foot_workspace_bytes: device memory bm_foot_field needs beside its buffers for a volume of shape (nz, ny, nx): 4 bytes for each
    of ceil(nz / 2) * ny * nx queue entries, plus 64."""
    return size_call("bm_foot_workspace_bytes", C.byref(_agent(_tight_params(shape), 1, 0, 0)))


def host_foot_room(volume, floor=True):
    """bm_host_foot_room (host only, no device): the room bytes of a dense volume [z, y, x] (uint8 or bool numpy array, non-zero = blocked,
    z up; a slice of a larger array works as long as x is contiguous).  Returns a uint8 array [z, y, x]: the low 7 bits count the free
    voxels from this one upwards (capped at 127, everything above the volume is free), bit 7 says that the voxel is free and stands on a
    blocked one -- or, with floor=True, on the bottom of the volume."""
    par, ptr, cuda = _volume_params(volume)
    assert not cuda
    if min(volume.shape) == 0:
        raise ValueError(f"host_foot_room: a volume with positive extents expected, got shape {tuple(volume.shape)}")
    room = np.zeros(tuple(volume.shape), np.uint8)
    check(_lib.load().bm_host_foot_room(C.byref(_agent(par, 1, 0, 0, floor=floor)), C.c_void_p(ptr), C.c_void_p(room.ctypes.data)))
    return room


def host_foot_field(room, seeds, height=2, climb=1, drop=3, toward=False, max_steps=0):
    """bm_host_foot_field (host only): the least number of moves from any accepted seed to every stand of `room` (host_foot_room's), or
    with toward=True from every stand to a seed, as a plain queue search.  seeds: [n, 3] of (x, y, z).  Returns (field, record): an int32
    array [z, y, x] (FOOT_NONE where there is no stand, no way or more than max_steps moves) and a FOOT_RESULT_DTYPE record."""
    room = _host_room(room, "host_foot_field")
    par = _agent(_tight_params(room.shape), height, climb, drop, toward, max_steps=max_steps)
    pts = _points(seeds, "host_foot_field")
    field = np.zeros(room.shape, np.int32)
    res = _lib.bm_foot_result()
    check(_lib.load().bm_host_foot_field(C.byref(par), C.c_void_p(room.ctypes.data), C.c_void_p(pts.ctypes.data if len(pts) else None), len(pts), C.c_void_p(field.ctypes.data),
                                         C.byref(res)))
    return field, record_of(res)


def host_foot_paths(room, field, starts, capacity, height=2, climb=1, drop=3, toward=False):
    """bm_host_foot_paths (host only): walks down an int32 / uint32 field [z, y, x] from every start ([n, 3] of (x, y, z)) by legal moves
    only.  Returns (path, lengths): int32 [n, capacity, 3], of which the first min(length, capacity) voxels of every path are written
    (the rest is -1), and int32 [n]: W(start) + 1, 0 for a start outside the volume or without a finite value, -1 where no legal move
    leads down."""
    room = _host_room(room, "host_foot_paths")
    field = np.ascontiguousarray(field)
    if field.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)) or field.shape != room.shape:
        raise ValueError(f"host_foot_paths: an int32 or uint32 field of the room's shape expected, got {field.dtype} {field.shape}")
    par = _agent(_tight_params(room.shape), height, climb, drop, toward)
    pts = _points(starts, "host_foot_paths")
    capacity = int(capacity)
    path = np.full((len(pts), max(capacity, 0), 3), -1, np.int32)
    lengths = np.zeros(len(pts), np.int32)
    check(_lib.load().bm_host_foot_paths(C.byref(par), C.c_void_p(room.ctypes.data), C.c_void_p(field.ctypes.data), C.c_void_p(pts.ctypes.data if len(pts) else None), len(pts),
                                         capacity, C.c_void_p(path.ctypes.data if path.size else None), C.c_void_p(lengths.ctypes.data if len(pts) else None)))
    return path, lengths


def foot_room(scene, volume, floor=True, stream=None):
    """bm_foot_room: the room bytes (see host_foot_room) of a dense volume [z, y, x] -- a uint8 or bool tensor on the scene's GPU, non-zero
    = blocked, strides as in write_region.  Returns a contiguous uint8 tensor of the volume's shape.  The host does not wait."""
    import torch
    par, ptr = _device_volume("foot_room", volume, _volume_params, volume)
    _agent(par, 1, 0, 0, floor=floor)
    h = scene._handoff(volume, stream)
    with h.on_target():
        room = torch.empty(tuple(int(v) for v in volume.shape), dtype=torch.uint8, device=volume.device)
    h.reads(volume, room)
    check(scene._L.bm_foot_room(scene.gpuScene, C.byref(par), C.c_void_p(ptr), C.c_void_p(room.data_ptr()), C.c_void_p(h.handle)))
    h.join()
    return room


class FootField(DeviceRecord):
    """The field of a foot_field: `field` is the int32 tensor [z, y, x] on the device (FOOT_NONE where there is no stand, no way or more
    than max_steps moves), `room` the room bytes it was made from and `result` the bm_foot_result there (four int64 words).  The field
    stands when foot_field returns.  record (a FOOT_RESULT_DTYPE scalar), path() and ground() copy to the host, which waits; paths()
    stays on the device."""
    _record_dtype = FOOT_RESULT_DTYPE

    def __init__(self, scene, field, room, result, agent):
        self.scene, self.field, self.room, self.result, self.agent = scene, field, room, result, agent

    reached = property(lambda self: int(self.record["reached"]))
    standable = property(lambda self: int(self.record["standable"]))

    def paths(self, starts, capacity, stream=None):
        """bm_foot_paths: from every start ([n, 3] of (x, y, z) in the volume's coordinates; a list, a numpy array or an int32 tensor on
        the scene's GPU) down the field by legal moves.  Returns (path, lengths), int32 tensors [n, capacity, 3] and [n] on the device:
        the first min(length, capacity) voxels of every path, the start first (the rest is -1); lengths as in host_foot_paths.  With
        toward=True a path is the walk from the start to a seed, otherwise the walk from a seed reversed.  The host does not wait."""
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
        h.reads(self.field, self.room, starts, path, lengths)
        par = _agent(_tight_params(self.field.shape), **self.agent)
        check(self.scene._L.bm_foot_paths(self.scene.gpuScene, C.byref(par), C.c_void_p(self.room.data_ptr()), C.c_void_p(self.field.data_ptr()),
                                          C.c_void_p(starts.data_ptr() if n else None), n, capacity, C.c_void_p(path.data_ptr() if n else None),
                                          C.c_void_p(lengths.data_ptr() if n else None), C.c_void_p(h.handle)))
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
        if t == FOOT_NONE:
            return None
        path, lengths = self.paths([(x, y, z)], t + 1)
        if int(lengths[0].item()) != t + 1:
            raise RuntimeError("path: the field was not made from this room by these parameters")
        return path[0].cpu().numpy()

    def ground(self, points):
        """The highest stand at or below each point ([n, 3] of (x, y, z)) in its column: a list of (x, y, z) tuples, None where the point
        is outside the volume or its column has no stand at or below it.  A few torch operations on `room`, not a kernel; waits."""
        return ground(self.room, points, self.agent["height"])


def ground(room, points, height):
    """FootField.ground on a room tensor (or numpy array) [z, y, x] for an agent of `height`"""
    import torch
    room = torch.as_tensor(room)
    nz, ny, nx = room.shape
    out = []
    for x, y, z in _points(points, "ground").tolist():
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
            out.append(None)
            continue
        column = room[: z + 1, y, x]
        stands = torch.nonzero(((column & SUPPORTED) != 0) & ((column & ROOM) >= int(height))).reshape(-1)
        out.append((x, y, int(stands.max().item())) if stands.numel() else None)
    return out


def _foot_field(scene, room, seeds, height, climb, drop, toward, max_steps, out, stream, times, batch=0):
    import torch
    if not hasattr(room, "is_cuda") or not room.is_cuda or room.dtype != torch.uint8 or room.dim() != 3 or not room.is_contiguous() or min(room.shape) == 0:
        raise ValueError("foot_field: room must be a contiguous uint8 tensor [z, y, x] with positive extents on the scene's GPU (foot_room's)")
    agent = dict(height=int(height), climb=int(climb), drop=int(drop), toward=bool(toward), max_steps=int(max_steps))
    dev, shape = room.device, tuple(int(v) for v in room.shape)
    par = _agent(_tight_params(shape), **agent)
    _int32_out("foot_field", out, shape)
    h = scene._handoff(room, stream)
    with h.on_target():
        seeds = _device_points("foot_field", "seeds", seeds, dev)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=dev)
        ws = torch.empty(foot_workspace_bytes(shape), dtype=torch.uint8, device=dev)
        result = torch.empty(4, dtype=torch.int64, device=dev)
    n = int(seeds.shape[0])
    h.reads(room, seeds, out)
    args = (scene.gpuScene, C.byref(par), C.c_void_p(room.data_ptr()), C.c_void_p(seeds.data_ptr() if n else None), n, C.c_void_p(out.data_ptr()), C.c_void_p(result.data_ptr()),
            C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(h.handle))
    counts = (C.c_uint32 * 2)()
    ms = stage_call(scene._L.bm_foot_field, scene._L.bm_debug_foot_times, args, 3 if times else None, before=(int(batch),), after=(counts,))
    h.join()
    agent.pop("max_steps")
    return FootField(scene, out, room, result, agent), ((ms, int(counts[0]), int(counts[1])) if times else None)


def foot_field(scene, room, seeds, height=2, climb=1, drop=3, toward=False, max_steps=0, out=None, stream=None):
    """bm_foot_field: the least number of moves of a walk from any accepted seed to every stand of `room` (foot_room's
    tensor) for an agent `height` voxels tall that climbs `climb` and drops `drop` voxels per move; with toward=True the least number of
    moves from every stand to a seed.  seeds: [n, 3] of (x, y, z) in the volume's coordinates (a list, a numpy array or an int32 tensor on
    the GPU); a seed that is outside the volume or on no stand is counted and ignored.  max_steps: 0 = no limit.  Returns a FootField:
    .field (int32 [z, y, x], FOOT_NONE where there is no value), .room, .record, .paths(starts, capacity), .path(start) and
    .ground(points).  Like Scene.travel_field the call returns when the field stands: it waits on the stream between batches of rounds.
    Stream handling as in write_region; the workspace (at most 2 bytes per voxel) comes from torch's pool."""
    return _foot_field(scene, room, seeds, height, climb, drop, toward, max_steps, out, stream, False)[0]


def foot_field_times(scene, room, seeds, height=2, climb=1, drop=3, toward=False, max_steps=0, out=None, stream=None, batch=0):
    """bm_debug_foot_times: foot_field with a hipEvent between its stages and `batch` rounds between two looks of the host (0 = the
    default).  Returns (FootField, ([ms of the set-up, the rounds, the finish], rounds, looks))."""
    return _foot_field(scene, room, seeds, height, climb, drop, toward, max_steps, out, stream, True, batch)


def find_walk(scene, start, goal, lo=None, hi=None, height=2, climb=1, drop=3, stream=None):
    """A shortest walk from world voxel `start` to world voxel `goal` inside the box lo <= v < hi (default: the bounding box of the two
    enlarged by 32, taken down by `drop` more and clipped to the world): read_region(lo, hi, device=True), the room bytes with the floor
    where the box stands on the world's bottom, both ends snapped to the ground under them, the field toward the goal, then the walk
    from the start.  Returns an int32 numpy array [length, 3] of world voxels, the start's ground first and the goal's last, or None
    when there is no way on foot.  Ordered like a query: it sees every edit issued before.  The host waits."""
    start, goal = [int(v) for v in start], [int(v) for v in goal]
    world = (scene.grid_size, scene.grid_size, scene.grid_height)
    if lo is None:
        lo = [max(min(s, g) - 32, 0) for s, g in zip(start, goal)]
        lo[2] = max(lo[2] - int(drop), 0)
    if hi is None:
        hi = [min(max(s, g) + 33, w) for s, g, w in zip(start, goal, world)]
    lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    if any(h <= l for l, h in zip(lo, hi)):
        return None
    room = foot_room(scene, scene.read_region(lo, hi, device=True, stream=stream), floor=lo[2] == 0, stream=stream)
    ends = ground(room, [[s - l for s, l in zip(start, lo)], [g - l for g, l in zip(goal, lo)]], height)
    if ends[0] is None or ends[1] is None:
        return None
    path = foot_field(scene, room, [ends[1]], height, climb, drop, toward=True, stream=stream).path(ends[0])
    return None if path is None else path + np.asarray(lo, np.int32)
