"""Rigid settling (bm_settle): the chosen pieces of a label volume fall straight down, each as one rigid body, and land.
The step between Scene.components and Scene.write_region.  Free functions on a scene; the package and brickmap_amd.host export none of
them: `from brickmap_amd import settle`."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import COMPONENT_DTYPE, SETTLE_RESULT_DTYPE, check, size_call, stage_call
from .volumes import record_of

ANCHOR = ("-x", "+x", "-y", "+y", "-z")


def _extent(shape, who):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3:
        raise ValueError(f"{who}: a shape (nz, ny, nx) expected, got {shape}")
    return (C.c_int32 * 3)(*shape[::-1])


def _table(records, chosen, who):
    """(records, chosen) as contiguous arrays of COMPONENT_DTYPE and uint8, one byte per record"""
    records = np.ascontiguousarray(records)
    if records.dtype != COMPONENT_DTYPE or records.ndim != 1:
        raise ValueError(f"{who}: records must be a one-dimensional array of COMPONENT_DTYPE, got {records.dtype} {records.shape}")
    chosen = (np.asarray(chosen).reshape(-1) != 0).astype(np.uint8)
    if len(chosen) != len(records):
        raise ValueError(f"{who}: one value per record expected ({len(records)}), got {len(chosen)}")
    return records, chosen


def settle_workspace_bytes(n, shape):
    """bm_settle_workspace_bytes: device memory bm_settle needs beside its buffers for n records and a volume of shape (nz, ny, nx):
    4 bytes per record and 4 per 64 columns, none per voxel."""
    return size_call("bm_settle_workspace_bytes", _extent(shape, "settle_workspace_bytes"), int(n))


def host_settle(labels, records, chosen):
    """bm_host_settle (host only, no device): labels is an int32 array [z, y, x] (0 = empty, equal values = one rigid piece), records an
    array of COMPONENT_DTYPE in ascending label, chosen one value per record (non-zero = the piece may fall).  Returns (out, drops,
    record): uint8 [z, y, x] with 1 where a voxel stayed and 2 where one arrived by falling, int32 drops per record, and a
    SETTLE_RESULT_DTYPE record.  The floor is the bottom of the volume."""
    labels = np.asarray(labels)
    if labels.dtype != np.dtype(np.int32) or labels.ndim != 3:
        raise ValueError(f"host_settle: an int32 array [z, y, x] expected, got {labels.dtype} of shape {labels.shape}")
    labels = np.ascontiguousarray(labels)
    records, chosen = _table(records, chosen, "host_settle")
    n = len(records)
    out = np.zeros(labels.shape, np.uint8)
    drops = np.zeros(n, np.int32)
    res = _lib.bm_settle_result()
    check(_lib.load().bm_host_settle(_extent(labels.shape, "host_settle"), C.c_void_p(labels.ctypes.data), C.c_void_p(records.ctypes.data if n else None), n,
                                     C.c_void_p(chosen.ctypes.data if n else None), C.c_void_p(out.ctypes.data), C.c_void_p(drops.ctypes.data if n else None), C.byref(res)))
    return out, drops, record_of(res)


class Settled:
    """Result of settle: `out` (uint8 tensor [z, y, x] on the device: 0 empty, 1 stayed, 2 arrived by falling -- what write_region's
    replace takes), `drops` (numpy int32, one per record, 0 for records not chosen) and `record` (a SETTLE_RESULT_DTYPE scalar).  All
    stand when settle returns."""

    def __init__(self, out, drops, record):
        self.out, self.drops, self.record = out, drops, record

    moved_pieces = property(lambda self: int(self.record["moved_pieces"]))
    moved_voxels = property(lambda self: int(self.record["moved_voxels"]))
    largest_drop = property(lambda self: int(self.record["largest_drop"]))


def _settle(scene, labels, records, chosen, stream, times, batch=0):
    import torch
    if not hasattr(labels, "is_cuda") or not labels.is_cuda or labels.dtype != torch.int32 or labels.dim() != 3 or not labels.is_contiguous():
        raise ValueError("settle: labels must be a contiguous int32 tensor [z, y, x] on the scene's GPU")
    shape = tuple(int(v) for v in labels.shape)
    if min(shape) == 0:
        raise ValueError(f"settle: a volume with positive extents expected, got shape {shape}")
    records, chosen = _table(records, chosen, "settle")
    n, dev = len(records), labels.device
    h = scene._handoff(labels, stream)
    with h.on_target():
        table = torch.from_numpy(records.view(np.int64).reshape(-1).copy()).to(dev) if n else None
        d_chosen = torch.from_numpy(chosen).to(dev) if n else None
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
        d_drops = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        ws = torch.empty(settle_workspace_bytes(n, shape), dtype=torch.uint8, device=dev)
        result = torch.empty(4, dtype=torch.int64, device=dev)
    h.reads(labels)
    ptr = lambda t: C.c_void_p(t.data_ptr() if n else None)
    args = (scene.gpuScene, _extent(shape, "settle"), C.c_void_p(labels.data_ptr()), ptr(table), n, ptr(d_chosen), C.c_void_p(out.data_ptr()), ptr(d_drops),
            C.c_void_p(result.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), 0, C.c_void_p(h.handle))
    counts = (C.c_uint32 * 2)()
    ms = stage_call(scene._L.bm_settle, scene._L.bm_debug_settle_times, args, 3 if times else None, before=(int(batch),), after=(counts,))
    with h.on_target():  # the call has returned: the result stands
        drops = d_drops[:n].cpu().numpy()
        record = result.cpu().numpy().view(SETTLE_RESULT_DTYPE).reshape(())
    h.join()
    return Settled(out, drops, record), ((ms, int(counts[0]), int(counts[1])) if times else None)


def settle_volume(scene, labels, records, chosen, stream=None):
    """bm_settle on a label volume of the caller's: labels is a contiguous int32 tensor [z, y, x] on the scene's GPU, records and chosen
    as host_settle takes them.  Returns a Settled.  Like Scene.travel_field the call returns when the result stands: it waits on the
    stream between batches of rounds.  Stream handling as in write_region; the workspace comes from torch's pool."""
    return _settle(scene, labels, records, chosen, stream, False)[0]


def settle(scene, components, chosen=None, stream=None):
    """The pieces of `components` (Scene.components) named by `chosen` -- one value per record, non-zero = may fall; None means
    components.loose(), the pieces that touch no anchor face -- fall and land.  Returns a Settled whose `out` covers the components'
    box.  The floor is the bottom of that box: take it down to the ground, or pieces land in mid-air."""
    return settle_volume(scene, components.labels, components.records, components.loose() if chosen is None else chosen, stream)


def settle_times(scene, labels, records, chosen, stream=None, batch=0):
    """bm_debug_settle_times: settle_volume with a hipEvent between its stages and `batch` rounds between two looks of the host (0 = the
    default).  Returns (Settled, ([ms of the set-up, the rounds, the move], rounds, looks))."""
    return _settle(scene, labels, records, chosen, stream, True, batch)


def settle_floating(scene, lo, hi, anchor=ANCHOR):
    """Let the floating pieces of the box lo <= v < hi fall: components, the pieces that touch none of the anchor faces of the box are
    chosen, settle, write_region with replace.  Returns (pieces, voxels, largest_drop) that moved.  A piece that touches an anchor face
    does not move; the floor is the bottom of the box, so take lo.z down to the ground."""
    comps = scene.components(lo, hi)
    loose = comps.loose(anchor)
    if min(comps.labels.shape) == 0 or not loose.any():
        return 0, 0, 0
    done = settle(scene, comps, loose)
    if done.moved_voxels:
        scene.write_region(lo, done.out, op="replace")
    return done.moved_pieces, done.moved_voxels, done.largest_drop
