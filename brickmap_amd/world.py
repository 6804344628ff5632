"""The world of a scene: the host-only doors of the generator, edits, loads and regions, dense regions as volumes with strides
(`region_of`), connected components, and the Scene methods that change or read the live world (`_WorldMethods`)."""
import ctypes as C

import numpy as np

from . import _lib
from ._handoff import Handoff
from ._lib import BM_EDIT_BOX, BM_EDIT_CLEAR, BM_EDIT_SET, BM_EDIT_SPHERE, BM_REGION_REPLACE, BM_VOXELS_DEVICE, BM_VOXELS_HOST, COMPONENT_DTYPE, bm_edit, bm_region, check


def _read_all(fn, dtype, *head):
    """everything a reader of the library has to give, as a flat array: asked for its size first, then filled"""
    n = C.c_size_t(0)
    check(fn(*head, None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype)
    check(fn(*head, out.ctypes.data, out.size, C.byref(n)))
    return out


def host_cube_field(grid_size, grid_height):
    """The octant cube field of the generated world (bm_host_cube_field): uint8 [8, cells_height+2, cells+2, cells+2]."""
    out = _read_all(_lib.load().bm_host_cube_field, np.uint8, grid_size, grid_height)
    cx, cz = grid_size // 8 + 2, grid_height // 8 + 2
    return out.reshape(8, cz, cx, cx)


def host_column_heights(grid_size, grid_height, sx, sy):
    """Terrain heights of one supercell column from the product's CPU generator (no device needed)."""
    out = np.zeros((128, 128), np.float32)
    check(_lib.load().bm_host_column_heights(grid_size, grid_height, sx, sy, out.ctypes.data))
    return out


def _supercell_arrays(indices=None, bricks=()):
    """(indices uint32[4096], brick count, bricks uint32[4096, 16]) for a host door of one supercell: zeros, or copies of the caller's"""
    idx = np.zeros(4096, np.uint32) if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).copy()
    buf = np.zeros((4096, 16), np.uint32)
    buf[: len(bricks)] = np.asarray(bricks, np.uint32).reshape(-1, 16)
    return idx, C.c_uint32(len(bricks)), buf


def host_generate_supercell(grid_size, grid_height, sx, sy, sz):
    """(indices[4096], bricks[n,16]) of one supercell from the product's CPU generator (no device needed)."""
    idx, n, bricks = _supercell_arrays()
    check(_lib.load().bm_host_generate_supercell(grid_size, grid_height, sx, sy, sz, idx.ctypes.data, C.byref(n), bricks.ctypes.data, 4096))
    return idx, bricks[: n.value].copy()


def edit_box(op, lo, hi):
    """One box edit (bm_edit): voxels lo <= v < hi on every axis; op is BM_EDIT_SET or BM_EDIT_CLEAR (or "set" / "clear")."""
    e = bm_edit()
    e.op, e.shape = _edit_op(op), BM_EDIT_BOX
    e.lo[:] = [int(v) for v in lo]
    e.hi[:] = [int(v) for v in hi]
    return e


def edit_sphere(op, center, radius):
    """One sphere edit (bm_edit): voxels v with sum((v - center)^2) <= radius^2, in integers."""
    e = bm_edit()
    e.op, e.shape = _edit_op(op), BM_EDIT_SPHERE
    e.center[:] = [int(v) for v in center]
    e.radius = int(radius)
    return e


def _edit_op(op):
    return {"set": BM_EDIT_SET, "clear": BM_EDIT_CLEAR}.get(op, op) if isinstance(op, str) else int(op)


def _edit_array(edits):
    edits = list(edits)
    arr = (bm_edit * max(len(edits), 1))()
    for i, e in enumerate(edits):
        arr[i] = e
    return arr, len(edits)


def host_edit_supercell(grid_size, grid_height, sx, sy, sz, indices, bricks, edits):
    """bm_host_edit_supercell: the host half of an edit batch on one supercell's arrays (no device needed).  indices: uint32[4096],
    bricks: uint32[n, 16] as host_generate_supercell returns them; returns the edited (indices, bricks) -- new arrays."""
    idx, n, buf = _supercell_arrays(indices, bricks)
    arr, count = _edit_array(edits)
    check(_lib.load().bm_host_edit_supercell(grid_size, grid_height, sx, sy, sz, idx.ctypes.data, C.byref(n), buf.ctypes.data, 4096, count, arr))
    return idx, buf[: n.value].copy()


# ---- dense voxels (bm_scene_load_voxels): a volume [z, y, x] of one byte per voxel, non-zero = solid
def volume_dims(volume, grid_size=None, grid_height=None):
    """(grid_size, grid_height) of a dense voxel volume, after checking it: a numpy array or torch tensor of shape
    (grid_height, grid_size, grid_size) -- [z, y, x], x fastest --, dtype uint8 or bool, C-contiguous, both dimensions positive multiples
    of 128; with grid_size / grid_height given the shape must be exactly that.  Raises ValueError otherwise (no library call is made)."""
    shape = tuple(getattr(volume, "shape", ()))
    if len(shape) != 3 or shape[1] != shape[2] or shape[0] <= 0 or shape[1] <= 0 or shape[0] % 128 or shape[1] % 128:
        raise ValueError(f"volume: shape (grid_height, grid_size, grid_size) in positive multiples of 128 voxels expected, got {shape}")
    if grid_size is not None and shape != (grid_height, grid_size, grid_size):
        raise ValueError(f"volume: shape {(grid_height, grid_size, grid_size)} expected for this scene, got {shape}")
    if _is_torch_voxels("volume", volume):
        if not volume.is_contiguous():
            raise ValueError("volume: a contiguous tensor expected (x fastest)")
    elif not volume.flags["C_CONTIGUOUS"]:
        raise ValueError("volume: a C-contiguous array expected (x fastest)")
    return int(shape[1]), int(shape[0])


def _is_torch_voxels(name, volume):
    """True for a torch tensor, False for a numpy array, of one byte per voxel (uint8 or bool); raises ValueError for anything else"""
    if hasattr(volume, "is_contiguous"):
        import torch
        kinds = (torch.uint8, torch.bool)
    elif isinstance(volume, np.ndarray):
        kinds = (np.dtype(np.uint8), np.dtype(np.bool_))
    else:
        raise ValueError(f"{name}: a numpy array or torch tensor expected, got {type(volume).__name__}")
    if volume.dtype not in kinds:
        raise ValueError(f"{name}: dtype uint8 or bool expected, got {volume.dtype}")
    return not isinstance(volume, np.ndarray)


def host_load_supercell(volume, sx, sy, sz):
    """bm_host_load_supercell: (indices[4096], bricks[n, 16]) of one supercell of the canonical build of `volume` (a numpy volume as
    volume_dims describes it; no device needed)."""
    gs, gh = volume_dims(volume)
    idx, n, bricks = _supercell_arrays()
    check(_lib.load().bm_host_load_supercell(gs, gh, sx, sy, sz, volume.ctypes.data, idx.ctypes.data, bricks.ctypes.data, C.byref(n)))
    return idx, bricks[: n.value].copy()


# ---- dense regions (bm_scene_write_region / bm_scene_read_region): a box of voxels as a volume [z, y, x] with strides
def _region_op(op):
    return {"replace": BM_REGION_REPLACE, "set": BM_EDIT_SET, "clear": BM_EDIT_CLEAR}.get(op, op) if isinstance(op, str) else int(op)


def region_of(lo, volume, name="volume"):
    """(bm_region, data pointer, is_cuda) of `volume` placed with its voxel [0, 0, 0] at world voxel lo = (x, y, z): a numpy array or a
    torch tensor [z, y, x], uint8 or bool, x contiguous (stride 1) and non-negative strides along y and z -- a slice of a larger array
    works.  Raises ValueError otherwise (no library call is made)."""
    shape = tuple(getattr(volume, "shape", ()))
    if len(shape) != 3:
        raise ValueError(f"{name}: three dimensions [z, y, x] expected, got shape {shape}")
    if _is_torch_voxels(name, volume):
        strides, ptr, cuda = tuple(volume.stride()), volume.data_ptr(), volume.is_cuda
    else:
        strides, ptr, cuda = volume.strides, volume.ctypes.data, False
    nz, ny, nx = shape
    if min(shape) == 0:  # an empty box: no voxel, no layout
        strides = (ny * nx, nx, 1)
    if nx > 1 and strides[2] != 1:
        raise ValueError(f"{name}: x must be contiguous (stride 1), got strides {strides}")
    row = strides[1] if ny > 1 else nx
    sl = strides[0] if nz > 1 else row * ny
    if row < nx or sl < row * ny:
        raise ValueError(f"{name}: rows and slices must not overlap or run backwards, got strides {strides} for shape {shape}")
    r = bm_region()
    r.lo[:] = [int(v) for v in lo]
    r.hi[:] = [int(lo[0]) + nx, int(lo[1]) + ny, int(lo[2]) + nz]
    r.row_pitch, r.slice_pitch = int(row), int(sl)
    return r, ptr, cuda


def host_write_region_supercell(grid_size, grid_height, sx, sy, sz, indices, bricks, lo, volume, op="replace"):
    """bm_host_write_region_supercell: the host half of Scene.write_region on one supercell's arrays (no device needed; the arrays as
    for host_edit_supercell).  Returns the new (indices, bricks)."""
    r, ptr, cuda = region_of(lo, volume)
    assert not cuda
    idx, n, buf = _supercell_arrays(indices, bricks)
    check(_lib.load().bm_host_write_region_supercell(grid_size, grid_height, sx, sy, sz, idx.ctypes.data, C.byref(n), buf.ctypes.data, 4096, C.byref(r), _region_op(op),
                                                     C.c_void_p(ptr)))
    return idx, buf[: n.value].copy()


# ---- connected components (bm_scene_label_region / bm_scene_label_components / bm_scene_label_mask)
FACE_BITS = {"-x": 1, "+x": 2, "-y": 4, "+y": 8, "-z": 16, "+z": 32}


def _box3(lo, hi, who):
    lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError(f"{who}: lo and hi are (x, y, z)")
    lim = np.iinfo(np.int32)
    if any(not lim.min <= v <= lim.max for v in lo + hi):
        raise ValueError(f"{who}: coordinates must fit 32 bits")
    return (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), tuple(h - l for l, h in zip(lo, hi))[::-1]


def host_label_volume(volume):
    """bm_host_label_volume (host only, no device): connected components by faces of a dense volume [z, y, x] (non-zero = solid) in plain
    loops.  Returns (labels, count): int32 [z, y, x] with 0 for empty voxels and 1 + index of the component's first voxel for solid
    ones, and the number of components."""
    volume = np.asarray(volume)
    if volume.ndim != 3 or volume.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)):
        raise ValueError(f"host_label_volume: a uint8 or bool array [z, y, x] expected, got {volume.dtype} of shape {volume.shape}")
    volume = np.ascontiguousarray(volume)
    nz, ny, nx = volume.shape
    labels = np.zeros(volume.shape, np.int32)
    count = C.c_uint64(0)
    check(_lib.load().bm_host_label_volume(volume.ctypes.data, nx, ny, nz, labels.ctypes.data, C.byref(count)))
    return labels, int(count.value)


class Components:
    """Result of Scene.components: `labels` (int32 CUDA tensor [z, y, x]), `records` (numpy array of COMPONENT_DTYPE, ascending label),
    and masks of chosen components as uint8 CUDA tensors [z, y, x] that write_region / read_region take as they are."""

    def __init__(self, scene, lo, hi, labels, records, table):
        self.scene, self.lo, self.hi, self.labels, self.records, self._table = scene, tuple(lo), tuple(hi), labels, records, table

    def __len__(self):
        return len(self.records)

    def mask(self, chosen, stream=None):
        """uint8 mask of the voxels whose component's entry in `chosen` (one value per record, non-zero = chosen) is set: that value."""
        import torch
        chosen = np.ascontiguousarray(np.asarray(chosen)).astype(np.uint8).reshape(-1)
        if len(chosen) != len(self.records):
            raise ValueError(f"mask: one value per record expected ({len(self.records)}), got {len(chosen)}")
        dev = self.labels.device
        mask = torch.empty(tuple(self.labels.shape), dtype=torch.uint8, device=dev)
        if mask.numel() == 0:
            return mask
        d_chosen = torch.from_numpy(chosen).to(dev) if len(chosen) else torch.zeros(1, dtype=torch.uint8, device=dev)
        self.scene.label_mask_raw(self.lo, self.hi, self.labels.data_ptr(), self._table.data_ptr() if len(chosen) else 0, len(chosen), d_chosen.data_ptr() if len(chosen) else 0,
                                  mask.data_ptr(), stream)
        return mask

    def floating(self, anchor=("-x", "+x", "-y", "+y", "-z"), stream=None):
        """uint8 mask (1) of the voxels whose component touches none of the anchor faces of (box and world)"""
        return self.mask(self.loose(anchor), stream)

    def loose(self, anchor=("-x", "+x", "-y", "+y", "-z")):
        """per record: the component touches none of the anchor faces"""
        bits = 0
        for a in anchor:
            if a not in FACE_BITS:
                raise ValueError(f"anchor faces are {tuple(FACE_BITS)}, got {a!r}")
            bits |= FACE_BITS[a]
        return (self.records["faces"] & bits) == 0


class _WorldMethods:
    """Scene's methods on its world: loads, edits, the walk-field readers, dense regions and connected components."""

    # ---- a scene from the caller's voxels (bm_scene_load_voxels)
    def load_voxels(self, volume, stream=None):
        """Make `volume` the scene's world (replacing the one it holds, if any): a numpy array or a torch tensor, [z, y, x] of shape
        (grid_height, grid_size, grid_size), uint8 or bool, contiguous.  Host memory is built on CPU threads and uploaded; a tensor on
        the scene's GPU is packed on the GPU without leaving it, behind the work queued on `stream` (a raw HIP stream handle; None =
        torch's current stream, which the given stream is made to wait for).  The scene is preloaded when the call returns.  A wrong
        shape, dtype or layout raises ValueError before the library is called."""
        volume_dims(volume, self.grid_size, self.grid_height)
        if hasattr(volume, "is_contiguous"):
            if volume.is_cuda:
                if volume.device.index != self.device:
                    raise ValueError(f"volume: a tensor on cuda:{self.device} (the scene's GPU) or on the CPU expected, got {volume.device}")
                check(self._L.bm_scene_load_voxels(self.gpuScene, C.c_void_p(volume.data_ptr()), volume.numel(), BM_VOXELS_DEVICE, C.c_void_p(Handoff(volume, stream).handle)))
                return self
            volume = volume.numpy()
        check(self._L.bm_scene_load_voxels(self.gpuScene, C.c_void_p(volume.ctypes.data), volume.size, BM_VOXELS_HOST, None))
        return self

    @classmethod
    def from_voxels(cls, volume, device=0):
        """A scene whose world is `volume` (see load_voxels); the dimensions come from its shape (grid_height, grid_size, grid_size)."""
        grid_size, grid_height = volume_dims(volume)
        return cls(grid_size, grid_height, device=device).load_voxels(volume)

    def voxels(self):
        """bm_scene_host_voxels: the host world as a bool volume [z, y, x]."""
        out = np.zeros((self.grid_height, self.grid_size, self.grid_size), np.uint8)
        n = C.c_size_t(0)
        check(self._L.bm_scene_host_voxels(self.gpuScene, out.ctypes.data, out.size, C.byref(n)))
        return out.view(np.bool_)

    def last_load_ms(self):
        """(pack_ms, field_ms, mirror_ms) of the last load from a device tensor (hipEvents on the load stream)."""
        return self._last_ms(self._L.bm_scene_last_load_ms, 3)

    def _last_ms(self, fn, n):
        t = [C.c_float(0) for _ in range(n)]
        check(fn(self.gpuScene, *[C.byref(v) for v in t]))
        return tuple(float(v.value) for v in t)

    # ---- voxel edits (bm_scene_edit): ordered behind the frames in flight, seen by every frame issued after the call
    def edit(self, edits, stream=None):
        """Apply a list of edits (edit_box / edit_sphere) in order.  A malformed edit raises and leaves the scene unchanged."""
        arr, count = _edit_array(edits)
        check(self._L.bm_scene_edit(self.gpuScene, count, arr, self._stream(stream)))
        return self

    def fill_box(self, lo, hi, stream=None):
        return self.edit([edit_box(BM_EDIT_SET, lo, hi)], stream)

    def clear_box(self, lo, hi, stream=None):
        return self.edit([edit_box(BM_EDIT_CLEAR, lo, hi)], stream)

    def fill_sphere(self, center, radius, stream=None):
        return self.edit([edit_sphere(BM_EDIT_SET, center, radius)], stream)

    def carve_sphere(self, center, radius, stream=None):
        return self.edit([edit_sphere(BM_EDIT_CLEAR, center, radius)], stream)

    def set_voxels(self, coords, values, stream=None):
        """coords: N x 3 int32 voxel coordinates (numpy array or CPU torch tensor); values: a scalar or N values (non-zero = solid)."""
        if hasattr(coords, "detach"):
            coords = coords.detach().cpu().numpy()
        xyz = np.ascontiguousarray(np.asarray(coords).reshape(-1, 3), dtype=np.int32)
        if hasattr(values, "detach"):
            values = values.detach().cpu().numpy()
        v = np.asarray(values)
        v = np.full(len(xyz), 1 if v.item() else 0, np.uint8) if v.ndim == 0 else np.ascontiguousarray(v != 0, dtype=np.uint8)
        assert len(v) == len(xyz), "values: a scalar or one per voxel"
        check(self._L.bm_scene_set_voxels(self.gpuScene, len(xyz), xyz.ctypes.data, v.ctypes.data, self._stream(stream)))
        return self

    def _cube_field(self, fn):
        out = _read_all(fn, np.uint8, self.gpuScene)
        cx, cz = self.grid_size // 8 + 2, self.grid_height // 8 + 2
        return out.reshape(8, cz, cx, cx)

    def device_cube_field(self):
        """bm_scene_device_cube_field: the device's octant cube field, uint8 [8, cells_height+2, cells+2, cells+2]."""
        return self._cube_field(self._L.bm_scene_device_cube_field)

    def host_cube_field(self):
        """bm_scene_host_cube_field: the cube field of the scene's current host world (same layout)."""
        return self._cube_field(self._L.bm_scene_host_cube_field)

    def sun_plane(self):
        """bm_scene_sun_plane: (plane, plan) -- the sun plane as last built, uint8 [cells_z + 2, cells + 2, cells + 2] with its border, or None
        when none has been built; and the plan it was built for as a dict (valid, octant, dom, m1, m2, lo1, hi1, lo2, hi2, clear, rise, bins)."""
        n = C.c_size_t(0)
        plan = (C.c_int32 * 12)()
        check(self._L.bm_scene_sun_plane(self.gpuScene, None, 0, C.byref(n), plan))
        names = ("valid", "octant", "dom", "m1", "m2", "lo1", "hi1", "lo2", "hi2", "clear", "rise", "bins")
        plan = dict(zip(names, (int(v) for v in plan)))
        if n.value == 0:
            return None, plan
        out = np.zeros(n.value, np.uint8)
        check(self._L.bm_scene_sun_plane(self.gpuScene, out.ctypes.data, out.size, C.byref(n), None))
        c = self.grid_size // 8 + 2
        return out.reshape(-1, c, c), plan

    def shadow_heights(self):
        """bm_scene_shadow_heights: (entries, plan, bytes) -- the table of shadow heights as last built, uint32 [cells, cells] (y, x): 0 = no
        dark cell, otherwise the sun plane's byte offset of the column's first slice that is not dark; None when nothing has been built.  plan:
        dict (valid, rise, rise_hi, unit); bytes: device memory of the slice and the build's scratch."""
        n, nbytes = C.c_size_t(0), C.c_uint64(0)
        plan = (C.c_int32 * 4)()
        check(self._L.bm_scene_shadow_heights(self.gpuScene, None, 0, C.byref(n), C.byref(nbytes), plan))
        plan = dict(zip(("valid", "rise", "rise_hi", "unit"), (int(v) for v in plan)))
        if n.value == 0:
            return None, plan, int(nbytes.value)
        out = np.zeros(n.value, np.uint32)
        check(self._L.bm_scene_shadow_heights(self.gpuScene, out.ctypes.data, out.size, C.byref(n), None, None))
        c = self.grid_size // 8
        return out.reshape(c, c), plan, int(nbytes.value)

    def sun_plane_stats(self):
        """bm_scene_sun_plane_stats: (builds so far, device ms of the last build)."""
        builds, ms = C.c_uint64(0), C.c_float(0)
        check(self._L.bm_scene_sun_plane_stats(self.gpuScene, C.byref(builds), C.byref(ms)))
        return int(builds.value), float(ms.value)

    def view_plane(self):
        """bm_scene_view_plane: (plane, origin) -- the view plane as last built, uint8 [cells_z + 2, cells + 2, cells + 2] with its border, and
        the origin it was built for as float32 [3]; (None, None) while no plane stands."""
        n = C.c_size_t(0)
        origin = np.zeros(3, np.float32)
        check(self._L.bm_scene_view_plane(self.gpuScene, None, 0, C.byref(n), origin.ctypes.data))
        if n.value == 0:
            return None, None
        out = np.zeros(n.value, np.uint8)
        check(self._L.bm_scene_view_plane(self.gpuScene, out.ctypes.data, out.size, C.byref(n), None))
        c = self.grid_size // 8 + 2
        return out.reshape(-1, c, c), origin

    def view_plane_stats(self):
        """bm_scene_view_plane_stats: (builds so far, device ms of the last build)."""
        builds, ms = C.c_uint64(0), C.c_float(0)
        check(self._L.bm_scene_view_plane_stats(self.gpuScene, C.byref(builds), C.byref(ms)))
        return int(builds.value), float(ms.value)

    def escape_table(self):
        """bm_scene_escape_table: the device's escape heights as thresholds, int32 [8, cells, cells] (octant, y, x)."""
        out = _read_all(self._L.bm_scene_escape_table, np.int32, self.gpuScene)
        c = self.grid_size // 8
        return out.reshape(8, c, c)

    def last_edit_ms(self):
        """(scatter_ms, field_ms) of the last edit batch that changed the scene (hipEvents on the load stream)."""
        return self._last_ms(self._L.bm_scene_last_edit_ms, 2)

    # ---- dense regions (bm_scene_write_region / bm_scene_read_region)
    def write_region(self, lo, volume, op="replace", stream=None):
        """Write a dense box of voxels into the live scene: `volume` ([z, y, x], uint8 or bool, numpy array or torch tensor; a slice of a
        larger one works as long as x is contiguous) lands with its first voxel at world voxel lo = (x, y, z).  op: "replace" (the box's
        voxels become the volume's), "set" (solid where the volume is non-zero) or "clear" (empty where it is non-zero).  Clipped to the
        world.  A tensor on the scene's GPU is packed there, behind the work queued on `stream` (a raw HIP stream handle; None = torch's
        current stream).  Ordered like an edit.  A wrong dtype, layout or device raises ValueError before the library is called."""
        r, ptr, cuda = region_of(lo, volume)
        if min(volume.shape) == 0:
            return self
        where, handle = (BM_VOXELS_DEVICE, C.c_void_p(self._handoff(volume, stream).handle)) if cuda else (BM_VOXELS_HOST, self._stream(stream))
        check(self._L.bm_scene_write_region(self.gpuScene, C.byref(r), _region_op(op), C.c_void_p(ptr), where, handle))
        return self

    def read_region(self, lo, hi, out=None, device=False, stream=None):
        """The voxels lo <= v < hi (x, y, z; clipped to the world, 0 outside it) as a volume [z, y, x]: a bool numpy array, or with
        device=True a uint8 torch tensor on the scene's GPU, written there by a kernel issued like a query on `stream`.  With `out` (numpy
        array or torch tensor of that shape, strides honoured as in write_region) the voxels are written into it and it is returned."""
        shape = tuple(int(h) - int(l) for l, h in zip(lo, hi))[::-1]
        if min(shape) < 0:
            raise ValueError(f"read_region: hi < lo ({lo} ... {hi})")
        result = out
        if out is None:
            if device:
                import torch
                out = result = torch.empty(shape, dtype=torch.uint8, device=f"cuda:{self.device}")
            else:
                out = np.zeros(shape, np.uint8)
                result = out.view(np.bool_)
        elif tuple(out.shape) != shape:
            raise ValueError(f"read_region: out of shape {shape} expected, got {tuple(out.shape)}")
        r, ptr, cuda = region_of(lo, out, "out")
        if min(shape) == 0:
            return result
        if cuda:
            h = self._handoff(out, stream)
            check(self._L.bm_scene_read_region(self.gpuScene, C.byref(r), C.c_void_p(ptr), BM_VOXELS_DEVICE, C.c_void_p(h.handle)))
            h.join()
        else:
            check(self._L.bm_scene_read_region(self.gpuScene, C.byref(r), C.c_void_p(ptr), BM_VOXELS_HOST, None))
        return result

    def last_region_ms(self):
        """(pack_ms, copy_ms, scatter_ms, field_ms) of the last write_region that reached the device (hipEvents on the load stream)."""
        return self._last_ms(self._L.bm_scene_last_region_ms, 4)

    # ---- connected components (bm_scene_label_region ...): label_region is issued like a query, asynchronous to the host
    def label_region_raw(self, lo, hi, labels_ptr, count_ptr, flags=0, stream=None):
        """bm_scene_label_region on device pointers (ints)"""
        clo, chi, _ = _box3(lo, hi, "label_region")
        check(self._L.bm_scene_label_region(self.gpuScene, C.byref(clo), C.byref(chi), int(flags), C.c_void_p(labels_ptr), C.c_void_p(count_ptr), self._stream(stream)))

    def label_components_raw(self, lo, hi, labels_ptr, comps_ptr, capacity, stream=None):
        clo, chi, _ = _box3(lo, hi, "label_components")
        check(self._L.bm_scene_label_components(self.gpuScene, C.byref(clo), C.byref(chi), C.c_void_p(labels_ptr), C.c_void_p(comps_ptr), int(capacity), self._stream(stream)))

    def label_mask_raw(self, lo, hi, labels_ptr, comps_ptr, n, chosen_ptr, mask_ptr, stream=None):
        clo, chi, _ = _box3(lo, hi, "label_mask")
        check(self._L.bm_scene_label_mask(self.gpuScene, C.byref(clo), C.byref(chi), C.c_void_p(labels_ptr), C.c_void_p(comps_ptr), int(n), C.c_void_p(chosen_ptr),
                                          C.c_void_p(mask_ptr), self._stream(stream)))

    def label_region(self, lo, hi, out=None, stream=None):
        """Connected components (by faces) of the voxels lo <= v < hi (x, y, z; voxels outside the world are empty): (labels, count).
        labels: an int32 tensor [z, y, x] on the scene's GPU, 0 for an empty voxel, else 1 + the index ((z * ny + y) * nx + x in the box)
        of the first voxel of its component -- or `out`, a contiguous int32 CUDA tensor of that shape.  count: a one-element int64 tensor on
        the GPU; reading it is the caller's synchronisation.  Issued like a query on `stream` (a raw HIP stream handle; None = torch's
        current stream).  A wrong dtype, layout or device raises ValueError before the library is called."""
        import torch
        _, _, shape = _box3(lo, hi, "label_region")
        if min(shape) < 0:
            raise ValueError(f"label_region: hi < lo ({lo} ... {hi})")
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=f"cuda:{self.device}")
        elif not hasattr(out, "is_contiguous"):
            raise ValueError(f"label_region: out must be a torch tensor on the scene's GPU, got {type(out).__name__}")
        elif out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
            raise ValueError(f"label_region: out must be a contiguous int32 CUDA tensor of shape {shape}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        h = self._handoff(out, stream)
        with h.on_target():
            count = torch.zeros(1, dtype=torch.int64, device=out.device)
        self.label_region_raw(lo, hi, out.data_ptr(), count.data_ptr(), 0, h.handle)
        h.join()
        return out, count

    def last_label_ms(self):
        """(local_ms, merge_ms, flatten_ms) of the last label_region that launched its kernels (hipEvents on its stream)."""
        return self._last_ms(self._L.bm_scene_last_label_ms, 3)

    def components(self, lo, hi, stream=None):
        """label_region, then the table of every component (waits for the count): a Components."""
        import torch
        labels, count = self.label_region(lo, hi, stream=stream)
        n = int(count.item())
        table = torch.zeros((max(n, 1), COMPONENT_DTYPE.itemsize // 8), dtype=torch.int64, device=labels.device)
        if n:
            h = self._handoff(labels, stream)
            self.label_components_raw(lo, hi, labels.data_ptr(), table.data_ptr(), n, h.handle)
            h.target.synchronize()
        records = table[:n].cpu().numpy().view(COMPONENT_DTYPE).reshape(-1)
        return Components(self, lo, hi, labels, records, table)

    def remove_floating(self, lo, hi, anchor=("-x", "+x", "-y", "+y", "-z")):
        """Clear every voxel of the box whose component (inside the box) touches none of the anchor faces: (pieces, voxels) removed."""
        comps = self.components(lo, hi)
        loose = comps.loose(anchor)
        pieces, voxels = int(np.count_nonzero(loose)), int(comps.records["voxels"][loose].sum())
        if voxels:
            self.write_region(lo, comps.floating(anchor), op="clear")
        return pieces, voxels
