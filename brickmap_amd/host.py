"""Host-side mirror of the reference's Scene / Camera / State / launch_kernels interface.

Same names, argument meaning and call order as the reference's C++ (file:line into
the reference checkout, src/): `Scene` (Scene.h:7-44), `Camera` (camera.h:3-24), `State` (state.h:5-34),
`launch_kernels` (launch.h:6, kernel.cu:366-439).  Everything below the method bodies is the
C-ABI of libbrickmap_hip.so; torch only provides device tensors and streams.
"""
import ctypes as C
import math
import os
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from ._lib import (BM_EDIT_BOX, BM_EDIT_CLEAR, BM_EDIT_SET, BM_EDIT_SPHERE, BM_REGION_REPLACE, bm_region, BM_QUERY_LOD, BM_QUERY_NO_REQUESTS, BM_VOLUME_ANY, BM_VOXELS_DEVICE, BM_VOXELS_HOST, bm_camera, bm_counters, bm_edit, bm_frame_params,
                   bm_scene_info, check)


# The reference's fly-through presets (performance_measure.h:4-25): camera position + (horizontal, vertical) angle.
# It lists 9 positions but only 8 angle pairs and indexes both with the same counter (performance_measure.cpp:32-34).
# World: the reference's native 4096 x 4096 x 512 voxels.
FLYTHROUGH_VIEWS = (
    ((512.0, 512.0, 300.0), (-61863.5, -0.501796)),
    ((840.254, 832.446, 1169.88), (-61864.4, -0.429796)),
    ((2227.83, 774.886, 204.955), (-61863.9, 0.0622036)),
    ((3326.19, 2055.72, 44.7995), (-61864.2, -0.981796)),
    ((7134.6, 1262.44, 5531.79), (-61865.2, -0.501796)),
    ((11298.6, 3113.03, 598.019), (-61866.3, -0.141796)),
    ((10921.4, 4774.14, 267.808), (-61859.4, 0.0142036)),
    ((9961.29, 4508.12, 189.59), (-61857.2, -0.261796)),
    # the 9th position has no angle pair of its own: the reference reads test_angles[8] past the end of the vector
    # (performance_measure.cpp:33-34, undefined behaviour); here it is flown with the last defined pair
    ((10835.3, 4160.83, 359.992), (-61857.2, -0.261796)),
)


def flythrough_camera(i):
    """Camera of the reference's i-th fly-through viewpoint."""
    pos, (h, v) = FLYTHROUGH_VIEWS[i % len(FLYTHROUGH_VIEWS)]
    return Camera(position=pos, horizontal_angle=h, vertical_angle=v).update()


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _normalize_f32(v):
    """glm::normalize in fp32: v * (1 / sqrt((x*x + y*y) + z*z))."""
    v = _f32(v)
    d = np.float32(np.float32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return v * (np.float32(1.0) / np.sqrt(d, dtype=np.float32))


@dataclass
class Camera:
    """camera.h:3-24.  `handle_input` (GLFW keys/mouse) is out of scope: there is no window."""
    position: tuple = (512.0, 512.0, 300.0)
    direction: tuple = (1.0, 0.0, 0.0)
    up: tuple = (0.0, 0.0, 1.0)
    focalDistance: float = 1.0
    lensRadius: float = 0.0
    horizontal_angle: float = 0.0
    vertical_angle: float = 0.0

    def update(self):
        """Camera::update (camera.cpp:48-54): direction from the two angles, then normalised."""
        h, v = self.horizontal_angle, self.vertical_angle
        d = _f32([math.cos(v) * math.sin(h), math.cos(v) * math.cos(h), math.sin(v)])
        self.direction = tuple(float(x) for x in _normalize_f32(d))
        return self

    def to_c(self):
        c = bm_camera()
        c.position[:] = [float(x) for x in self.position]
        c.direction[:] = [float(x) for x in self.direction]
        c.up[:] = [float(x) for x in self.up]
        c.focal_distance = float(self.focalDistance)
        c.lens_radius = float(self.lensRadius)
        return c


@dataclass
class FrameParams:
    """Per-launch parameters the reference keeps as constexprs / statics (kernel.cu:13,369; variables.cpp:3)."""
    width: int
    height: int
    spp: int = 1
    sample_base: int = 0
    max_bounces: int = 3
    base_frame: int = 1
    flags: int = 0
    band_rows: int = 0  # 0 = whole image in one band
    shard_rank: int = 0
    shard_count: int = 1
    sun_position: tuple = (0.05, 0.1)

    def to_c(self):
        p = bm_frame_params()
        p.width, p.height, p.spp, p.sample_base = self.width, self.height, self.spp, self.sample_base
        p.max_bounces, p.base_frame, p.flags = self.max_bounces, self.base_frame, self.flags
        p.band_rows = self.band_rows if self.band_rows > 0 else self.height
        p.shard_rank, p.shard_count = self.shard_rank, self.shard_count
        p.sun_position[:] = [float(self.sun_position[0]), float(self.sun_position[1])]
        return p


def local_rows(params: FrameParams) -> int:
    """Rows of the frame owned by this shard (bm_local_rows)."""
    p = params.to_c()
    return int(_lib.load().bm_local_rows(C.byref(p)))


def frame_plan(params: FrameParams, hit_records=False):
    """bm_frame_plan_of: what the library decides for a frame with these parameters (host only): flags after its own choice of work
    items, ordered / helpers / sample_items / xcd_handout / refill_min / instrumented, tiles and local rows."""
    plan = _lib.bm_frame_plan()
    par_c = params.to_c()
    check(_lib.load().bm_frame_plan_of(C.byref(par_c), 1 if hit_records else 0, C.byref(plan)))
    return {name: int(getattr(plan, name)) for name, _ in _lib.bm_frame_plan._fields_}


def launch_plan(cameras, params, accum_ptrs, debug_ptrs=None, grid_size=256, grid_height=256):
    """bm_launch_plan_of: what the library decides for a bm_render_frames launch of `len(params)` frames (host only, no scene): the ring
    mode (0 one frame, 1 frame ring, 2 uniform frame ring), the frame group and strides of a uniform launch, shared_digest, instrumented,
    counter_blocks, refill_min and the workgroups before the residency cap.  cameras: one Camera or one per frame; accum_ptrs: one
    address or one per frame; debug_ptrs: None or one entry per frame (None or an address).  The addresses are integers -- a tensor's
    data_ptr() -- and are only compared, never read.  Raises what Scene.render_frames would raise on a world of that size."""
    n = len(params)
    cams = list(cameras) if isinstance(cameras, (list, tuple)) else [cameras] * n
    accs = list(accum_ptrs) if isinstance(accum_ptrs, (list, tuple)) else [accum_ptrs] * n
    assert len(cams) == n and len(accs) == n and (debug_ptrs is None or len(debug_ptrs) == n)
    cam_c = (_lib.bm_camera * n)(*[c.to_c() for c in cams])
    par_c = (_lib.bm_frame_params * n)(*[p.to_c() for p in params])
    acc_p = (C.c_void_p * n)(*accs)
    dbg_p = (C.c_void_p * n)(*debug_ptrs) if debug_ptrs is not None else None
    plan = _lib.bm_launch_plan()
    check(_lib.load().bm_launch_plan_of(n, cam_c, par_c, acc_p, dbg_p, grid_size, grid_height, C.byref(plan)))
    return {name: int(getattr(plan, name)) for name, _ in _lib.bm_launch_plan._fields_}


def trace_waves_per_simd(instrumented=False, xcd_handout=False, helpers=True, device=0):
    """bm_trace_waves_per_simd: resident waves per SIMD of the trace_paths instantiation on `device`."""
    n = C.c_int(0)
    check(_lib.load().bm_trace_waves_per_simd(device, int(bool(instrumented)), int(bool(xcd_handout)), int(bool(helpers)), C.byref(n)))
    return int(n.value)


def tuning_overrides():
    """bm_tuning_overrides: {name: value} of the BM_* tuning variables this process runs under ({} = the product's own rules)."""
    buf = C.create_string_buffer(512)
    check(_lib.load().bm_tuning_overrides(buf, 512))
    return {k: int(v) for k, v in (item.split("=") for item in buf.value.decode().split())}


def host_cube_field(grid_size, grid_height):
    """The octant cube field of the generated world (bm_host_cube_field): uint8 [8, cells_height+2, cells+2, cells+2]."""
    L = _lib.load()
    n = C.c_size_t(0)
    check(L.bm_host_cube_field(grid_size, grid_height, None, 0, C.byref(n)))
    out = np.zeros(n.value, np.uint8)
    check(L.bm_host_cube_field(grid_size, grid_height, out.ctypes.data, out.size, C.byref(n)))
    cx, cz = grid_size // 8 + 2, grid_height // 8 + 2
    return out.reshape(8, cz, cx, cx)


def host_column_heights(grid_size, grid_height, sx, sy):
    """Terrain heights of one supercell column from the product's CPU generator (no device needed)."""
    out = np.zeros((128, 128), np.float32)
    check(_lib.load().bm_host_column_heights(grid_size, grid_height, sx, sy, out.ctypes.data))
    return out


def host_generate_supercell(grid_size, grid_height, sx, sy, sz):
    """(indices[4096], bricks[n,16]) of one supercell from the product's CPU generator (no device needed)."""
    L = _lib.load()
    idx = np.zeros(4096, np.uint32)
    n = C.c_uint32(0)
    bricks = np.zeros((4096, 16), np.uint32)
    check(L.bm_host_generate_supercell(grid_size, grid_height, sx, sy, sz, idx.ctypes.data, C.byref(n), bricks.ctypes.data, 4096))
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
    idx = np.ascontiguousarray(indices, dtype=np.uint32).copy()
    n = C.c_uint32(len(bricks))
    buf = np.zeros((4096, 16), np.uint32)
    buf[: len(bricks)] = np.asarray(bricks, np.uint32).reshape(-1, 16)
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
    if hasattr(volume, "is_contiguous"):  # torch
        import torch
        if volume.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"volume: dtype uint8 or bool expected, got {volume.dtype}")
        if not volume.is_contiguous():
            raise ValueError("volume: a contiguous tensor expected (x fastest)")
    else:
        if not isinstance(volume, np.ndarray):
            raise ValueError(f"volume: a numpy array or torch tensor expected, got {type(volume).__name__}")
        if volume.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)):
            raise ValueError(f"volume: dtype uint8 or bool expected, got {volume.dtype}")
        if not volume.flags["C_CONTIGUOUS"]:
            raise ValueError("volume: a C-contiguous array expected (x fastest)")
    return int(shape[1]), int(shape[0])


def host_load_supercell(volume, sx, sy, sz):
    """bm_host_load_supercell: (indices[4096], bricks[n, 16]) of one supercell of the canonical build of `volume` (a numpy volume as
    volume_dims describes it; no device needed)."""
    gs, gh = volume_dims(volume)
    idx = np.zeros(4096, np.uint32)
    bricks = np.zeros((4096, 16), np.uint32)
    n = C.c_uint32(0)
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
    if hasattr(volume, "is_contiguous"):  # torch
        import torch
        if volume.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{name}: dtype uint8 or bool expected, got {volume.dtype}")
        strides, ptr, cuda = tuple(volume.stride()), volume.data_ptr(), volume.is_cuda
    elif isinstance(volume, np.ndarray):
        if volume.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)):
            raise ValueError(f"{name}: dtype uint8 or bool expected, got {volume.dtype}")
        strides, ptr, cuda = volume.strides, volume.ctypes.data, False
    else:
        raise ValueError(f"{name}: a numpy array or torch tensor expected, got {type(volume).__name__}")
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
    idx = np.ascontiguousarray(indices, dtype=np.uint32).copy()
    n = C.c_uint32(len(bricks))
    buf = np.zeros((4096, 16), np.uint32)
    buf[: len(bricks)] = np.asarray(bricks, np.uint32).reshape(-1, 16)
    check(_lib.load().bm_host_write_region_supercell(grid_size, grid_height, sx, sy, sz, idx.ctypes.data, C.byref(n), buf.ctypes.data, 4096, C.byref(r), _region_op(op),
                                                     C.c_void_p(ptr)))
    return idx, buf[: n.value].copy()


# ---- connected components (bm_scene_label_region / bm_scene_label_components / bm_scene_label_mask)
COMPONENT_DTYPE = np.dtype([("label", "<i4"), ("faces", "<u4"), ("voxels", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)])  # bm_component, 40 bytes
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


# ---- meshes -> voxels (bm_voxelize / bm_host_voxelize)
VOXELIZE_RESULT_DTYPE = np.dtype([("rejected", "<u4"), ("degenerate", "<u4"), ("open_columns", "<u8")])  # bm_voxelize_result, 16 bytes
_VOXELIZE_MODES = {"surface": _lib.BM_VOXELIZE_SURFACE, "solid": _lib.BM_VOXELIZE_SOLID,
                   "solid+surface": _lib.BM_VOXELIZE_SURFACE | _lib.BM_VOXELIZE_SOLID, "surface+solid": _lib.BM_VOXELIZE_SURFACE | _lib.BM_VOXELIZE_SOLID}


def _voxelize_mode(mode):
    if isinstance(mode, str):
        if mode not in _VOXELIZE_MODES:
            raise ValueError(f"voxelize: mode 'surface', 'solid' or 'solid+surface' expected, got {mode!r}")
        return _VOXELIZE_MODES[mode]
    return int(mode)


def _voxelize_params(lo, volume, mode, keep, name="out"):
    """(bm_voxelize_params, data pointer, is_cuda) of `volume` ([z, y, x], laid out as region_of takes it) with its voxel [0, 0, 0] at lo"""
    r, ptr, cuda = region_of(lo, volume, name)
    nz, ny, nx = volume.shape
    par = _lib.bm_voxelize_params()
    par.lo[:] = list(r.lo)
    par.extent[:] = [nx, ny, nz]
    par.row_pitch, par.slice_pitch = r.row_pitch, r.slice_pitch
    par.mode = _voxelize_mode(mode)
    par.flags = _lib.BM_VOXELIZE_KEEP if keep else 0
    return par, ptr, cuda


def voxelize_workspace_bytes(shape, n, mode="solid+surface"):
    """bm_voxelize_workspace_bytes: device memory bm_voxelize needs beside its buffers for a volume of shape (nz, ny, nx) and n triangles."""
    par = _lib.bm_voxelize_params()
    par.extent[:] = [int(shape[2]), int(shape[1]), int(shape[0])]
    par.mode = _voxelize_mode(mode)
    out = C.c_size_t(0)
    check(_lib.load().bm_voxelize_workspace_bytes(C.byref(par), int(n), C.byref(out)))
    return int(out.value)


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
    rec = np.zeros((), VOXELIZE_RESULT_DTYPE)
    rec["rejected"], rec["degenerate"], rec["open_columns"] = res.rejected, res.degenerate, res.open_columns
    return out, rec


class VoxelizeResult:
    """The bm_voxelize_result of a Scene.voxelize, read lazily: `packed` is the record on the device (two int64 words); rejected,
    degenerate, open_columns and record (a VOXELIZE_RESULT_DTYPE scalar) copy it to the host, which waits for the call."""

    def __init__(self, packed):
        self.packed = packed
        self._record = None

    @property
    def record(self):
        if self._record is None:
            self._record = self.packed.cpu().numpy().view(VOXELIZE_RESULT_DTYPE).reshape(())
        return self._record

    rejected = property(lambda self: int(self.record["rejected"]))
    degenerate = property(lambda self: int(self.record["degenerate"]))
    open_columns = property(lambda self: int(self.record["open_columns"]))


# ---- voxels -> quads (bm_mesh_quads / bm_host_mesh_quads)
QUAD_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("shape", "<u4")])   # bm_quad, 16 bytes: shape = d | w << 4 | h << 8
MESH_RESULT_DTYPE = np.dtype([("quads", "<u8"), ("faces", "<u8")])                     # bm_mesh_result, 16 bytes


def _mesh_params(lo, volume, halo, unit, name="volume"):
    """(bm_mesh_params, data pointer, is_cuda) of `volume` ([z, y, x], laid out as region_of takes it) with its voxel [0, 0, 0] at lo"""
    r, ptr, cuda = region_of(lo, volume, name)
    nz, ny, nx = volume.shape
    par = _lib.bm_mesh_params()
    par.lo[:] = list(r.lo)
    par.extent[:] = [nx, ny, nz]
    par.row_pitch, par.slice_pitch = r.row_pitch, r.slice_pitch
    par.flags = (_lib.BM_MESH_HALO if halo else 0) | (_lib.BM_MESH_UNIT_FACES if unit else 0)
    return par, ptr, cuda


def mesh_workspace_bytes(shape, halo=False, lo=(0, 0, 0)):
    """bm_mesh_workspace_bytes: device memory bm_mesh_quads needs beside its buffers for a volume of shape (nz, ny, nx) whose first voxel is
    world voxel lo (the cells are the world's, so their number depends on lo modulo 8)."""
    par = _lib.bm_mesh_params()
    par.lo[:] = [int(v) for v in lo]
    par.extent[:] = [int(shape[2]), int(shape[1]), int(shape[0])]
    par.flags = _lib.BM_MESH_HALO if halo else 0
    out = C.c_size_t(0)
    check(_lib.load().bm_mesh_workspace_bytes(C.byref(par), C.byref(out)))
    return int(out.value)


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
    rec = np.zeros((), MESH_RESULT_DTYPE)
    rec["quads"], rec["faces"] = res.quads, res.faces
    return quads, rec


def host_mesh_triangles(quads):
    """bm_host_mesh_triangles (host only): the two triangles of every quad (a QUAD_DTYPE array) as float32 [2 n, 3, 3], counter-clockwise
    seen from outside: what host_voxelize and Scene.voxelize read."""
    quads = np.ascontiguousarray(np.asarray(quads, dtype=QUAD_DTYPE).reshape(-1))
    tri = np.zeros((2 * len(quads), 3, 3), np.float32)
    check(_lib.load().bm_host_mesh_triangles(C.c_void_p(quads.ctypes.data), len(quads), C.c_void_p(tri.ctypes.data)))
    return tri


class Quads:
    """The quads of a Scene.mesh_quads, read lazily: `packed` is the quad buffer on the device (an int32 tensor [capacity, 4]) and
    `result` the bm_mesh_result there (two int64 words); count, faces, record (a MESH_RESULT_DTYPE scalar) and records (a QUAD_DTYPE array
    of the min(count, capacity) quads written) copy to the host, which waits for the call.  triangles() stays on the device."""

    def __init__(self, scene, packed, result, record=None):
        self.scene, self.packed, self.result = scene, packed, result
        self._record, self._records = record, None

    @property
    def record(self):
        if self._record is None:
            self._record = self.result.cpu().numpy().view(MESH_RESULT_DTYPE).reshape(())
        return self._record

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
        current, target = self.scene._volume_stream(self.packed, stream)
        with torch.cuda.stream(target):
            tri = torch.empty((2 * n, 3, 3), dtype=torch.float32, device=self.packed.device)
        if n:
            check(self.scene._L.bm_mesh_triangles(self.scene.gpuScene, C.c_void_p(self.packed.data_ptr()), n, C.c_void_p(tri.data_ptr()), C.c_void_p(target.cuda_stream)))
            if target.cuda_stream != current.cuda_stream:
                self.packed.record_stream(target)
                current.wait_stream(target)
        return tri


# ---- voxels -> distances (bm_distance_field / bm_host_distance_field)
DISTANCE_NONE = _lib.BM_DISTANCE_NONE
DISTANCE_RESULT_DTYPE = np.dtype([("sources", "<u8"), ("max_sq", "<u4"), ("reserved0", "<u4"), ("max_at", "<u8"), ("reserved1", "<u8")])  # bm_distance_result, 32 bytes


def _distance_flags(to, outside):
    if to not in ("solid", "empty"):
        raise ValueError(f"distance_field: to 'solid' or 'empty' expected, got {to!r}")
    return (_lib.BM_DISTANCE_TO_EMPTY if to == "empty" else 0) | (_lib.BM_DISTANCE_OUTSIDE if outside else 0)


def _distance_params(volume, to, outside, name="volume"):
    """(bm_distance_params, data pointer, is_cuda) of `volume` ([z, y, x], laid out as region_of takes it)"""
    flags = _distance_flags(to, outside)
    r, ptr, cuda = region_of((0, 0, 0), volume, name)
    nz, ny, nx = volume.shape
    par = _lib.bm_distance_params()
    par.extent[:] = [nx, ny, nz]
    par.row_pitch, par.slice_pitch = r.row_pitch, r.slice_pitch
    par.flags = flags
    return par, ptr, cuda


def distance_workspace_bytes(shape):
    """bm_distance_workspace_bytes: device memory bm_distance_field needs beside its buffers for a volume of shape (nz, ny, nx)."""
    par = _lib.bm_distance_params()
    par.extent[:] = [int(shape[2]), int(shape[1]), int(shape[0])]
    out = C.c_size_t(0)
    check(_lib.load().bm_distance_workspace_bytes(C.byref(par), C.byref(out)))
    return int(out.value)


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
    rec = np.zeros((), DISTANCE_RESULT_DTYPE)
    rec["sources"], rec["max_sq"], rec["max_at"] = res.sources, res.max_sq, res.max_at
    return field, rec


def host_distance_mask(field, limit_sq, above=False):
    """bm_host_distance_mask (host only): the uint8 volume field <= limit_sq (above=True: the opposite) of an int32 / uint32 field, in its
    shape; DISTANCE_NONE is above every limit."""
    field = np.ascontiguousarray(field)
    if field.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)):
        raise ValueError(f"host_distance_mask: an int32 or uint32 field expected, got {field.dtype}")
    out = np.zeros(field.shape, np.uint8)
    check(_lib.load().bm_host_distance_mask(field.size, C.c_void_p(field.ctypes.data), int(limit_sq), _lib.BM_DISTANCE_MASK_ABOVE if above else 0, C.c_void_p(out.ctypes.data)))
    return out


class DistanceField:
    """The field of a Scene.distance_field: `field` is the int32 tensor [z, y, x] on the device (DISTANCE_NONE where there is no source)
    and `result` the bm_distance_result there (four int64 words).  record (a DISTANCE_RESULT_DTYPE scalar) and largest() copy the result
    to the host, which waits for the call; mask() stays on the device."""

    def __init__(self, scene, field, result):
        self.scene, self.field, self.result = scene, field, result
        self._record = None

    @property
    def record(self):
        if self._record is None:
            self._record = self.result.cpu().numpy().view(DISTANCE_RESULT_DTYPE).reshape(())
        return self._record

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
        current, target = self.scene._volume_stream(self.field, stream)
        with torch.cuda.stream(target):
            if out is None:
                out = torch.empty(tuple(self.field.shape), dtype=torch.uint8, device=self.field.device)
        if not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != self.field.numel():
            raise ValueError("mask: out must be a contiguous uint8 tensor of the field's size on the scene's GPU")
        if target.cuda_stream != current.cuda_stream:
            self.field.record_stream(target)
            out.record_stream(target)
        check(self.scene._L.bm_distance_mask(self.scene.gpuScene, self.field.numel(), C.c_void_p(self.field.data_ptr()), int(radius_sq),
                                             _lib.BM_DISTANCE_MASK_ABOVE if above else 0, C.c_void_p(out.data_ptr()), C.c_void_p(target.cuda_stream)))
        if target.cuda_stream != current.cuda_stream:
            current.wait_stream(target)
        return out


# ---- voxels + seeds -> shortest face-step distances and paths (bm_travel_field / bm_host_travel_field)
TRAVEL_NONE = _lib.BM_TRAVEL_NONE
TRAVEL_RESULT_DTYPE = np.dtype([("reached", "<u8"), ("farthest", "<u4"), ("seeds_rejected", "<u4"), ("farthest_at", "<u8"), ("reserved", "<u8")])  # bm_travel_result, 32 bytes


def _travel_params(volume, max_steps, name="volume"):
    """(bm_travel_params, data pointer, is_cuda) of `volume` ([z, y, x], laid out as region_of takes it)"""
    if not 0 <= int(max_steps) <= 0xFFFFFFFF:
        raise ValueError(f"travel_field: max_steps in 0 ... 2^32 - 1 expected (0 = no limit), got {max_steps}")
    r, ptr, cuda = region_of((0, 0, 0), volume, name)
    nz, ny, nx = volume.shape
    par = _lib.bm_travel_params()
    par.extent[:] = [nx, ny, nz]
    par.max_steps = int(max_steps)
    par.row_pitch, par.slice_pitch = r.row_pitch, r.slice_pitch
    return par, ptr, cuda


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


def travel_workspace_bytes(shape):
    """bm_travel_workspace_bytes: device memory bm_travel_field needs beside its buffers for a volume of shape (nz, ny, nx)."""
    par = _lib.bm_travel_params()
    par.extent[:] = [int(shape[2]), int(shape[1]), int(shape[0])]
    out = C.c_size_t(0)
    check(_lib.load().bm_travel_workspace_bytes(C.byref(par), C.byref(out)))
    return int(out.value)


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
    rec = np.zeros((), TRAVEL_RESULT_DTYPE)
    rec["reached"], rec["farthest"], rec["seeds_rejected"], rec["farthest_at"] = res.reached, res.farthest, res.seeds_rejected, res.farthest_at
    return field, rec


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


class TravelField:
    """The field of a Scene.travel_field: `field` is the int32 tensor [z, y, x] on the device (TRAVEL_NONE where blocked, unreachable or
    beyond max_steps) and `result` the bm_travel_result there (four int64 words).  The field stands when travel_field returns.  record (a
    TRAVEL_RESULT_DTYPE scalar) and path() copy to the host, which waits; paths() stays on the device."""

    def __init__(self, scene, field, result):
        self.scene, self.field, self.result = scene, field, result
        self._record = None

    @property
    def record(self):
        if self._record is None:
            self._record = self.result.cpu().numpy().view(TRAVEL_RESULT_DTYPE).reshape(())
        return self._record

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
        if not (hasattr(starts, "is_cuda") and starts.is_cuda):
            starts = torch.from_numpy(_points(starts, "paths")).to(dev)
        if starts.dtype != torch.int32 or starts.dim() != 2 or starts.shape[1] != 3 or not starts.is_contiguous():
            raise ValueError("paths: starts must be a contiguous int32 tensor [n, 3]")
        n = int(starts.shape[0])
        current, target = self.scene._volume_stream(self.field, stream)
        with torch.cuda.stream(target):
            path = torch.full((n, capacity, 3), -1, dtype=torch.int32, device=dev)
            lengths = torch.zeros(n, dtype=torch.int32, device=dev)
        if target.cuda_stream != current.cuda_stream:
            for t in (self.field, starts, path, lengths):
                t.record_stream(target)
        nz, ny, nx = self.field.shape
        extent = (C.c_int32 * 3)(nx, ny, nz)
        check(self.scene._L.bm_travel_paths(self.scene.gpuScene, extent, C.c_void_p(self.field.data_ptr()), C.c_void_p(starts.data_ptr() if n else None), n, capacity,
                                            C.c_void_p(path.data_ptr() if n else None), C.c_void_p(lengths.data_ptr() if n else None), C.c_void_p(target.cuda_stream)))
        if target.cuda_stream != current.cuda_stream:
            current.wait_stream(target)
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


# ---- ray queries (bm_scene_cast_rays): packed records, 32 bytes each
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("tmax", "<f4"), ("reserved", "<u4")])   # bm_ray
RAY_HIT_DTYPE = np.dtype([("distance", "<f4"), ("normal", "<f4", 3), ("voxel", "<i4", 3), ("level", "<i4")])  # bm_ray_hit


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


def denoise_workspace_bytes(width, height):
    """bm_denoise_workspace_bytes: device memory bm_denoise needs beside its images (36 bytes per pixel)."""
    n = C.c_size_t(0)
    check(_lib.load().bm_denoise_workspace_bytes(int(width), int(height), C.byref(n)))
    return int(n.value)


def host_denoise(accum, hits, width=None, height=None, iterations=5, sigma_l=4.0, flags=0, reserved=0):
    """bm_host_denoise (host only, no device): the a-trous filter of Scene.denoise as plain loops.  accum: float32 [height, width, 4]
    (R, G, B, n); hits: a RAY_HIT_DTYPE array of height * width records (or float32 [height * width, 8]).  width / height default to
    accum's shape.  Returns float32 [height, width, 4] = (c, 1)."""
    accum = np.ascontiguousarray(accum, np.float32)
    if width is None or height is None:
        assert accum.ndim == 3 and accum.shape[2] == 4, "accum: [height, width, 4], or pass width and height"
        height, width = accum.shape[:2]
    hits = np.ascontiguousarray(hits)
    n = max(int(width), 0) * max(int(height), 0)
    assert accum.size == 4 * n and hits.nbytes == 32 * n, "accum: 4 floats per pixel; hits: one 32-byte record per pixel"
    out = np.zeros((max(int(height), 0), max(int(width), 0), 4), np.float32)
    par = _lib.bm_denoise_params(int(width), int(height), int(iterations), float(sigma_l), int(flags), int(reserved))
    check(_lib.load().bm_host_denoise(C.byref(par), accum.ctypes.data, hits.ctypes.data, out.ctypes.data))
    return out


def history_bytes(width, height):
    """bm_history_bytes: bytes of a history of Scene.reproject -- a float4 image, then the surface keys (20 bytes per pixel)."""
    n = C.c_size_t(0)
    check(_lib.load().bm_history_bytes(int(width), int(height), C.byref(n)))
    return int(n.value)


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
    accum = np.ascontiguousarray(accum, np.float32)
    if width is None or height is None:
        assert accum.ndim == 3 and accum.shape[2] == 4, "accum: [height, width, 4], or pass width and height"
        height, width = accum.shape[:2]
    hits = np.ascontiguousarray(hits)
    n = max(int(width), 0) * max(int(height), 0)
    assert accum.size == 4 * n and hits.nbytes == 32 * n, "accum: 4 floats per pixel; hits: one 32-byte record per pixel"
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
VOLUME_DTYPE = np.dtype([("shape", "<i4"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("center", "<i4", 3), ("radius", "<i4"), ("reserved", "<u4")])  # bm_volume
VOLUME_RESULT_DTYPE = np.dtype([("solid", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("unresolved", "<u4"), ("status", "<u4")])             # bm_volume_result


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
    L = _lib.load()
    arr = (C.c_void_p * int(count))()
    _lib.check(L.bm_probe_streams(int(device), int(count), arr))
    return [int(h) for h in arr]


def release_streams(handles):
    L = _lib.load()
    arr = (C.c_void_p * len(handles))(*handles)
    L.bm_release_streams(len(handles), arr)


class Scene:
    """Scene (Scene.h:7-44): CPU-built world + its residency on ONE GPU.

    World dimensions are a constructor argument here (the reference's are constexpr, variables.h:7-8);
    the defaults are the reference's 4096 x 4096 x 512 voxels.
    """

    def __init__(self, grid_size=4096, grid_height=512, device=0):
        self._L = _lib.load()
        self.device = device
        h = C.c_void_p()
        check(self._L.bm_scene_create(device, grid_size, grid_height, C.byref(h)))
        self.gpuScene = h  # the reference passes Scene::GPUScene by value; here it is the scene handle
        self.grid_size, self.grid_height = grid_size, grid_height

    def close(self):
        if getattr(self, "gpuScene", None):
            self._L.bm_scene_destroy(self.gpuScene)
            self.gpuScene = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference API
    def generate(self, threads=None):
        """Scene::generate (Scene.cpp:118-194)."""
        check(self._L.bm_scene_generate(self.gpuScene, threads or os.cpu_count() or 1))
        return self

    def generate_supercell(self, start_x, start_y, start_z):
        """Scene::generate_supercell (Scene.cpp:44-116), host only."""
        check(self._L.bm_scene_generate_supercell(self.gpuScene, start_x, start_y, start_z))

    def process_load_queue(self):
        """Scene::process_load_queue (Scene.cpp:200-252) + upload (kernel.cu:141-151). Returns bricks serviced."""
        n = C.c_uint32(0)
        check(self._L.bm_scene_process_load_queue(self.gpuScene, C.byref(n)))
        return int(n.value)

    def dump(self, path="dump.txt"):
        """Scene::dump (Scene.cpp:254-258)."""
        check(self._L.bm_scene_dump(self.gpuScene, path.encode()))

    # ---- additions the BASELINE configs need
    def preload_all(self):
        check(self._L.bm_scene_preload_all(self.gpuScene))
        return self

    def reset_residency(self):
        check(self._L.bm_scene_reset_residency(self.gpuScene))
        return self

    def set_lod(self, lod_distance_8x8x8=600000, lod_distance_2x2x2=100000):
        check(self._L.bm_scene_set_lod(self.gpuScene, lod_distance_8x8x8, lod_distance_2x2x2))
        return self

    def set_queue_capacity(self, capacity):
        check(self._L.bm_scene_set_queue_capacity(self.gpuScene, capacity))
        return self

    def set_streaming_mode(self, overlapped):
        """False: reference order (service right after the frame). True: double-buffered rings, no host wait."""
        check(self._L.bm_scene_set_streaming_mode(self.gpuScene, int(bool(overlapped))))
        return self

    def info(self):
        i = bm_scene_info()
        check(self._L.bm_scene_get_info(self.gpuScene, C.byref(i)))
        return {name: int(getattr(i, name)) for name, _ in bm_scene_info._fields_}

    def host_supercell(self, sc):
        idx = np.zeros(4096, np.uint32)
        n = C.c_uint32(0)
        check(self._L.bm_scene_host_supercell(self.gpuScene, sc, idx.ctypes.data, C.byref(n), None, 0))
        bricks = np.zeros((int(n.value), 16), np.uint32)
        if n.value:
            check(self._L.bm_scene_host_supercell(self.gpuScene, sc, None, None, bricks.ctypes.data, n.value))
        return idx, bricks

    def device_indices(self, sc):
        idx = np.zeros(4096, np.uint32)
        check(self._L.bm_scene_device_indices(self.gpuScene, sc, idx.ctypes.data))
        return idx

    def device_brick(self, sc, device_slot):
        out = np.zeros(16, np.uint32)
        check(self._L.bm_scene_device_brick(self.gpuScene, sc, device_slot, out.ctypes.data))
        return out

    def column_heights(self, sx, sy):
        out = np.zeros((128, 128), np.float32)
        check(self._L.bm_scene_column_heights(self.gpuScene, sx, sy, out.ctypes.data))
        return out

    # ---- a scene from the caller's voxels (bm_scene_load_voxels)
    def load_voxels(self, volume, stream=None):
        """Make `volume` the scene's world (replacing the one it holds, if any): a numpy array or a torch tensor, [z, y, x] of shape
        (grid_height, grid_size, grid_size), uint8 or bool, contiguous.  Host memory is built on CPU threads and uploaded; a tensor on
        the scene's GPU is packed on the GPU without leaving it, behind the work queued on `stream` (a raw HIP stream handle; None =
        torch's current stream, which the given stream is made to wait for).  The scene is preloaded when the call returns.  A wrong
        shape, dtype or layout raises ValueError before the library is called."""
        volume_dims(volume, self.grid_size, self.grid_height)
        if hasattr(volume, "is_contiguous"):
            import torch
            if volume.is_cuda:
                if volume.device.index != self.device:
                    raise ValueError(f"volume: a tensor on cuda:{self.device} (the scene's GPU) or on the CPU expected, got {volume.device}")
                current = torch.cuda.current_stream(volume.device)
                target = current if stream is None else torch.cuda.ExternalStream(int(stream), device=volume.device)
                if target.cuda_stream != current.cuda_stream:
                    target.wait_stream(current)
                check(self._L.bm_scene_load_voxels(self.gpuScene, C.c_void_p(volume.data_ptr()), volume.numel(), BM_VOXELS_DEVICE, C.c_void_p(target.cuda_stream)))
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
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        check(self._L.bm_scene_last_load_ms(self.gpuScene, C.byref(a), C.byref(b), C.byref(c)))
        return float(a.value), float(b.value), float(c.value)

    # ---- voxel edits (bm_scene_edit): ordered behind the frames in flight, seen by every frame issued after the call
    def _stream(self, stream):
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device).cuda_stream
        return C.c_void_p(stream)

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
        n = C.c_size_t(0)
        check(fn(self.gpuScene, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        check(fn(self.gpuScene, out.ctypes.data, out.size, C.byref(n)))
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
        n = C.c_size_t(0)
        check(self._L.bm_scene_escape_table(self.gpuScene, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        check(self._L.bm_scene_escape_table(self.gpuScene, out.ctypes.data, out.size, C.byref(n)))
        c = self.grid_size // 8
        return out.reshape(8, c, c)

    def last_edit_ms(self):
        """(scatter_ms, field_ms) of the last edit batch that changed the scene (hipEvents on the load stream)."""
        a, b = C.c_float(0), C.c_float(0)
        check(self._L.bm_scene_last_edit_ms(self.gpuScene, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    # ---- dense regions (bm_scene_write_region / bm_scene_read_region)
    def _volume_stream(self, tensor, stream):
        """(current, target) torch streams for a CUDA tensor of the scene's GPU: the call is issued on `target` (the given raw handle, or
        torch's current stream), which is made to wait for the current stream"""
        import torch
        if tensor.device.index != self.device:
            raise ValueError(f"a tensor on cuda:{self.device} (the scene's GPU) or on the CPU expected, got {tensor.device}")
        current = torch.cuda.current_stream(tensor.device)
        target = current if stream is None else torch.cuda.ExternalStream(int(stream), device=tensor.device)
        if target.cuda_stream != current.cuda_stream:
            target.wait_stream(current)
        return current, target

    def write_region(self, lo, volume, op="replace", stream=None):
        """Write a dense box of voxels into the live scene: `volume` ([z, y, x], uint8 or bool, numpy array or torch tensor; a slice of a
        larger one works as long as x is contiguous) lands with its first voxel at world voxel lo = (x, y, z).  op: "replace" (the box's
        voxels become the volume's), "set" (solid where the volume is non-zero) or "clear" (empty where it is non-zero).  Clipped to the
        world.  A tensor on the scene's GPU is packed there, behind the work queued on `stream` (a raw HIP stream handle; None = torch's
        current stream).  Ordered like an edit.  A wrong dtype, layout or device raises ValueError before the library is called."""
        r, ptr, cuda = region_of(lo, volume)
        if min(volume.shape) == 0:
            return self
        if cuda:
            _, target = self._volume_stream(volume, stream)
            check(self._L.bm_scene_write_region(self.gpuScene, C.byref(r), _region_op(op), C.c_void_p(ptr), BM_VOXELS_DEVICE, C.c_void_p(target.cuda_stream)))
        else:
            check(self._L.bm_scene_write_region(self.gpuScene, C.byref(r), _region_op(op), C.c_void_p(ptr), BM_VOXELS_HOST, self._stream(stream)))
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
            current, target = self._volume_stream(out, stream)
            check(self._L.bm_scene_read_region(self.gpuScene, C.byref(r), C.c_void_p(ptr), BM_VOXELS_DEVICE, C.c_void_p(target.cuda_stream)))
            if target.cuda_stream != current.cuda_stream:
                current.wait_stream(target)
        else:
            check(self._L.bm_scene_read_region(self.gpuScene, C.byref(r), C.c_void_p(ptr), BM_VOXELS_HOST, None))
        return result

    def last_region_ms(self):
        """(pack_ms, copy_ms, scatter_ms, field_ms) of the last write_region that reached the device (hipEvents on the load stream)."""
        t = [C.c_float(0) for _ in range(4)]
        check(self._L.bm_scene_last_region_ms(self.gpuScene, *[C.byref(v) for v in t]))
        return tuple(float(v.value) for v in t)

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
        current, target = self._volume_stream(out, stream)
        with torch.cuda.stream(target):
            count = torch.zeros(1, dtype=torch.int64, device=out.device)
        self.label_region_raw(lo, hi, out.data_ptr(), count.data_ptr(), 0, target.cuda_stream)
        if target.cuda_stream != current.cuda_stream:
            current.wait_stream(target)
        return out, count

    def last_label_ms(self):
        """(local_ms, merge_ms, flatten_ms) of the last label_region that launched its kernels (hipEvents on its stream)."""
        t = [C.c_float(0) for _ in range(3)]
        check(self._L.bm_scene_last_label_ms(self.gpuScene, *[C.byref(v) for v in t]))
        return tuple(float(v.value) for v in t)

    def components(self, lo, hi, stream=None):
        """label_region, then the table of every component (waits for the count): a Components."""
        import torch
        labels, count = self.label_region(lo, hi, stream=stream)
        n = int(count.item())
        table = torch.zeros((max(n, 1), COMPONENT_DTYPE.itemsize // 8), dtype=torch.int64, device=labels.device)
        if n:
            _, target = self._volume_stream(labels, stream)
            self.label_components_raw(lo, hi, labels.data_ptr(), table.data_ptr(), n, target.cuda_stream)
            target.synchronize()
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

    # ---- meshes -> voxels (bm_voxelize): the scene only names the GPU; nothing of the world is read
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
        current, target = self._volume_stream(tri, stream)
        with torch.cuda.stream(target):
            if out is None:
                out = torch.empty(tuple(int(v) for v in shape), dtype=torch.uint8, device=dev)
            par, ptr, _ = _voxelize_params(lo, out, mode, keep)
            n = int(tri.shape[0])
            ws = torch.empty(voxelize_workspace_bytes(out.shape, n, par.mode), dtype=torch.uint8, device=dev)
            packed = torch.empty(2, dtype=torch.int64, device=dev)
        if target.cuda_stream != current.cuda_stream:
            for x in (tri, out):
                x.record_stream(target)
        args = (self.gpuScene, C.byref(par), n, C.c_void_p(tri.data_ptr()), C.c_void_p(ptr), C.c_void_p(packed.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                C.c_void_p(target.cuda_stream))
        ms = None
        if times:
            ms = (C.c_float * 5)()
            check(self._L.bm_debug_voxelize_times(*args, ms))
        else:
            check(self._L.bm_voxelize(*args))
        if target.cuda_stream != current.cuda_stream:
            current.wait_stream(target)
        return out, VoxelizeResult(packed), ms

    def voxelize(self, triangles, lo, shape=None, mode="solid+surface", keep=False, out=None, stream=None):
        """bm_voxelize: fill a dense volume [z, y, x] of bytes 0 / 1 whose first voxel is world voxel lo = (x, y, z) from a
        triangle mesh -- a float32 tensor [n, 3, 3] on the scene's GPU (xyz per vertex, world voxel units), or (vertices [m, 3], faces
        [n, 3]), gathered with torch.  mode: "surface" (every voxel whose cube meets a triangle), "solid" (every voxel whose centre lies
        inside the closed mesh) or "solid+surface".  shape = (nz, ny, nx) for a new uint8 tensor, or `out`: a uint8 / bool CUDA tensor to
        fill (strides as in write_region); keep=True ORs into what `out` holds.  Returns (volume, VoxelizeResult); the result's
        open_columns is 0 for a closed mesh.  Stream handling as in write_region; the workspace comes from torch's pool; the host does
        not wait."""
        out, res, _ = self._voxelize(triangles, lo, shape, mode, keep, out, stream, False)
        return out, res

    def voxelize_times(self, triangles, lo, shape=None, mode="solid+surface", keep=False, out=None, stream=None):
        """bm_debug_voxelize_times: Scene.voxelize with a hipEvent between its stages; waits.  Returns (volume, VoxelizeResult, [ms of
        zeroing the workspace, plan + scan, the surface items, the solid items, the dense pass])."""
        out, res, ms = self._voxelize(triangles, lo, shape, mode, keep, out, stream, True)
        return out, res, [float(v) for v in ms]

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

    # ---- voxels -> quads (bm_mesh_quads): the scene only names the GPU; nothing of the world is read
    def _mesh_quads(self, volume, lo, halo, unit, capacity, stream, times):
        import torch
        if not hasattr(volume, "is_cuda") or not volume.is_cuda:
            raise ValueError("mesh_quads: volume must be a uint8 or bool tensor [z, y, x] on the scene's GPU")
        par, ptr, _ = _mesh_params(lo, volume, halo, unit)
        if min(volume.shape) == 0:
            raise ValueError(f"mesh_quads: a volume with positive extents expected, got shape {tuple(volume.shape)}")
        dev = volume.device
        current, target = self._volume_stream(volume, stream)
        with torch.cuda.stream(target):
            ws = torch.empty(mesh_workspace_bytes(volume.shape, halo, lo), dtype=torch.uint8, device=dev)
            result = torch.empty(2, dtype=torch.int64, device=dev)
        if target.cuda_stream != current.cuda_stream:
            volume.record_stream(target)
        ms = (C.c_float * 3)() if times else None

        def call(packed, cap):
            args = (self.gpuScene, C.byref(par), C.c_void_p(ptr), C.c_void_p(packed.data_ptr() if packed is not None else 0), cap, C.c_void_p(result.data_ptr()),
                    C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(target.cuda_stream))
            check(self._L.bm_debug_mesh_times(*args, ms) if times else self._L.bm_mesh_quads(*args))

        record = None
        if capacity is None:
            call(None, 0)
            with torch.cuda.stream(target):
                record = result.cpu().numpy().view(MESH_RESULT_DTYPE).reshape(())   # waits for the counting call
            capacity = int(record["quads"])
        capacity = int(capacity)
        with torch.cuda.stream(target):
            packed = torch.empty((capacity, 4), dtype=torch.int32, device=dev)
        if capacity > 0 or record is None:
            call(packed if capacity > 0 else None, capacity)
        if target.cuda_stream != current.cuda_stream:
            current.wait_stream(target)
        return Quads(self, packed, result, record), ([float(v) for v in ms] if times else None)

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
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if any(h <= l for l, h in zip(lo, hi)):
            raise ValueError(f"extract_mesh: an empty box ({lo} ... {hi})")
        if not closed:
            lo, hi = [v - 1 for v in lo], [v + 1 for v in hi]
        volume = self.read_region(lo, hi, device=True, stream=stream)
        return self.mesh_quads(volume, lo, halo=not closed, unit=unit, stream=stream)

    # ---- voxels -> distances (bm_distance_field): the scene only names the GPU; nothing of the world is read
    def _distance_field(self, volume, to, outside, out, stream, times):
        import torch
        if not hasattr(volume, "is_cuda") or not volume.is_cuda:
            raise ValueError("distance_field: volume must be a uint8 or bool tensor [z, y, x] on the scene's GPU")
        par, ptr, _ = _distance_params(volume, to, outside)
        if min(volume.shape) == 0:
            raise ValueError(f"distance_field: a volume with positive extents expected, got shape {tuple(volume.shape)}")
        dev = volume.device
        shape = tuple(int(v) for v in volume.shape)
        if out is not None and (not hasattr(out, "is_cuda") or not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError(f"distance_field: out must be a contiguous int32 tensor of shape {shape} on the scene's GPU")
        current, target = self._volume_stream(volume, stream)
        with torch.cuda.stream(target):
            if out is None:
                out = torch.empty(shape, dtype=torch.int32, device=dev)
            ws = torch.empty(distance_workspace_bytes(shape), dtype=torch.uint8, device=dev)
            result = torch.empty(4, dtype=torch.int64, device=dev)
        if target.cuda_stream != current.cuda_stream:
            volume.record_stream(target)
            out.record_stream(target)
        args = (self.gpuScene, C.byref(par), C.c_void_p(ptr), C.c_void_p(out.data_ptr()), C.c_void_p(result.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                C.c_void_p(target.cuda_stream))
        ms = None
        if times:
            ms = (C.c_float * 3)()
            check(self._L.bm_debug_distance_times(*args, ms))
        else:
            check(self._L.bm_distance_field(*args))
        if target.cuda_stream != current.cuda_stream:
            current.wait_stream(target)
        return DistanceField(self, out, result), ([float(v) for v in ms] if times else None)

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
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if any(h <= l for l, h in zip(lo, hi)):
            raise ValueError(f"clearance: an empty box ({lo} ... {hi})")
        return self.distance_field(self.read_region(lo, hi, device=True, stream=stream), stream=stream)

    def _morph(self, name, lo, hi, radius_sq, to, op, stream):
        import math
        radius_sq = int(radius_sq)
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if radius_sq < 1 or radius_sq > 3 * 16383 * 16383:
            raise ValueError(f"{name}: radius_sq, an integer in 1 ... 3 * 16383^2, expected, got {radius_sq}")
        if any(h <= l for l, h in zip(lo, hi)):
            raise ValueError(f"{name}: an empty box ({lo} ... {hi})")
        m = math.isqrt(radius_sq - 1) + 1  # ceil(sqrt(radius_sq))
        volume = self.read_region([v - m for v in lo], [v + m for v in hi], device=True, stream=stream)
        inner = (slice(m, -m),) * 3
        mask = self.distance_field(volume, to=to, stream=stream).mask(radius_sq, stream=stream)[inner]
        before = volume[inner] != 0
        changed = (mask != 0) & (before if op == "clear" else ~before)
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

    # ---- voxels + seeds -> shortest face-step distances (bm_travel_field): the scene only names the GPU; nothing of the world is read
    def _travel_field(self, volume, seeds, max_steps, out, stream, times, batch=0):
        import torch
        if not hasattr(volume, "is_cuda") or not volume.is_cuda:
            raise ValueError("travel_field: volume must be a uint8 or bool tensor [z, y, x] on the scene's GPU")
        par, ptr, _ = _travel_params(volume, max_steps)
        if min(volume.shape) == 0:
            raise ValueError(f"travel_field: a volume with positive extents expected, got shape {tuple(volume.shape)}")
        dev = volume.device
        shape = tuple(int(v) for v in volume.shape)
        if out is not None and (not hasattr(out, "is_cuda") or not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError(f"travel_field: out must be a contiguous int32 tensor of shape {shape} on the scene's GPU")
        current, target = self._volume_stream(volume, stream)
        with torch.cuda.stream(target):
            if not (hasattr(seeds, "is_cuda") and seeds.is_cuda):
                seeds = torch.from_numpy(_points(seeds, "travel_field")).to(dev)
            if seeds.dtype != torch.int32 or seeds.dim() != 2 or seeds.shape[1] != 3 or not seeds.is_contiguous():
                raise ValueError("travel_field: seeds must be a contiguous int32 tensor [n, 3]")
            if out is None:
                out = torch.empty(shape, dtype=torch.int32, device=dev)
            ws = torch.empty(travel_workspace_bytes(shape), dtype=torch.uint8, device=dev)
            result = torch.empty(4, dtype=torch.int64, device=dev)
        n = int(seeds.shape[0])
        if target.cuda_stream != current.cuda_stream:
            for t in (volume, seeds, out):
                t.record_stream(target)
        args = (self.gpuScene, C.byref(par), C.c_void_p(ptr), C.c_void_p(seeds.data_ptr() if n else None), n, C.c_void_p(out.data_ptr()), C.c_void_p(result.data_ptr()),
                C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(target.cuda_stream))
        info = None
        if times:
            ms, counts = (C.c_float * 3)(), (C.c_uint32 * 2)()
            check(self._L.bm_debug_travel_times(*args, int(batch), ms, counts))
            info = ([float(v) for v in ms], int(counts[0]), int(counts[1]))
        else:
            check(self._L.bm_travel_field(*args))
        if target.cuda_stream != current.cuda_stream:
            current.wait_stream(target)
        return TravelField(self, out, result), info

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
        import math
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        clearance_sq = int(clearance_sq)
        if any(h <= l for l, h in zip(lo, hi)):
            raise ValueError(f"{name}: an empty box ({lo} ... {hi})")
        if clearance_sq < 0 or clearance_sq > 3 * 16383 * 16383:
            raise ValueError(f"{name}: clearance_sq, an integer in 0 ... 3 * 16383^2, expected, got {clearance_sq}")
        if clearance_sq == 0:
            return self.read_region(lo, hi, device=True, stream=stream)
        m = math.isqrt(clearance_sq - 1) + 1  # ceil(sqrt(clearance_sq))
        volume = self.read_region([v - m for v in lo], [v + m for v in hi], device=True, stream=stream)
        return self.distance_field(volume, to="solid", stream=stream).mask(clearance_sq - 1, stream=stream)[(slice(m, -m),) * 3]

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

    # ---- ray queries (bm_scene_cast_rays): issued like a frame -- after every edit and upload issued before, asynchronous to the host
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
        # Everything the query touches is made on the stream it runs on: the packed rays and the hits come from that stream's pool, the
        # stream first waits for the work queued so far on the current stream (which wrote the inputs), and an input tensor read there is
        # marked as in use by it, so that the caching allocator does not hand its memory out again while the query still reads it.
        current = torch.cuda.current_stream(dev)
        target = current if stream is None else torch.cuda.ExternalStream(int(stream), device=dev)
        other = target.cuda_stream != current.cuda_stream
        if other:
            target.wait_stream(current)
        with torch.cuda.stream(target):
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
                if other:
                    for x in inputs:
                        x.record_stream(target)
                n = rays.shape[0]
                hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
                self.cast_rays_raw(n, rays.data_ptr(), hits.data_ptr(), flags, lod_origin, target.cuda_stream)
                return RayHits(hits[:, 0], hits[:, 1:4], hits[:, 4:7].view(torch.int32), hits[:, 7].view(torch.int32), hits)
            rays = origins if directions is None else pack_rays(origins, directions, tmax)
            rays = np.ascontiguousarray(rays)
            assert rays.dtype == RAY_DTYPE, "packed rays: a RAY_DTYPE array"
            n = len(rays)
            out = np.zeros(n, RAY_HIT_DTYPE)
            if n:
                d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8)).to(dev)
                d_hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
                self.cast_rays_raw(n, d_rays.data_ptr(), d_hits.data_ptr(), flags, lod_origin, target.cuda_stream)
                target.synchronize()
                out = d_hits.cpu().numpy().view(RAY_HIT_DTYPE).reshape(n)
            return RayHits(out["distance"], out["normal"], out["voxel"], out["level"], out)

    def _target_stream(self, dev, stream):
        """(target, other): the torch stream a call runs on -- `stream` (a raw handle) or the current one -- made to wait for the work queued
        on the current stream so far; other: it is not the current stream (inputs then need record_stream)"""
        import torch
        current = torch.cuda.current_stream(dev)
        target = current if stream is None else torch.cuda.ExternalStream(int(stream), device=dev)
        other = target.cuda_stream != current.cuda_stream
        if other:
            target.wait_stream(current)
        return target, other

    def pixel_rays(self, camera, width, height, stream=None):
        """bm_camera_pixel_rays_device: the pixel-centre rays of a width x height frame of `camera`, written on the device -- a float32
        [height * width, 8] CUDA tensor of packed bm_ray records, ray y * width + x through pixel (x, y), bit for bit what
        camera_pixel_rays gives for (x + 0.5, y + 0.5).  Ready in stream order on `stream` (None = torch's current stream)."""
        import torch
        dev = torch.device("cuda", self.device)
        target, _ = self._target_stream(dev, stream)
        with torch.cuda.stream(target):
            rays = torch.empty((int(height) * int(width), 8), dtype=torch.float32, device=dev)
            c = camera.to_c()
            check(self._L.bm_camera_pixel_rays_device(self.gpuScene, C.byref(c), int(width), int(height), C.c_void_p(rays.data_ptr()), C.c_void_p(target.cuda_stream)))
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

    def _denoise_args(self, accum, hits, width, height, iterations, sigma_l, out, stream):
        import torch
        hits = hits.packed if isinstance(hits, RayHits) else hits
        n = int(width) * int(height)
        assert accum.is_cuda and accum.dtype == torch.float32 and accum.is_contiguous() and accum.numel() == 4 * n, "accum: float32 [height, width, 4] on the GPU"
        assert hits.is_cuda and hits.dtype == torch.float32 and hits.is_contiguous() and hits.numel() == 8 * n, "hits: the packed records, float32 [height * width, 8]"
        target, other = self._target_stream(accum.device, stream)
        with torch.cuda.stream(target):
            if out is None:
                out = torch.empty_like(accum)
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == 4 * n, "out: like accum"
            ws = torch.empty(denoise_workspace_bytes(width, height), dtype=torch.uint8, device=accum.device)
        if other:
            for x in (accum, hits, out):
                x.record_stream(target)
        par = _lib.bm_denoise_params(int(width), int(height), int(iterations), float(sigma_l), 0, 0)
        return par, hits, out, ws, target

    def denoise(self, accum, hits, width, height, iterations=5, sigma_l=4.0, out=None, stream=None):
        """bm_denoise: the edge-avoiding a-trous filter of an accumulation buffer `accum` (float32 [height, width, 4]: R, G, B,
        n), guided by `hits` (Scene.pixel_hits, or its .packed tensor).  Returns (c, 1) per pixel -- what Scene.resolve takes -- in `out`
        (None = a new tensor; may be accum itself).  The workspace comes from torch's pool on the stream the filter runs on: `stream` (a raw
        HIP stream handle; None = torch's current stream), which first waits for the work queued on the current stream.  The host does not wait."""
        par, hits, out, ws, target = self._denoise_args(accum, hits, width, height, iterations, sigma_l, out, stream)
        check(self._L.bm_denoise(self.gpuScene, C.byref(par), C.c_void_p(accum.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(out.data_ptr()),
                                 C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(target.cuda_stream)))
        return out

    def denoise_times(self, accum, hits, width, height, iterations=5, sigma_l=4.0, out=None, stream=None):
        """bm_debug_denoise_times: Scene.denoise with a hipEvent between its kernels; waits.  Returns (out, [ms of prepare, the variance pass,
        every a-trous pass])."""
        par, hits, out, ws, target = self._denoise_args(accum, hits, width, height, iterations, sigma_l, out, stream)
        ms = (C.c_float * (2 + max(int(iterations), 0)))()
        check(self._L.bm_debug_denoise_times(self.gpuScene, C.byref(par), C.c_void_p(accum.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(target.cuda_stream), ms))
        return out, [float(v) for v in ms]

    def reproject(self, accum, hits, camera, prev_camera, history_prev, width, height, max_history=32.0, out=None, stream=None):
        """bm_reproject: temporal accumulation for a moving camera.  `accum` (float32 [height, width, 4]: R, G, B, n) is the
        frame just rendered with `camera`, `hits` its guides (Scene.pixel_hits, or its .packed tensor); `history_prev` is the History of the
        frame before, rendered with `prev_camera`, or None (no history: the result is accum and its keys).  Returns the new History -- `out`,
        or a new one; never history_prev itself: the taps read neighbours, so two histories take turns.  Its .image is an accumulation buffer
        of up to max_history + the frame's own samples per pixel, which Scene.denoise and Scene.resolve take.  Stream handling as in
        Scene.denoise; the host does not wait."""
        import torch
        hits = hits.packed if isinstance(hits, RayHits) else hits
        n = int(width) * int(height)
        assert accum.is_cuda and accum.dtype == torch.float32 and accum.is_contiguous() and accum.numel() == 4 * n, "accum: float32 [height, width, 4] on the GPU"
        assert hits.is_cuda and hits.dtype == torch.float32 and hits.is_contiguous() and hits.numel() == 8 * n, "hits: the packed records, float32 [height * width, 8]"
        assert history_prev is None or (history_prev.buffer.is_cuda and history_prev.buffer.numel() == 5 * n), "history_prev: a History of this size on the GPU"
        target, other = self._target_stream(accum.device, stream)
        with torch.cuda.stream(target):
            if out is None:
                out = History(torch.empty(5 * n, dtype=torch.float32, device=accum.device), width, height)
        assert out.buffer.is_cuda and out.buffer.dtype == torch.float32 and out.buffer.numel() == 5 * n, "out: a History of this size on the GPU"
        if other:
            for x in (accum, hits, out.buffer) + ((history_prev.buffer,) if history_prev is not None else ()):
                x.record_stream(target)
        par = _lib.bm_reproject_params(int(width), int(height), float(max_history), 0, 0)
        c, cp = camera.to_c(), (prev_camera.to_c() if prev_camera is not None else None)
        check(self._L.bm_reproject(self.gpuScene, C.byref(par), C.byref(c), C.byref(cp) if cp is not None else None, C.c_void_p(accum.data_ptr()),
                                   C.c_void_p(hits.data_ptr()), C.c_void_p(history_prev.buffer.data_ptr()) if history_prev is not None else None,
                                   C.c_void_p(out.buffer.data_ptr()), C.c_void_p(target.cuda_stream)))
        return out

    def pick(self, camera, x, y, width, height, lod_origin=None):
        """The voxel under pixel (x, y) of a width x height frame of `camera`: one ray through the pixel's centre, one query, then the host
        waits.  Returns a RayHit, or None on a miss.  (A level-3 hit means the brick is not resident yet: service the load queue and pick again.)"""
        rays = camera_pixel_rays(camera, width, height, [x + 0.5], [y + 0.5])
        h = self.cast_rays(rays, lod_origin=lod_origin).packed[0]
        if int(h["level"]) < 0:
            return None
        return RayHit(float(h["distance"]), tuple(float(v) for v in h["normal"]), tuple(int(v) for v in h["voxel"]), int(h["level"]))

    # ---- volume queries (bm_scene_query_volumes): issued like a ray query, asynchronous to the host
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
        current = torch.cuda.current_stream(dev)
        target = current if stream is None else torch.cuda.ExternalStream(int(stream), device=dev)
        other = target.cuda_stream != current.cuda_stream
        if other:
            target.wait_stream(current)
        with torch.cuda.stream(target):  # (what the query touches is made on the stream it runs on, as in cast_rays)
            if isinstance(volumes, torch.Tensor):
                assert volumes.is_cuda and volumes.dtype == torch.uint8 and volumes.is_contiguous() and volumes.numel() % 48 == 0, "packed volumes: contiguous uint8, 48 bytes per record, on the GPU"
                if other:
                    volumes.record_stream(target)
                n = volumes.numel() // 48
                res = torch.empty((n, 40), dtype=torch.uint8, device=dev)
                self.query_volumes_raw(n, volumes.data_ptr(), res.data_ptr(), flags, target.cuda_stream)
                return VolumeResults(res[:, 0:8].view(torch.int64).reshape(n), res[:, 8:20].view(torch.int32), res[:, 20:32].view(torch.int32),
                                     res[:, 32:36].view(torch.int32).reshape(n), res[:, 36:40].view(torch.int32).reshape(n), res)
            volumes = np.ascontiguousarray(volumes)
            assert volumes.dtype == VOLUME_DTYPE, "packed volumes: a VOLUME_DTYPE array"
            n = volumes.size
            out = np.zeros(n, VOLUME_RESULT_DTYPE)
            if n:
                d_vol = torch.from_numpy(volumes.reshape(n).view(np.uint8).reshape(n, 48)).to(dev)
                d_res = torch.empty((n, 40), dtype=torch.uint8, device=dev)
                self.query_volumes_raw(n, d_vol.data_ptr(), d_res.data_ptr(), flags, target.cuda_stream)
                target.synchronize()
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

    def synchronize(self):
        check(self._L.bm_synchronize(self.gpuScene))

    def last_render_ms(self):
        ms = C.c_float(0)
        check(self._L.bm_last_render_ms(self.gpuScene, C.byref(ms)))
        return float(ms.value)

    def render_times(self, capacity=256):
        """Kernel durations (ms) of the most recent launches, oldest first (hipEvents on the launch stream)."""
        ms = np.zeros(capacity, np.float32)
        n = C.c_int(0)
        check(self._L.bm_render_times(self.gpuScene, ms.ctypes.data, capacity, C.byref(n)))
        return ms[: n.value].copy()

    def counters(self):
        c = bm_counters()
        check(self._L.bm_counters_read(self.gpuScene, C.byref(c)))
        return c.as_dict()

    def sched_stats(self):
        """Per-phase run / active-lane counts of the wave scheduler (instrumented launches only)."""
        st = _lib.bm_sched_stats()
        check(self._L.bm_sched_stats_read(self.gpuScene, C.byref(st)))
        return {n: int(getattr(st, n)) for n in _lib.SCHED_NAMES}

    def sched_detail(self):
        """-DBM_PHASE_TIMING builds: time split of the shade pass and loop lengths of the candidate pass (bm_sched_detail_read)."""
        out = (C.c_uint64 * 8)()
        check(self._L.bm_sched_detail_read(self.gpuScene, out))
        names = ("connect_cycles", "shade_hit_cycles", "sky_cycles", "primary_cycles", "setup_cycles", "brick_passes", "brick_loop_trips", "brick_lane_steps")
        return dict(zip(names, (int(v) for v in out)))

    def counters_reset(self):
        check(self._L.bm_counters_reset(self.gpuScene))

    def render(self, camera: Camera, params: FrameParams, accum, debug=None, stream=None):
        """bm_render_frame: add params.spp paths per pixel into `accum` (torch CUDA float32 [rows, W, 4])."""
        import torch
        rows = local_rows(params)
        assert accum.is_cuda and accum.dtype == torch.float32 and accum.is_contiguous()
        assert accum.numel() == rows * params.width * 4, "accum must be [local_rows, width, 4]"
        dbg_ptr = None
        if debug is not None:
            assert debug.is_cuda and debug.dtype == torch.int32 and debug.is_contiguous() and debug.numel() == rows * params.width * 8
            dbg_ptr = C.c_void_p(debug.data_ptr())
        if stream is None:
            stream = torch.cuda.current_stream(accum.device).cuda_stream
        cam_c, par_c = camera.to_c(), params.to_c()
        check(self._L.bm_render_frame(self.gpuScene, C.byref(cam_c), C.byref(par_c), C.c_void_p(accum.data_ptr()), dbg_ptr,
                                      C.c_void_p(stream)))

    def render_frames(self, cameras, params, accums, debugs=None, stream=None):
        """bm_render_frames: `len(params)` consecutive frames -- the reference's per-frame loop, main.cpp:117-147 -- as ONE launch (the
        frame ring: every wave walks from a used-up frame to the next by itself).  cameras: one Camera for all frames or one per frame;
        accums: one tensor for all frames (production frames add with float atomics) or one per frame; debugs: None or one entry per frame
        (None or a hit-record tensor of its own)."""
        import torch
        n = len(params)
        cams = list(cameras) if isinstance(cameras, (list, tuple)) else [cameras] * n
        accs = list(accums) if isinstance(accums, (list, tuple)) else [accums] * n
        dbgs = list(debugs) if debugs is not None else None
        assert len(cams) == n and len(accs) == n and (dbgs is None or len(dbgs) == n)
        cam_c = (_lib.bm_camera * n)(*[c.to_c() for c in cams])
        par_c = (_lib.bm_frame_params * n)(*[p.to_c() for p in params])
        acc_p = (C.c_void_p * n)()
        dbg_p = (C.c_void_p * n)() if dbgs is not None else None
        for i in range(n):
            rows = local_rows(params[i])
            a = accs[i]
            assert a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and a.numel() == rows * params[i].width * 4, "accum must be [local_rows, width, 4]"
            acc_p[i] = a.data_ptr()
            if dbgs is not None and dbgs[i] is not None:
                d = dbgs[i]
                assert d.is_cuda and d.dtype == torch.int32 and d.is_contiguous() and d.numel() == rows * params[i].width * 8
                dbg_p[i] = d.data_ptr()
        if stream is None:
            stream = torch.cuda.current_stream(accs[0].device if accs else None).cuda_stream
        check(self._L.bm_render_frames(self.gpuScene, n, cam_c, par_c, acc_p, dbg_p, C.c_void_p(stream)))

    def resolve(self, accum, out=None, stream=None):
        """blit_onto_framebuffer (kernel.cu:348-364) into an offscreen float4 tensor."""
        import torch
        if out is None:
            out = torch.empty_like(accum)
        if stream is None:
            stream = torch.cuda.current_stream(accum.device).cuda_stream
        check(self._L.bm_resolve(self.gpuScene, C.c_void_p(accum.data_ptr()), C.c_void_p(out.data_ptr()), accum.numel() // 4,
                                 C.c_void_p(stream)))
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


# numpy views of the queue records (variables.h:43-52 RayQueue, :54-59 ShadowQueue)
RAY_QUEUE_DTYPE = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("throughput", "<f4", 3), ("normal", "<f4", 3),
                            ("distance", "<f4"), ("identifier", "<i4"), ("bounces", "<i4"), ("pixel_index", "<u4")])
SHADOW_QUEUE_DTYPE = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("color", "<f4", 3), ("pixel_index", "<u4")])


class Wavefront:
    """The reference's own schedule (kernel.cu:366-439): every `frame()` is one launch_kernels call -- primary_rays
    tops the work queue up to `queue_size` (ray_queue_buffer_size, variables.h:61), extend, shade, connect, swap --
    so a path needs max_bounces + 1 frames.  Holds what the reference keeps in statics / __device__ globals
    (frame counter, start_position, primary_ray_cnt) and in State (the two ray queues and the shadow queue)."""

    def __init__(self, scene: Scene, queue_size=2 * 1048576):
        self._L = _lib.load()
        self.scene, self.queue_size = scene, queue_size
        self.handle = C.c_void_p()
        check(self._L.bm_wavefront_create(scene.gpuScene, queue_size, C.byref(self.handle)))

    def close(self):
        if getattr(self, "handle", None):
            self._L.bm_wavefront_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def reset(self):
        """reset_buffer branch of launch_kernels (:397-403); the caller zeroes the accumulation buffer."""
        check(self._L.bm_wavefront_reset(self.handle))

    def frame(self, camera: Camera, params: FrameParams, accum, stream=None):
        import torch
        assert accum.is_cuda and accum.dtype == torch.float32 and accum.is_contiguous()
        assert accum.numel() == params.width * params.height * 4, "accum must be [height, width, 4]"
        if stream is None:
            stream = torch.cuda.current_stream(accum.device).cuda_stream
        cam_c, par_c = camera.to_c(), params.to_c()
        check(self._L.bm_wavefront_frame(self.handle, C.byref(cam_c), C.byref(par_c), C.c_void_p(accum.data_ptr()), C.c_void_p(stream)))

    def stats(self):
        out = np.zeros(6, np.uint32)
        check(self._L.bm_wavefront_stats(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return dict(survivors=int(out[0]), shadow=int(out[1]), start_position=int(out[2]), frame=int(out[3]),
                    generated=int(out[4]), primary_ray_cnt=int(out[5]))

    def read_queue(self, which, first=0, count=None):
        """which = "work" (RayQueue records; the survivors of the last frame lead) or "shadow"."""
        kind = {"work": 0, "shadow": 1}[which]
        dtype = RAY_QUEUE_DTYPE if kind == 0 else SHADOW_QUEUE_DTYPE
        if count is None:
            count = self.queue_size - first
        out = np.zeros(count, dtype)
        check(self._L.bm_wavefront_read_queue(self.handle, kind, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def counters(self, which="both"):
        """traversal counters of the BM_FLAG_COUNTERS frames: of the "extend" kernel, the "connect" kernel, or "both" """
        c = bm_counters()
        check(self._L.bm_wavefront_counters_read(self.handle, {"extend": 0, "connect": 1, "both": 2}[which], C.byref(c)))
        return c.as_dict()

    def counters_reset(self):
        check(self._L.bm_wavefront_counters_reset(self.handle))

    def sched_stats(self, which="extend"):
        """wave-scheduler statistics of the BM_FLAG_COUNTERS frames of the "extend" or "connect" kernel"""
        out = (C.c_uint64 * 6)()
        check(self._L.bm_wavefront_sched_stats_read(self.handle, {"extend": 0, "connect": 1}[which], out))
        names = ("step_runs", "step_lanes", "candidate_runs", "candidate_lanes", "refills", "refill_rays")
        return dict(zip(names, (int(v) for v in out)))

    def times(self):
        """hipEvent durations (ms) of the last frame."""
        ms = (C.c_float * 5)()
        check(self._L.bm_wavefront_times(self.handle, ms))
        return dict(total=ms[0], primary=ms[1], extend=ms[2], shade=ms[3], connect=ms[4])


class State:
    """state.h:5-34 minus the wavefront queues and the GL interop: owns the float4 accumulation
    ("blit") buffer of this process' shard of the frame."""

    def __init__(self, screen_width, screen_height, device=0, band_rows=0, shard_rank=0, shard_count=1):
        import torch
        self.screen_width, self.screen_height = screen_width, screen_height
        self.device = torch.device("cuda", device)
        self.band_rows, self.shard_rank, self.shard_count = band_rows, shard_rank, shard_count
        self._alloc()

    def _alloc(self):
        import torch
        rows = local_rows(FrameParams(self.screen_width, self.screen_height, band_rows=self.band_rows,
                                      shard_rank=self.shard_rank, shard_count=self.shard_count))
        self.local_rows = rows
        self.blit_buffer = torch.zeros((rows, self.screen_width, 4), dtype=torch.float32, device=self.device)

    def screen_resize(self, screen_width, screen_height):
        self.screen_width, self.screen_height = screen_width, screen_height
        self._alloc()


@dataclass
class _LaunchStatics:
    """The function-local statics of launch_kernels (kernel.cu:367-382)."""
    first_time: bool = True
    frame: int = 1
    sample_base: int = 0
    last: tuple = field(default_factory=tuple)
    sun_position: tuple = (0.05, 0.1)
    sun_position_changed: bool = True


_statics = _LaunchStatics()


def launch_kernels(state: State, blit_buffer, gpuScene: Scene, camera: Camera, spp=1, max_bounces=3, flags=0,
                   sun_position=None, statics=None, queues: "Wavefront" = None):
    """launch_kernels (launch.h:6, kernel.cu:366-439) for the per-pixel design.

    Differences forced by the redesign (DESIGN.md "Boundary"): no GL surface and no ray queues
    (paths live in registers); one call traces `spp` complete paths per pixel instead of advancing
    every in-flight path by one bounce.  As in the reference, a change of camera position /
    direction / focal distance / lens radius or of the sun resets the accumulation buffer
    (kernel.cu:387-403).  Returns 0 (the reference always returns cudaSuccess, kernel.cu:438).

    With `queues` (a Wavefront: the reference's ray_buffer_work / ray_buffer_next / shadow_queue_buffer) the call is
    the reference's own schedule instead: every path in flight advances by one segment, `spp` is ignored.
    """
    st = statics or _statics
    if sun_position is not None and tuple(sun_position) != st.sun_position:
        st.sun_position = tuple(sun_position)
        st.sun_position_changed = True
    key = (tuple(camera.position), tuple(camera.direction), camera.focalDistance, camera.lensRadius)
    reset_buffer = key != st.last
    if st.sun_position_changed:
        st.sun_position_changed = False
        reset_buffer = True
    if reset_buffer:
        blit_buffer.zero_()
        st.sample_base = 0
    if queues is not None:
        assert state.shard_count == 1, "the queue schedule does not shard"
        if reset_buffer and not st.first_time:
            queues.reset()
        queues.frame(camera, FrameParams(state.screen_width, state.screen_height, max_bounces=max_bounces, flags=flags,
                                         sun_position=st.sun_position), blit_buffer)
        st.frame += 1
        st.first_time = False
        st.last = key
        return 0
    params = FrameParams(state.screen_width, state.screen_height, spp=spp, sample_base=st.sample_base, max_bounces=max_bounces,
                         base_frame=1, flags=flags, band_rows=state.band_rows, shard_rank=state.shard_rank,
                         shard_count=state.shard_count, sun_position=st.sun_position)
    gpuScene.render(camera, params, blit_buffer)
    st.sample_base += spp
    st.frame += 1
    st.first_time = False
    st.last = key
    return 0
