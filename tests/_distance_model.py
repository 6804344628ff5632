"""The numpy model of the distance-field contract (include/brickmap.h, bm_distance_field), written from the header's sentences only: the
minimum over all sources by brute force, with broadcasting -- no separable passes and no envelope."""
import numpy as np

NONE = 0x7FFFFFFF
RESULT_DTYPE = np.dtype([("sources", "<u8"), ("max_sq", "<u4"), ("reserved0", "<u4"), ("max_at", "<u8"), ("reserved1", "<u8")])


def model_sources(volume, to="solid"):
    """the sources of the volume: its solid voxels (any non-zero byte), or with to="empty" its empty ones"""
    solid = np.asarray(volume) != 0
    return solid if to == "solid" else ~solid


def model_distance_field(volume, to="solid", outside=False, chunk=None):
    """(field, record) of a volume [z, y, x]: D(p) = min over the sources q of |p - q|^2 (NONE without a source); with `outside` every
    voxel outside the volume is a source too, which is min(D, m^2), m = the least over the axes of min(i + 1, n - i)."""
    src = model_sources(volume, to)
    nz, ny, nx = src.shape
    z, y, x = np.indices(src.shape, dtype=np.int64)
    pz, py, px = (a.reshape(-1, 1) for a in (z, y, x))
    q = np.argwhere(src).astype(np.int64)
    out = np.full(src.size, NONE, np.int64)
    chunk = chunk or max(16, (1 << 21) // src.size)   # sources at a time: a few million differences in flight
    for first in range(0, len(q), chunk):
        qz, qy, qx = (q[first:first + chunk, k].reshape(1, -1) for k in range(3))
        out = np.minimum(out, ((pz - qz) ** 2 + (py - qy) ** 2 + (px - qx) ** 2).min(axis=1))
    out = out.reshape(src.shape)
    if outside:
        m = np.minimum.reduce([x + 1, nx - x, y + 1, ny - y, z + 1, nz - z])
        out = np.minimum(out, m * m)
    rec = np.zeros((), RESULT_DTYPE)
    rec["sources"] = int(src.sum())
    finite = out[out != NONE]
    if finite.size:
        rec["max_sq"] = int(finite.max())
        rec["max_at"] = int(np.flatnonzero(out.ravel() == finite.max())[0])  # the lowest index
    else:
        rec["max_sq"] = NONE
    return out.astype(np.int32), rec


def model_mask(field, limit_sq, above=False):
    """out = (D <= limit_sq) ? 1 : 0, inverted with `above`; NONE is above every limit"""
    field = np.asarray(field).astype(np.int64)
    within = (field != NONE) & (field <= int(limit_sq))
    return (within != bool(above)).astype(np.uint8)


def model_ball(radius_sq):
    """the offsets (dz, dy, dx) of the Euclidean ball of squared radius radius_sq"""
    m = int(np.ceil(np.sqrt(radius_sq)))
    r = np.arange(-m, m + 1)
    dz, dy, dx = np.meshgrid(r, r, r, indexing="ij")
    keep = dz * dz + dy * dy + dx * dx <= radius_sq
    return np.stack([dz[keep], dy[keep], dx[keep]], axis=1), m


def model_dilate(solid, radius_sq):
    """the voxels within sqrt(radius_sq) of a solid voxel; everything outside the array is empty.  By shifting, not by distances."""
    solid = np.asarray(solid) != 0
    offsets, m = model_ball(radius_sq)
    pad = np.pad(solid, m)
    out = np.zeros_like(solid)
    nz, ny, nx = solid.shape
    for dz, dy, dx in offsets:
        out |= pad[m + dz:m + dz + nz, m + dy:m + dy + ny, m + dx:m + dx + nx]
    return out


def model_erode(solid, radius_sq):
    """the solid voxels farther than sqrt(radius_sq) from every empty voxel; everything outside the array is empty"""
    solid = np.asarray(solid) != 0
    m = model_ball(radius_sq)[1]
    return ~model_dilate(~np.pad(solid, m), radius_sq)[m:-m, m:-m, m:-m]
