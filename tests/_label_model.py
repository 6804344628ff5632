"""Helpers of the connected-component tests (no tests here): the numpy model of the labelling contract of include/brickmap.h
(bm_scene_label_region), the component table computed from a label volume, and the hand-made shapes at which each kernel of
csrc/label.hip can go wrong.  Volumes are [z, y, x]."""
import functools

import numpy as np

FACES = ("-x", "+x", "-y", "+y", "-z", "+z")
COMPONENT_DTYPE = np.dtype([("label", "<i4"), ("faces", "<u4"), ("voxels", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)])


def model_labels(vol):
    """(labels, count, rounds): min-label propagation over the six neighbours until nothing changes.  labels: int32, 0 for empty voxels,
    else 1 + the smallest index ((z * ny + y) * nx + x) of the voxel's component.  Slow (one round per step of the longest path): small volumes only."""
    solid = np.asarray(vol) != 0
    big = np.int64(solid.size + 1)
    lab = np.where(solid, np.arange(1, solid.size + 1, dtype=np.int64).reshape(solid.shape), big)
    rounds = 0
    while True:
        rounds += 1
        new = lab.copy()
        for axis in range(3):
            n = lab.shape[axis]
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[axis], b[axis] = slice(1, n), slice(0, n - 1)
            a, b = tuple(a), tuple(b)
            new[a] = np.minimum(new[a], lab[b])
            new[b] = np.minimum(new[b], lab[a])
        new[~solid] = big
        if np.array_equal(new, lab):
            break
        lab = new
    lab = np.where(solid, lab, 0).astype(np.int32)
    count = int(np.count_nonzero(lab == np.arange(1, solid.size + 1, dtype=np.int64).reshape(solid.shape)))
    return lab, count, rounds


def model_records(labels, lo, world_dims):
    """the component table of a label volume whose voxel [0, 0, 0] is world voxel lo = (x, y, z): one record per label in ascending
    order; the faces are those of the box clipped to a world of world_dims = (X, Y, Z)"""
    labels = np.asarray(labels)
    nz, ny, nx = labels.shape
    hi = (lo[0] + nx, lo[1] + ny, lo[2] + nz)
    clo = [max(0, int(lo[k])) for k in range(3)]
    chi = [min(int(world_dims[k]), int(hi[k])) for k in range(3)]
    flat = labels.reshape(-1)
    at = np.flatnonzero(flat)
    uniq, inverse, counts = np.unique(flat[at], return_inverse=True, return_counts=True)
    recs = np.zeros(len(uniq), COMPONENT_DTYPE)
    recs["label"], recs["voxels"] = uniq, counts
    coords = (at % nx + lo[0], at // nx % ny + lo[1], at // (nx * ny) + lo[2])
    for k, v in enumerate(coords):
        mn = np.full(len(uniq), np.iinfo(np.int64).max)
        mx = np.full(len(uniq), np.iinfo(np.int64).min)
        np.minimum.at(mn, inverse, v)
        np.maximum.at(mx, inverse, v)
        recs["lo"][:, k], recs["hi"][:, k] = mn, mx + 1
        low, high = np.zeros(len(uniq), bool), np.zeros(len(uniq), bool)
        np.logical_or.at(low, inverse, v == clo[k])
        np.logical_or.at(high, inverse, v == chi[k] - 1)
        recs["faces"] |= (low.astype(np.uint32) << (2 * k)) | (high.astype(np.uint32) << (2 * k + 1))
    return recs


def same_partition(a, b):
    """two label volumes name the same components (whatever the labels are)"""
    a, b = np.asarray(a).reshape(-1).astype(np.int64), np.asarray(b).reshape(-1).astype(np.int64)
    if not np.array_equal(a != 0, b != 0):
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


# ---------------------------------------------------------------- hand-made shapes: name -> uint8 [z, y, x]
def serpentine(n=24):
    """a one-voxel-wide path through an n^3 box that crosses brick faces dozens of times, one component: in every second slice the rows
    at even y run along x and are joined at alternating ends; a slice is joined to the next one at the end of its path and that one to
    the one after it at the path's start, in turn"""
    v = np.zeros((n, n, n), np.uint8)
    last_y = (n - 1) // 2 * 2
    end_x = n - 1 if (last_y // 2) % 2 == 0 else 0
    for z in range(0, n, 2):
        for y in range(0, n, 2):
            v[z, y, :] = 1
            if y + 2 < n:
                v[z, y + 1, n - 1 if (y // 2) % 2 == 0 else 0] = 1
        if z + 2 < n:
            if (z // 2) % 2 == 0:
                v[z + 1, last_y, end_x] = 1
            else:
                v[z + 1, 0, 0] = 1
    return v


def combs(n=24):
    """two interleaved combs that touch only along edges and at corners, so they stay two components: comb A has teeth at (x even,
    y even) hanging from a spine at z = 0, comb B teeth at (x odd, y odd) from a spine at z = n - 1; a tooth of A and one of B share a
    vertical edge, never a face"""
    v = np.zeros((n, n, n), np.uint8)
    v[0:n - 2, 0::2, 0::2] = 1      # teeth of A
    v[0, 0::2, :] = 1               # spine of A: the rows at even y ...
    v[0, :, 0] = 1                  # ... joined along x = 0
    v[2:n, 1::2, 1::2] = 1          # teeth of B
    v[n - 1, 1::2, :] = 1
    v[n - 1, :, n - 1] = 1
    return v


def u_shape(n=40):
    """two pillars along z, joined only at their far end (z = n - 1): the second pillar's voxels are re-rooted late"""
    v = np.zeros((n, 12, 30), np.uint8)
    v[:, 3:6, 2:5] = 1
    v[:, 3:6, 24:27] = 1
    v[n - 1, 4, 2:27] = 1
    return v


def checkerboard(n=12):
    z, y, x = np.indices((n, n, n))
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def solid_block(n=64):
    return np.ones((n, n, n), np.uint8)


@functools.lru_cache(maxsize=None)
def shape(name):
    v = {"serpentine": serpentine, "combs": combs, "u_shape": u_shape, "checkerboard": checkerboard, "solid_block": solid_block}[name]()
    v.setflags(write=False)
    return v


SHAPES = ("serpentine", "combs", "u_shape", "checkerboard", "solid_block")
# components of each shape (what the model must find, by construction)
SHAPE_COUNTS = {"serpentine": 1, "combs": 2, "u_shape": 1, "checkerboard": 12 ** 3 // 2, "solid_block": 1}


def seeded_volume(seed, shape_zyx, fill):
    return (np.random.default_rng(seed).random(shape_zyx) < fill).astype(np.uint8)
