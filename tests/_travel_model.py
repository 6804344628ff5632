"""The numpy model of the travel-field contract (include/brickmap.h, bm_travel_field and bm_travel_paths), written from the header's
sentences only: a level-by-level search by shifting the front along the three axes -- no tiles, no lists, no rounds; the path rule is a
plain loop."""
import numpy as np

NONE = 0x7FFFFFFF
RESULT_DTYPE = np.dtype([("reached", "<u8"), ("farthest", "<u4"), ("seeds_rejected", "<u4"), ("farthest_at", "<u8"), ("reserved", "<u8")])
NEIGHBOURS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))   # (dx, dy, dz): -x, +x, -y, +y, -z, +z


def model_travel_field(volume, seeds, max_steps=0):
    """(field, record) of a volume [z, y, x] (non-zero = blocked) and seeds [n, 3] of (x, y, z)"""
    open_ = np.asarray(volume) == 0
    nz, ny, nx = open_.shape
    field = np.full(open_.shape, NONE, np.int64)
    front = np.zeros(open_.shape, bool)
    rejected = 0
    for x, y, z in np.asarray(seeds, np.int64).reshape(-1, 3):
        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and open_[z, y, x]:
            front[z, y, x] = True
        else:
            rejected += 1
    field[front] = 0
    level = 0
    while front.any() and (max_steps == 0 or level < max_steps):
        level += 1
        grown = np.zeros_like(front)
        grown[1:] |= front[:-1]
        grown[:-1] |= front[1:]
        grown[:, 1:] |= front[:, :-1]
        grown[:, :-1] |= front[:, 1:]
        grown[:, :, 1:] |= front[:, :, :-1]
        grown[:, :, :-1] |= front[:, :, 1:]
        front = grown & open_ & (field == NONE)
        field[front] = level
    rec = np.zeros((), RESULT_DTYPE)
    finite = field[field != NONE]
    rec["reached"] = finite.size
    rec["seeds_rejected"] = rejected
    if finite.size:
        rec["farthest"] = int(finite.max())
        rec["farthest_at"] = int(np.flatnonzero(field.ravel() == finite.max())[0])   # the lowest index
    else:
        rec["farthest"] = NONE
    return field.astype(np.int32), rec


def model_travel_paths(field, starts, capacity):
    """(path [n, capacity, 3] with -1 where nothing is written, lengths [n]) by the header's rule"""
    field = np.asarray(field).astype(np.int64)
    nz, ny, nx = field.shape
    starts = np.asarray(starts, np.int64).reshape(-1, 3)
    path = np.full((len(starts), capacity, 3), -1, np.int32)
    lengths = np.zeros(len(starts), np.int32)
    for q, (x, y, z) in enumerate(starts):
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz) or field[z, y, x] == NONE:
            continue
        t = int(field[z, y, x])
        lengths[q] = t + 1
        path[q, 0] = (x, y, z)
        for k in range(1, min(t + 1, capacity)):
            for dx, dy, dz in NEIGHBOURS:
                u, v, w = x + dx, y + dy, z + dz
                if 0 <= u < nx and 0 <= v < ny and 0 <= w < nz and field[w, v, u] == t - 1:
                    break
            else:
                lengths[q] = -1
                break
            x, y, z, t = u, v, w, t - 1
            path[q, k] = (x, y, z)
    return path, lengths


def check_full_path(volume, field, path):
    """a full path on its own: consecutive voxels one face step apart, none blocked, values descending by one to 0"""
    path = np.asarray(path, np.int64)
    assert (np.abs(np.diff(path, axis=0)).sum(axis=1) == 1).all()
    values = np.asarray(field)[path[:, 2], path[:, 1], path[:, 0]]
    assert (values == np.arange(len(path) - 1, -1, -1)).all()
    assert not np.asarray(volume)[path[:, 2], path[:, 1], path[:, 0]].any()
