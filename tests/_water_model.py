"""The numpy model of the spill-level contract (include/brickmap.h, bm_water_field and bm_water_mask), written from the header's sentences
only: for every height h in rising order the outlets at or below h are flooded through the free voxels at or below h by shifting along
the three axes until nothing changes, and a voxel reached for the first time gets max(h, sea_level) -- no tiles, no lists, no rounds, no
queue.  (What was reached at h - 1 is reached at h, so each height goes on from the one before.)"""
import numpy as np

NONE = 0x7FFFFFFF
RESULT_DTYPE = np.dtype([("wet", "<u8"), ("deepest", "<u4"), ("drains_rejected", "<u4"), ("deepest_at", "<u8"), ("closed", "<u8")])
FACES = {"-x": 1, "+x": 2, "-y": 4, "+y": 8, "-z": 16, "+z": 32}
SIDES = ("-x", "+x", "-y", "+y")


def model_water_field(volume, drains=None, open=SIDES, sea_level=0):
    """(field, record) of a volume [z, y, x] (non-zero = solid, z up), drains [n, 3] of (x, y, z) and the names of the open faces"""
    free = np.asarray(volume) == 0
    nz, ny, nx = free.shape
    outlet = np.zeros(free.shape, bool)
    for name in ([open] if isinstance(open, str) else open):
        axis, side = {"x": 2, "y": 1, "z": 0}[name[1]], (0 if name[0] == "-" else -1)
        index = [slice(None)] * 3
        index[axis] = side
        outlet[tuple(index)] = True
    outlet &= free
    rejected = 0
    for x, y, z in np.asarray([] if drains is None else drains, np.int64).reshape(-1, 3):
        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and free[z, y, x]:
            outlet[z, y, x] = True
        else:
            rejected += 1
    field = np.full(free.shape, NONE, np.int64)
    reached = np.zeros(free.shape, bool)
    for h in range(nz):
        low, r = free[:h + 1], reached[:h + 1]   # the slab z <= h (views: r writes through)
        r |= outlet[:h + 1]
        while True:
            grown = r.copy()
            grown[1:] |= r[:-1]
            grown[:-1] |= r[1:]
            grown[:, 1:] |= r[:, :-1]
            grown[:, :-1] |= r[:, 1:]
            grown[:, :, 1:] |= r[:, :, :-1]
            grown[:, :, :-1] |= r[:, :, 1:]
            grown &= low
            if (grown == r).all():
                break
            r[...] = grown
        field[reached & (field == NONE)] = max(h, int(sea_level))
    z = np.arange(nz, dtype=np.int64)[:, None, None]
    depth = np.where(field != NONE, field - z, 0)
    assert (depth >= 0).all()
    rec = np.zeros((), RESULT_DTYPE)
    rec["wet"] = int((depth > 0).sum())
    rec["closed"] = int((free & (field == NONE)).sum())
    rec["drains_rejected"] = rejected
    if depth.max() > 0:
        rec["deepest"] = int(depth.max())
        rec["deepest_at"] = int(np.flatnonzero(depth.ravel() == depth.max())[0])   # the lowest index
    return field.astype(np.int32), rec


def model_water_mask(field, min_depth=1):
    field = np.asarray(field).astype(np.int64)
    z = np.arange(field.shape[0], dtype=np.int64)[:, None, None]
    return ((field != NONE) & (field - z >= max(int(min_depth), 1)) & (field > z)).astype(np.uint8)


def counts(field):
    """(wet, dry, closed-or-solid) voxels of a field"""
    field = np.asarray(field).astype(np.int64)
    z = np.arange(field.shape[0], dtype=np.int64)[:, None, None]
    return int(((field != NONE) & (field > z)).sum()), int((field == z).sum()), int((field == NONE).sum())
