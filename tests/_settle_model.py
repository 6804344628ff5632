"""The numpy model of the settling contract (include/brickmap.h, bm_settle), written from the header's sentences only: the contacts of
every column by a plain loop, the drops by relaxing the list of contacts until nothing changes, then a scatter -- no rounds, no groups,
no shared step function.  And the cases the host and the device tests share (cases())."""
from bisect import bisect_left

import numpy as np

RESULT_DTYPE = np.dtype([("moved_voxels", "<u8"), ("chosen_pieces", "<u4"), ("moved_pieces", "<u4"), ("largest_drop", "<u4"), ("reserved", "<u4"), ("contacts", "<u8")])
COMPONENT_DTYPE = np.dtype([("label", "<i4"), ("faces", "<u4"), ("voxels", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)])
UNKNOWN = None
NAMES = ["cube over nothing", "cube over flat ground", "a piece that is not chosen hangs", "a label missing from the table", "two stacked pieces", "three stacked pieces",
         "a piece resting on two pieces", "two interlocked pieces", "13 pieces in one column", "a staircase of 20 pieces", "70 x 17 x 33 at density 0.05", "70 x 17 x 33 at density 0.15",
         "70 x 17 x 33 at density 0.3", "height 1", "height 7", "height 8", "height 9", "height 17", "n = 0", "chosen all zero", "a table cut to its first half",
         "the only moving piece in the last column group"]
FACES = {"-x": 1, "+x": 2, "-y": 4, "+y": 8, "-z": 16, "+z": 32}


def model_settle(labels, records, chosen):
    """(out, drops, record) of a label volume [z, y, x], a table in ascending label and one value per record"""
    labels = np.asarray(labels)
    nz, ny, nx = labels.shape
    table = [int(v) for v in np.asarray(records)["label"]]
    chosen = [bool(v) for v in np.asarray(chosen).reshape(-1)]
    assert table == sorted(table) and len(chosen) == len(table), "the model searches ascending tables only"

    def moving(label):   # the slot of a moving label, None for a static one
        slot = bisect_left(table, label)
        return slot if slot < len(table) and table[slot] == label and chosen[slot] else None

    contacts = []   # (upper slot, lower slot or None, gap)
    for y in range(ny):
        for x in range(nx):
            below_label, below_z = None, -1   # the floor
            for z in range(nz):
                label = int(labels[z, y, x])
                if label == 0:
                    continue
                if label != below_label and moving(label) is not None:
                    contacts.append((moving(label), None if below_label is None else moving(below_label), z - below_z - 1))
                below_label, below_z = label, z
    drop = [UNKNOWN if c else 0 for c in chosen]
    changed = True
    while changed:
        changed = False
        for upper, lower, gap in contacts:
            base = 0 if lower is None else drop[lower]
            if base is UNKNOWN:
                continue
            if drop[upper] is UNKNOWN or base + gap < drop[upper]:
                drop[upper] = base + gap
                changed = True
    drop = [0 if d is UNKNOWN else d for d in drop]   # a chosen record at which no voxel's search arrives
    out = np.zeros(labels.shape, np.uint8)
    for z, y, x in np.argwhere(labels != 0):
        slot = moving(int(labels[z, y, x]))
        d = 0 if slot is None else drop[slot]
        assert z - d >= 0 and out[z - d, y, x] == 0, "two voxels on one, or one below the floor"
        out[z - d, y, x] = 2 if d else 1
    rec = np.zeros((), RESULT_DTYPE)
    rec["moved_voxels"] = int((out == 2).sum())
    rec["chosen_pieces"] = sum(chosen)
    rec["moved_pieces"] = sum(1 for d in drop if d)
    rec["largest_drop"] = max(drop, default=0)
    rec["contacts"] = len(contacts)
    return out, np.array(drop, np.int32).reshape(-1), rec


def table_of(labels):
    """the component table of a label volume [z, y, x], as bm_scene_label_components writes it for a box at the origin"""
    labels = np.asarray(labels)
    nz, ny, nx = labels.shape
    values = np.unique(labels[labels != 0])
    records = np.zeros(len(values), COMPONENT_DTYPE)
    for i, v in enumerate(values):
        z, y, x = np.nonzero(labels == v)
        records[i] = (v, (x.min() == 0) * 1 | (x.max() == nx - 1) * 2 | (y.min() == 0) * 4 | (y.max() == ny - 1) * 8 | (z.min() == 0) * 16 | (z.max() == nz - 1) * 32,
                      len(z), (x.min(), y.min(), z.min()), (x.max() + 1, y.max() + 1, z.max() + 1))
    return records


def loose(records, anchor=("-x", "+x", "-y", "+y", "-z")):
    bits = sum(FACES[a] for a in anchor)
    return ((records["faces"] & bits) == 0).astype(np.uint8)


def label_and_table(bm, volume):
    labels, count = bm.host_label_volume(np.asarray(volume, np.uint8))
    records = table_of(labels)
    assert len(records) == count
    return labels, records


# the interlocked pair, written by hand: a C (label 5) in the plane y = 1, open towards +x, a bar (label 7) along y through its opening
# and a post (label 9, not chosen) under the bar's end at y = 0.  The bar can fall 2, onto the post; the C hangs on the bar.
INTERLOCKED = np.zeros((6, 3, 3), np.int32)   # [z, y, x]
INTERLOCKED[5, 1, :] = INTERLOCKED[3, 1, :] = INTERLOCKED[4, 1, 0] = 5
INTERLOCKED[4, :, 1] = 7
INTERLOCKED[0:2, 0, 1] = 9
INTERLOCKED_OUT = np.zeros((6, 3, 3), np.uint8)
INTERLOCKED_OUT[3, 1, :] = INTERLOCKED_OUT[1, 1, :] = INTERLOCKED_OUT[2, 1, 0] = 2
INTERLOCKED_OUT[2, :, 1] = 2
INTERLOCKED_OUT[0:2, 0, 1] = 1


# The staircase, written by hand: 20 pieces of two voxels each, labels 10 ... 29 (a piece need not hang together).  Piece k has one voxel
# in column x = k at z = 16 (21 - k) + 4, just above a voxel of piece k - 1 (one empty voxel between them), and one in column x = k + 1
# just below piece k + 1; piece 0 stands one voxel above a static post (label 5).  So piece k rests on piece k - 1 and falls k + 1 -- and
# the contact that tells it so lies a whole run of slices BELOW the contact that tells piece k - 1: a lane that walks upwards meets the
# contacts in the wrong order, a round settles one piece, and the device needs 20 rounds and one more (the 13 pieces in one column above
# can settle in a single round, since one lane walks them from the bottom: they were done within the first batch).
STAIRS = 20
STAIRCASE = np.zeros((16 * (STAIRS + 1) + 6, 1, STAIRS), np.int32)   # [z, y, x]
STAIRCASE[0:16 * (STAIRS + 1) + 3, 0, 0] = 5
for _k in range(STAIRS):
    STAIRCASE[16 * (STAIRS + 1 - _k) + 4, 0, _k] = 10 + _k
    if _k < STAIRS - 1:
        STAIRCASE[16 * (STAIRS - _k) + 2, 0, _k + 1] = 10 + _k


def chosen_of(records, volume_labels, *voxels):
    """one byte per record: 1 for the pieces that own the given voxels (x, y, z)"""
    chosen = np.zeros(len(records), np.uint8)
    for x, y, z in voxels:
        chosen[np.searchsorted(records["label"], volume_labels[z, y, x])] = 1
    return chosen


_CASES = {}


def cases(bm):
    """name -> (labels int32 [z, y, x], records, chosen, expected drops of the chosen records by hand or None)"""
    if _CASES:
        return _CASES

    def add(name, volume, voxels, want=None, cut=None):
        labels, records = label_and_table(bm, volume)
        chosen = chosen_of(records, labels, *voxels)
        if cut is not None:
            records, chosen = cut(records, chosen)
        _CASES[name] = (labels, records, chosen, want)

    v = np.zeros((10, 8, 8), np.uint8)
    v[4:6, 3:5, 3:5] = 1
    add("cube over nothing", v.copy(), [(3, 3, 4)], [4])
    v[0] = 1
    add("cube over flat ground", v.copy(), [(3, 3, 4)], [3])
    v[7:9, 0:2, 0:2] = 1
    add("a piece that is not chosen hangs", v.copy(), [(3, 3, 4)], [3])
    # a slab whose label is cut out of the table is static; the cube lands on it
    v = np.zeros((10, 8, 8), np.uint8)
    v[2, 2:6, 2:6] = 1
    v[6:8, 3:5, 3:5] = 1
    add("a label missing from the table", v, [(3, 3, 6)], [3], cut=lambda r, c: (r[1:], c[1:]))
    v = np.zeros((12, 4, 5), np.uint8)
    v[3, 1:3, 1:4] = 1
    v[8, 1, 1] = 1
    add("two stacked pieces", v.copy(), [(1, 1, 3), (1, 1, 8)], [3, 7])
    v[10:12, 1, 1:3] = 1
    add("three stacked pieces", v.copy(), [(1, 1, 3), (1, 1, 8), (1, 1, 10)], [3, 7, 8])
    # a beam over a post of three voxels that falls 1 and a block that falls 4: it follows the post, 1 + 3, not the block, 4 + 2
    v = np.zeros((9, 3, 7), np.uint8)
    v[1:4, 1, 0] = v[4, 1, 6] = 1
    v[7, 1, :] = 1
    add("a piece resting on two pieces", v, [(0, 1, 1), (6, 1, 4), (3, 1, 7)], [1, 4, 4])
    records = table_of(INTERLOCKED)
    _CASES["two interlocked pieces"] = (INTERLOCKED, records, np.array([1, 1, 0], np.uint8), [2, 2])
    v = np.zeros((26, 2, 3), np.uint8)
    v[1::2, 1, 1] = 1
    add("13 pieces in one column", v, [(1, 1, z) for z in range(1, 26, 2)], list(range(1, 14)))
    _CASES["a staircase of 20 pieces"] = (STAIRCASE, table_of(STAIRCASE), np.array([0] + [1] * STAIRS, np.uint8), list(range(1, STAIRS + 1)))
    for density in (0.05, 0.15, 0.3):
        rng = np.random.default_rng(int(density * 100))
        labels, records = label_and_table(bm, rng.random((33, 17, 70)) < density)
        _CASES[f"70 x 17 x 33 at density {density}"] = (labels, records, (rng.random(len(records)) < 0.7).astype(np.uint8), None)
    for nz in (1, 7, 8, 9, 17):
        rng = np.random.default_rng(nz)
        labels, records = label_and_table(bm, rng.random((nz, 5, 9)) < 0.2)
        _CASES[f"height {nz}"] = (labels, records, (rng.random(len(records)) < 0.7).astype(np.uint8), None)
    labels, records = label_and_table(bm, np.random.default_rng(5).random((9, 6, 11)) < 0.2)
    _CASES["n = 0"] = (labels, records[:0], np.zeros(0, np.uint8), None)
    _CASES["chosen all zero"] = (labels, records, np.zeros(len(records), np.uint8), None)
    half = len(records) // 2
    _CASES["a table cut to its first half"] = (labels, records[:half], np.ones(half, np.uint8), None)
    # 130 x 3 x 6: 390 columns in 7 groups; static clutter everywhere, the only chosen piece in the last group (columns 384 ... 389)
    v = (np.random.default_rng(6).random((6, 3, 130)) < 0.2)
    v[:, 2, 124:] = False
    v[4, 1, 127] = False
    v[4, 2, 127] = True
    add("the only moving piece in the last column group", v, [(127, 2, 4)], [4])
    return _CASES
