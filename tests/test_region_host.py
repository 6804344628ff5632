"""The host half of bm_scene_write_region (no GPU), through bm_host_write_region_supercell: the bits each op gives against numpy slice
assignment, the slots against bm_host_edit_supercell with the per-cell set-then-clear batch that include/brickmap.h names, untouched
cells, clipping, pitches and refusals.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from _load_model import canonical_supercell, expand_supercell

EINVAL = 10001
G = 128  # a world of one supercell


@pytest.fixture(scope="module")
def terrain(bm):
    """(indices, bricks, voxels) of the generated 128^3 world's only supercell"""
    idx, bricks = bm.host_generate_supercell(G, G, 0, 0, 0)
    vol = np.zeros((G, G, G), np.uint8)
    expand_supercell(vol, 0, 0, 0, idx, bricks)
    assert 0 < len(bricks) < 4096 and (idx == 0).any()
    return idx, bricks, vol


def voxels_of(idx, bricks, sx=0, sy=0, sz=0, size=G, height=G):
    vol = np.zeros((height, size, size), np.uint8)
    expand_supercell(vol, sx, sy, sz, idx, bricks)
    return vol


def model_write(vol, lo, V, op):
    """numpy model: the part of V inside the world lands at lo"""
    Z, Y, X = vol.shape
    nz, ny, nx = V.shape
    a = [max(0, -lo[0]), max(0, -lo[1]), max(0, -lo[2])]
    b = [min(nx, X - lo[0]), min(ny, Y - lo[1]), min(nz, Z - lo[2])]
    if any(h <= l for l, h in zip(a, b)):
        return vol
    out = vol.copy()
    src = (V[a[2]:b[2], a[1]:b[1], a[0]:b[0]] != 0).astype(np.uint8)
    dst = np.s_[lo[2] + a[2]:lo[2] + b[2], lo[1] + a[1]:lo[1] + b[1], lo[0] + a[0]:lo[0] + b[0]]
    if op == "replace":
        out[dst] = src
    elif op == "set":
        out[dst] |= src
    else:
        out[dst] &= ~src & 1
    return out


def check_consistent(idx, bricks, vol):
    """words, LoD masks and bricks are what the canonical build stores for `vol`, whatever the slots"""
    words, want = canonical_supercell(vol, 0, 0, 0)
    occ = words != 0
    assert np.array_equal(idx != 0, occ)
    live = idx[occ]
    assert ((live & np.uint32(0x80000000)) != 0).all() and not (live & np.uint32(0x7FF00000)).any()
    slots = live & np.uint32(0xFFF)
    assert len(np.unique(slots)) == len(slots) and (slots < len(bricks)).all()
    assert np.array_equal((live >> np.uint32(12)) & np.uint32(0xFF), (words[occ] >> np.uint32(12)) & np.uint32(0xFF))
    assert np.array_equal(bricks[slots], want)


BOXES = {
    "aligned": ((16, 32, 40), (64, 24, 48)),                 # lo, (nz, ny, nx): whole bricks
    "unaligned": ((9, 18, 27), (62 - 27, 53 - 18, 44 - 9)),  # lo at residues 1, 2, 3 and hi at 4, 5, 6 mod 8
    "inside one cell": ((41, 50, 66), (3, 4, 5)),
    "one voxel": ((77, 13, 63), (1, 1, 1)),
}


@pytest.mark.parametrize("op", ["replace", "set", "clear"])
@pytest.mark.parametrize("box", list(BOXES))
def test_each_op_gives_the_models_bits(bm, terrain, op, box):
    idx, bricks, vol = terrain
    lo, shape = BOXES[box]
    if box == "unaligned":
        hi = tuple(l + n for l, n in zip(lo, shape[::-1]))
        assert len({v % 8 for v in lo + hi}) == 6
    rng = np.random.default_rng(sum(map(ord, op + box)))
    for fill in (0.5, 0.0, 1.0):
        V = (rng.random(shape) < fill).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)  # non-zero = solid, any value
        want = model_write(vol, lo, V, op)
        i2, b2 = bm.host_write_region_supercell(G, G, 0, 0, 0, idx, bricks, lo, V, op)
        assert np.array_equal(voxels_of(i2, b2), want)
        check_consistent(i2, b2, want)
        i3, b3 = bm.host_write_region_supercell(G, G, 0, 0, 0, idx, bricks, lo, V != 0, op)  # a bool volume
        assert np.array_equal(i3, i2) and np.array_equal(b3, b2)


def cell_slice(local):
    x, y, z = (local & 15) * 8, ((local >> 4) & 15) * 8, (local >> 8) * 8
    return np.s_[z:z + 8, y:y + 8, x:x + 8]


def set_then_clear_batch(bm, old, new):
    """cell by cell in ascending local index, for each changed cell: set the voxels of new & ~old, then clear those of old & ~new"""
    edits = []
    for local in range(4096):
        sl = cell_slice(local)
        o, n = old[sl] != 0, new[sl] != 0
        if np.array_equal(o, n):
            continue
        x0, y0, z0 = (local & 15) * 8, ((local >> 4) & 15) * 8, (local >> 8) * 8
        for op, mask in (("set", n & ~o), ("clear", o & ~n)):
            for z, y, x in np.argwhere(mask):
                v = (x0 + int(x), y0 + int(y), z0 + int(z))
                edits.append(bm.edit_box(op, v, tuple(c + 1 for c in v)))
    return edits


def test_slots_equal_the_edit_door_with_the_set_then_clear_batch(bm, terrain):
    idx, bricks, vol = terrain
    lo, hi = (19, 27, 35), (77, 69, 101)
    inside = [l for l in range(4096) if all(lo[k] <= c * 8 and c * 8 + 8 <= hi[k] for k, c in enumerate((l & 15, (l >> 4) & 15, l >> 8)))]
    new = vol.copy()
    loses = next(l for l in inside if idx[l] != 0)
    new[cell_slice(loses)] = 0
    gains = [l for l in inside if l > loses and idx[l] == 0][:2]
    assert len(gains) == 2
    for l in gains:
        new[cell_slice(l)][3, 4, 5] = 1
    changes = next(l for l in inside if l > gains[1] and idx[l] != 0 and 2 <= vol[cell_slice(l)].sum() < 512)
    z, y, x = np.argwhere(vol[cell_slice(changes)])[0]
    new[cell_slice(changes)][z, y, x] = 0
    z, y, x = np.argwhere(vol[cell_slice(changes)] == 0)[0]
    new[cell_slice(changes)][z, y, x] = 1
    V = new[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].copy()
    # a partly covered cell changes too: one voxel on the box's low x face
    edge = np.argwhere(V[:, :, 0] == 0)[0]
    V[edge[0], edge[1], 0] = 1
    new[lo[2] + edge[0], lo[1] + edge[1], lo[0]] = 1

    i2, b2 = bm.host_write_region_supercell(G, G, 0, 0, 0, idx, bricks, lo, V, "replace")
    batch = set_then_clear_batch(bm, vol, new)
    assert len(batch) > 64
    i3, b3 = bm.host_edit_supercell(G, G, 0, 0, 0, idx, bricks, batch)
    assert np.array_equal(i2, i3), f"{np.count_nonzero(i2 != i3)} index words differ from the edit door's"
    assert b2.shape == b3.shape and np.array_equal(b2, b3)
    assert np.array_equal(voxels_of(i2, b2), new)
    # each kind of cell occurs
    assert idx[loses] != 0 and i2[loses] == 0
    assert all(idx[l] == 0 and i2[l] != 0 for l in gains)
    assert (i2[gains[0]] & 0xFFF) == (idx[loses] & 0xFFF), "the later cell did not take the slot just freed"
    assert (i2[gains[1]] & 0xFFF) == len(bricks), "with no freed slot left a new brick is appended"
    assert (i2[changes] & 0xFFF) == (idx[changes] & 0xFFF) and not np.array_equal(b2[i2[changes] & 0xFFF], bricks[idx[changes] & 0xFFF])
    same = [l for l in inside if l not in (loses, changes, *gains) and idx[l] != 0]
    assert same and all(i2[l] == idx[l] and np.array_equal(b2[i2[l] & 0xFFF], bricks[idx[l] & 0xFFF]) for l in same)


def raw_write(bm, idx, buf, n, capacity, region, op, ptr):
    L = bm._lib.load()
    count = C.c_uint32(n)
    code = L.bm_host_write_region_supercell(G, G, 0, 0, 0, idx.ctypes.data, C.byref(count), buf.ctypes.data, capacity, region, op, C.c_void_p(ptr))
    return code, count.value


def test_writing_the_content_already_there_touches_nothing(bm, terrain):
    idx, bricks, vol = terrain
    # free slots in the arrays, so that any slot traffic would show
    i1, b1 = bm.host_edit_supercell(G, G, 0, 0, 0, idx, bricks, [bm.edit_box("clear", (0, 0, 0), (40, 40, G))])
    now = voxels_of(i1, b1)
    lo, hi = (5, 6, 7), (99, 100, 101)
    V = now[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].copy()
    idx2, buf = i1.copy(), np.zeros((4096, 16), np.uint32)
    buf[:len(b1)] = b1
    before = buf.copy()
    for op, vol_in in ((0, V), (bm.BM_EDIT_SET, V), (bm.BM_EDIT_CLEAR, 1 - V)):
        keep = np.ascontiguousarray(vol_in)
        r, ptr, _ = bm.region_of(lo, keep)
        code, n = raw_write(bm, idx2, buf, len(b1), 4096, C.byref(r), op, ptr)
        assert code == 0 and n == len(b1)
        assert idx2.tobytes() == i1.tobytes() and buf.tobytes() == before.tobytes()


def test_clipping(bm, terrain):
    idx, bricks, vol = terrain
    rng = np.random.default_rng(5)
    lo = (-5, -6, -7)
    V = (rng.random((G + 7 + 9, G + 6 + 10, G + 5 + 11)) < 0.3).astype(np.uint8)  # sticks out on both sides of every axis
    for op in ("replace", "set", "clear"):
        want = model_write(vol, lo, V, op)
        i2, b2 = bm.host_write_region_supercell(G, G, 0, 0, 0, idx, bricks, lo, V, op)
        assert np.array_equal(voxels_of(i2, b2), want)
    assert np.array_equal(model_write(vol, lo, V, "replace"), V[7:7 + G, 6:6 + G, 5:5 + G])
    small = np.ones((4, 4, 4), np.uint8)
    for outside in ((G, 0, 0), (0, -4, 0), (3, 3, G + 100), (-(2 ** 31), 5, 5), (2 ** 31 - 5, 5, 5)):
        i2, b2 = bm.host_write_region_supercell(G, G, 0, 0, 0, idx, bricks, outside, small, "replace")
        assert np.array_equal(i2, idx) and np.array_equal(b2, bricks)
    for shape in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):  # an empty box
        i2, b2 = bm.host_write_region_supercell(G, G, 0, 0, 0, idx, bricks, (8, 8, 8), np.ones(shape, np.uint8), "replace")
        assert np.array_equal(i2, idx) and np.array_equal(b2, bricks)


def test_one_supercell_of_a_box_that_spans_several(bm):
    size, height = 256, 128
    rng = np.random.default_rng(6)
    lo = (100, 90, 30)
    V = (rng.random((60, 70, 80)) < 0.5).astype(np.uint8)
    world = np.zeros((height, size, size), np.uint8)
    want = model_write(world, lo, V, "replace")
    for sx, sy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        idx, bricks = bm.host_write_region_supercell(size, height, sx, sy, 0, np.zeros(4096, np.uint32), np.zeros((0, 16), np.uint32), lo, V, "replace")
        got = voxels_of(idx, bricks, sx, sy, 0, size, height)
        part = np.zeros_like(want)
        part[:, sy * 128:sy * 128 + 128, sx * 128:sx * 128 + 128] = want[:, sy * 128:sy * 128 + 128, sx * 128:sx * 128 + 128]
        assert np.array_equal(got, part)
        words, canon = canonical_supercell(want, sx, sy, 0)
        assert np.array_equal(idx, words) and np.array_equal(bricks, canon)  # into an empty supercell: the canonical build


def test_a_sub_box_of_a_larger_array_equals_its_tight_copy(bm, terrain):
    idx, bricks, vol = terrain
    rng = np.random.default_rng(7)
    big = (rng.random((50, 60, 70)) < 0.5).astype(np.uint8)
    sub = big[5:38, 7:49, 11:52]
    assert not sub.flags["C_CONTIGUOUS"]
    lo = (13, 21, 30)
    for op in ("replace", "set", "clear"):
        a = bm.host_write_region_supercell(G, G, 0, 0, 0, idx, bricks, lo, sub, op)
        b = bm.host_write_region_supercell(G, G, 0, 0, 0, idx, bricks, lo, np.ascontiguousarray(sub), op)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(voxels_of(*a), model_write(vol, lo, sub, op))
    with pytest.raises(ValueError):
        bm.region_of(lo, big[:, :, ::2])
    with pytest.raises(ValueError):
        bm.region_of(lo, big.astype(np.float32))


def test_refusals_leave_the_arrays_unchanged(bm, terrain):
    idx, bricks, vol = terrain
    V = np.ones((8, 8, 8), np.uint8)
    idx2, buf = idx.copy(), np.zeros((4096, 16), np.uint32)
    buf[:len(bricks)] = bricks
    before = buf.copy()

    def region(lo, hi, row=0, sl=0):
        r = bm.bm_region()
        r.lo[:], r.hi[:] = lo, hi
        r.row_pitch, r.slice_pitch = row, sl
        return r

    ok = region((0, 0, 120), (8, 8, 128))  # sky: every cell it covers gains a brick
    cases = {
        "hi < lo on x": (region((8, 0, 120), (7, 8, 128)), 0, V.ctypes.data, 4096),
        "hi < lo on z": (region((0, 0, 120), (8, 8, 119)), 0, V.ctypes.data, 4096),
        "unknown op": (ok, 3, V.ctypes.data, 4096),
        "negative op": (ok, -1, V.ctypes.data, 4096),
        "null volume": (ok, 0, None, 4096),
        "row pitch below the row": (region((0, 0, 120), (8, 8, 128), row=7), 0, V.ctypes.data, 4096),
        "slice pitch below the slice": (region((0, 0, 120), (8, 8, 128), row=8, sl=63), 0, V.ctypes.data, 4096),
        "negative pitch": (region((0, 0, 120), (8, 8, 128), row=-8), 0, V.ctypes.data, 4096),
        "brick capacity too small": (ok, 0, V.ctypes.data, len(bricks)),
    }
    for name, (r, op, ptr, capacity) in cases.items():
        code, n = raw_write(bm, idx2, buf, len(bricks), capacity, C.byref(r), op, ptr)
        assert code == EINVAL, name
        assert n == len(bricks) and idx2.tobytes() == idx.tobytes() and buf.tobytes() == before.tobytes(), name
    code, n = raw_write(bm, idx2, buf, len(bricks), 4096, None, 0, V.ctypes.data)
    assert code == EINVAL and idx2.tobytes() == idx.tobytes()
    code, n = raw_write(bm, idx2, buf, len(bricks), 4096, C.byref(ok), 0, V.ctypes.data)  # and the valid call goes through
    assert code == 0 and n == len(bricks) + 1
