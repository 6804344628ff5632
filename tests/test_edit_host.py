"""Voxel edits, host half (bm_host_edit_supercell; CPU only): bits, LoD masks, index words and slot reuse of an edited supercell,
checked against a numpy model of the supercell's 128^3 voxels."""
import ctypes as C

import numpy as np
import pytest

G, H = 256, 256  # world; supercell (1, 0, 0) holds terrain surface
SC = (1, 0, 0)
ORG = np.array(SC) * 128


def voxels(idx, bricks):
    """the supercell's voxels, [z, y, x] bool, from its index words and bricks (bit = x + 8y + 64z in a brick, Scene.cpp:91-93)"""
    v = np.zeros((128, 128, 128), bool)
    for cell in np.nonzero(idx)[0]:
        bits = np.unpackbits(bricks[idx[cell] & 0xFFF].view(np.uint8), bitorder="little").reshape(8, 8, 8).astype(bool)
        bx, by, bz = cell & 15, (cell >> 4) & 15, cell >> 8
        v[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = bits
    return v


def check_consistent(idx, bricks, want):
    """the arrays are what the generator would store for the voxels `want`: a brick exactly where a cell has voxels, word =
    slot | loaded | lod << 12 with the LoD mask of its bits, distinct slots below 4096"""
    assert len(bricks) <= 4096
    cells = want.reshape(16, 8, 16, 8, 16, 8).transpose(0, 2, 4, 1, 3, 5)  # [bz, by, bx, z, y, x]
    solid = cells.reshape(16, 16, 16, -1).any(-1).reshape(-1)
    assert np.array_equal(idx != 0, solid), "a brick where there are no voxels, or none where there are"
    live = idx[idx != 0]
    assert np.all(live & 0x80000000) and not np.any(live & 0x70000000)
    assert len(np.unique(live & 0xFFF)) == len(live), "two cells share a slot"
    assert np.all((live & 0xFFF) < len(bricks))
    assert np.array_equal(voxels(idx, bricks), want)
    # LoD mask: octant q = (x >= 4) + 2 (y >= 4) + 4 (z >= 4) of the brick holds a voxel (Scene.cpp:95)
    q = cells.reshape(16, 16, 16, 2, 4, 2, 4, 2, 4).any(axis=(4, 6, 8))  # [bz, by, bx, qz, qy, qx]
    lod = (q.reshape(4096, 8).astype(np.uint32) * (1 << np.arange(8, dtype=np.uint32))).sum(-1)  # bit order qz qy qx -> 4 qz + 2 qy + qx
    assert np.array_equal((idx >> 12) & 0xFF, np.where(solid, lod, 0).astype(np.uint32))


def model(want, op, lo=None, hi=None, center=None, radius=None):
    """apply one edit to the numpy model (global voxel coordinates)"""
    z, y, x = np.meshgrid(*(np.arange(128) + ORG[k] for k in (2, 1, 0)), indexing="ij")
    if lo is not None:
        m = (x >= lo[0]) & (x < hi[0]) & (y >= lo[1]) & (y < hi[1]) & (z >= lo[2]) & (z < hi[2])
    else:
        c = [np.int64(v) for v in center]
        m = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= np.int64(radius) ** 2
    want = want.copy()
    want[m] = op == "set"
    return want


@pytest.fixture(scope="module")
def sc(bm):
    idx, bricks = bm.host_generate_supercell(G, H, *SC)
    check_consistent(idx, bricks, voxels(idx, bricks))
    return idx, bricks


def test_generated_supercell_is_consistent_with_the_model(sc):
    idx, bricks = sc
    assert np.count_nonzero(idx) == len(bricks) > 0


def test_box_sphere_and_voxel_edits_match_the_model(bm, sc):
    idx, bricks = sc
    want = voxels(idx, bricks)
    steps = [
        (bm.edit_box("clear", (130, 5, 60), (170, 47, 140)), dict(op="clear", lo=(130, 5, 60), hi=(170, 47, 140))),
        (bm.edit_sphere("set", (200, 64, 200), 17), dict(op="set", center=(200, 64, 200), radius=17)),
        (bm.edit_sphere("clear", (128, 0, 100), 40), dict(op="clear", center=(128, 0, 100), radius=40)),  # crosses the supercell's border
        (bm.edit_box("set", (250, 120, 250), (300, 300, 300)), dict(op="set", lo=(250, 120, 250), hi=(300, 300, 300))),  # clipped by the world
        (bm.edit_box("set", (140, 30, 230), (141, 31, 231)), dict(op="set", lo=(140, 30, 230), hi=(141, 31, 231))),  # one voxel in the sky
        (bm.edit_box("clear", (150, 20, 90), (151, 21, 91)), dict(op="clear", lo=(150, 20, 90), hi=(151, 21, 91))),
    ]
    for e, m in steps:
        idx, bricks = bm.host_edit_supercell(G, H, *SC, idx, bricks, [e])
        want = model(want, **m)
        check_consistent(idx, bricks, want)
    # a batch applies in order: set then clear of the same box leaves it empty, clear then set leaves it solid
    idx2, bricks2 = bm.host_edit_supercell(G, H, *SC, idx, bricks, [bm.edit_box("set", (129, 1, 1), (140, 9, 9)), bm.edit_box("clear", (129, 1, 1), (140, 9, 9))])
    check_consistent(idx2, bricks2, model(want, "clear", lo=(129, 1, 1), hi=(140, 9, 9)))
    idx3, bricks3 = bm.host_edit_supercell(G, H, *SC, idx, bricks, [bm.edit_box("clear", (129, 1, 1), (140, 9, 9)), bm.edit_box("set", (129, 1, 1), (140, 9, 9))])
    check_consistent(idx3, bricks3, model(want, "set", lo=(129, 1, 1), hi=(140, 9, 9)))


def test_emptied_brick_gets_word_zero_and_its_slot_is_reused(bm, sc):
    idx, bricks = sc
    cell = int(np.nonzero(idx)[0][10])
    slot = int(idx[cell] & 0xFFF)
    bx, by, bz = cell & 15, (cell >> 4) & 15, cell >> 8
    lo = ORG + np.array([bx, by, bz]) * 8
    i2, b2 = bm.host_edit_supercell(G, H, *SC, idx, bricks, [bm.edit_box("clear", lo, lo + 8)])
    assert i2[cell] == 0 and len(b2) == len(bricks)
    # the next brick that appears takes the freed slot instead of a new one
    sky = int(np.nonzero(i2 == 0)[0][-1])
    sx_, sy_, sz_ = sky & 15, (sky >> 4) & 15, sky >> 8
    p = ORG + np.array([sx_, sy_, sz_]) * 8
    i3, b3 = bm.host_edit_supercell(G, H, *SC, i2, b2, [bm.edit_box("set", p, p + 1)])
    assert len(b3) == len(b2) and (i3[sky] & 0xFFF) == slot and (i3[sky] >> 12) & 0xFF == 1


def test_slots_stay_below_4096_under_remove_add_cycles(bm, sc):
    idx, bricks = sc
    base = voxels(idx, bricks)
    rng = np.random.default_rng(7)
    # 20000 edits, alternately clearing and filling whole bricks at random cells, in batches
    edits, want = [], base.copy()
    for k in range(20000):
        c = rng.integers(0, 16, 3)
        lo = ORG + c * 8
        op = "clear" if k % 2 == 0 else "set"
        edits.append(bm.edit_box(op, lo, lo + 8))
        want[c[2] * 8:c[2] * 8 + 8, c[1] * 8:c[1] * 8 + 8, c[0] * 8:c[0] * 8 + 8] = op == "set"
        if len(edits) == 500:
            idx, bricks = bm.host_edit_supercell(G, H, *SC, idx, bricks, edits)
            assert len(bricks) <= 4096  # ~10000 new bricks in all: without slot reuse the slots would pass 4095
            edits = []
    check_consistent(idx, bricks, want)


@pytest.mark.parametrize("bad", [
    dict(op=3, shape=1, lo=(0, 0, 0), hi=(1, 1, 1)),
    dict(op=1, shape=7, lo=(0, 0, 0), hi=(1, 1, 1)),
    dict(op=1, shape=1, lo=(5, 0, 0), hi=(4, 1, 1)),
    dict(op=2, shape=2, center=(5, 5, 5), radius=-1),
    dict(op=0, shape=1, lo=(0, 0, 0), hi=(1, 1, 1)),
])
def test_bad_edits_are_refused_and_change_nothing(bm, sc, bad):
    from brickmap_amd import _lib
    idx, bricks = sc
    e = _lib.bm_edit()
    e.op, e.shape = bad["op"], bad["shape"]
    if "lo" in bad:
        e.lo[:], e.hi[:] = bad["lo"], bad["hi"]
    else:
        e.center[:], e.radius = bad["center"], bad["radius"]
    good = bm.edit_box("clear", (128, 0, 0), (256, 128, 128))  # would change everything: the batch is checked before anything applies
    L = _lib.load()
    i = idx.copy()
    n = C.c_uint32(len(bricks))
    buf = np.zeros((4096, 16), np.uint32)
    buf[:len(bricks)] = bricks
    before = buf.copy()
    arr = (_lib.bm_edit * 2)(good, e)
    assert L.bm_host_edit_supercell(G, H, *SC, i.ctypes.data, C.byref(n), buf.ctypes.data, 4096, 2, arr) == 10001  # BM_EINVAL
    assert np.array_equal(i, idx) and n.value == len(bricks) and np.array_equal(buf, before)
    with pytest.raises(bm.BrickmapError):
        bm.host_edit_supercell(G, H, *SC, idx, bricks, [good, e])


def test_noop_batches_change_nothing(bm, sc):
    idx, bricks = sc
    for edits in ([], [bm.edit_box("set", (-50, -50, -50), (-1, 10, 10))], [bm.edit_sphere("clear", (10 ** 9, 0, 0), 1000)],
                  [bm.edit_box("set", (130, 3, 3), (130, 9, 9))],  # empty box (hi == lo on x)
                  [bm.edit_box("clear", (0, 0, 0), (128, 128, 128))]):  # another supercell
        i2, b2 = bm.host_edit_supercell(G, H, *SC, idx, bricks, edits)
        assert np.array_equal(i2, idx) and np.array_equal(b2, bricks)


def test_sphere_far_from_the_world_with_huge_radius_is_exact(bm, sc):
    # the sum of squares needs more than 64 bits here; the membership test must still be exact (all of the supercell is inside)
    idx, bricks = sc
    big = 2 ** 31 - 1
    i2, b2 = bm.host_edit_supercell(G, H, *SC, idx, bricks, [bm.edit_sphere("clear", (-big, -big, -big), big)])
    assert np.array_equal(i2, idx)  # the closest voxel is farther than the radius: nothing cleared
    i3, b3 = bm.host_edit_supercell(G, H, *SC, idx, bricks, [bm.edit_sphere("set", (192, 64, -2 ** 30), 2 ** 30 + 200)])
    check_consistent(i3, b3, model(voxels(idx, bricks), "set", center=(192, 64, -2 ** 30), radius=2 ** 30 + 200))
