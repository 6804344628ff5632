"""What the case generators of tests/_box_cases.py cover (no GPU): the conditions that tests/test_gpu_region_edges.py and
tests/test_gpu_volume_edges.py rely on, so that a change of a seed, a world or a generator that loses one of them fails here; and the
numpy models those tests compare with, against voxel-by-voxel brute force on a tiny world."""
import numpy as np
import pytest

from _box_cases import (BIG_RECORDS, BIG_RUNS, BOX, HOLES, ROUTES, SOLID_CELLS, SPHERE, SWEEPS, WORLDS, Slab, axis_sweep, base_batch, big_batch, clipping_faces,
                        items_of, model_read, model_sweep, random_boxes, region_cases, run_boundaries, run_records, tall_sweeps, world_voxels, x_sweep,
                        zero_item_records)
from _edit_model import occupancy
from test_gpu_volume import model_results
from test_region_host import model_write


def clipped(dims, lo, hi):
    return [max(0, lo[k]) for k in range(3)], [min(dims[k], hi[k]) for k in range(3)]


@pytest.mark.parametrize("world", list(WORLDS))
def test_the_worlds(world):
    X, Y, Z = WORLDS[world]
    vox = world_voxels(world)
    assert vox.shape == (Z, Y, X) and X == Y and all(n % 128 == 0 for n in (X, Y, Z))
    assert 0.25 < vox.mean() < 0.32
    occ = occupancy(vox)
    (x0, x1), (y0, y1), (z0, z1) = HOLES[world]
    in_hole = [c for c in SOLID_CELLS[world] if x0 <= 8 * c[0] < x1 and y0 <= 8 * c[1] < y1 and z0 <= 8 * c[2] < z1]  # (the tall world's shaft holds two)
    assert all(v % 8 == 0 for v in (x0, x1, y0, y1, z0, z1)) and occ[z0 // 8:z1 // 8, y0 // 8:y1 // 8, x0 // 8:x1 // 8].sum() == len(in_hole)
    assert (~occ).sum() == (x1 - x0) * (y1 - y0) * (z1 - z0) // 512 - len(in_hole) >= 500, "the hole's cells are empty and no other cell is"
    full = vox.reshape(Z // 8, 8, Y // 8, 8, X // 8, 8).all(axis=(1, 3, 5))
    assert full.sum() == len(SOLID_CELLS[world]) >= 3


@pytest.mark.parametrize("world", list(WORLDS))
def test_x_sweep_covers_every_chunk_residue(world):
    dims = WORLDS[world]
    general, aligned = x_sweep(dims, "general"), x_sweep(dims, "aligned")
    assert {(lo[0] % 16, hi[0] % 16) for lo, hi in general} == {(a, b) for a in range(16) for b in range(16)}
    assert {(lo[0] % 16, hi[0] % 16) for lo, hi in aligned} == {(0, b) for b in range(16)}
    assert {lo[0] for lo, hi in aligned} >= {-32, -16, 0}, "boxes whose clipped lo.x differs from the volume's origin"
    for cases in (general, aligned):
        assert all(hi[0] > max(lo[0], 0) and lo[0] < dims[0] for lo, hi in cases), "every box keeps a part inside the world"
        assert any(lo[0] >= 0 and lo[0] // 16 == (hi[0] - 1) // 16 for lo, hi in cases), "a box inside one 16-byte chunk"
        assert any(lo[0] >= 0 and lo[0] // 8 == (hi[0] - 1) // 8 for lo, hi in cases), "a box inside one brick cell"
        assert any(hi[0] == 128 for lo, hi in cases), "a box that ends on the run boundary"
        assert any(lo[0] < 128 and hi[0] - lo[0] >= 48 and hi[0] > 128 for lo, hi in cases), "a box across x = 128 with whole chunks inside"
        for B in run_boundaries(dims[0]):
            assert sum(lo[0] < B < hi[0] for lo, hi in cases) >= 16 and any(hi[0] == B for lo, hi in cases), f"boxes across and onto x = {B}"
        for lo, hi in cases:
            assert (lo[1] % 8, hi[1] % 8, lo[2] % 8, hi[2] % 8) == (3, 6, 3, 5), "y and z stand at residues that are not 0"
    for b in range(16):  # aligned: each hi residue with a partial last chunk alone, behind whole chunks, and behind a clipped origin
        assert any(hi[0] % 16 == b and hi[0] - lo[0] <= 16 for lo, hi in aligned) and any(hi[0] % 16 == b and hi[0] - max(lo[0], 0) > 32 for lo, hi in aligned)
        assert any(hi[0] % 16 == b and lo[0] < 0 for lo, hi in aligned)


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("world", list(WORLDS))
def test_y_and_z_sweeps_cover_every_cell_residue(world, route, axis):
    dims = WORLDS[world]
    cases = axis_sweep(dims, route, axis)
    assert {(lo[axis] % 8, hi[axis] % 8) for lo, hi in cases} == {(a, b) for a in range(8) for b in range(8)}
    thin = [(lo, hi) for lo, hi in cases if lo[axis] // 8 == (hi[axis] - 1) // 8]
    assert len(thin) >= 36 and any(hi[axis] - lo[axis] == 8 for lo, hi in thin) and any(hi[axis] - lo[axis] == 1 for lo, hi in thin), "boxes one cell thick"
    for B in run_boundaries(dims[axis]):
        assert sum(lo[axis] < B < hi[axis] for lo, hi in cases) >= 64, f"boxes across the supercell boundary at {B}"
    assert all(0 <= lo[k] < hi[k] <= dims[k] for lo, hi in cases for k in (1, 2))
    other = 3 - axis
    assert all((lo[other] % 8, hi[other] % 8) in ((3, 6), (3, 5)) for lo, hi in cases)
    if dims[0] > 128:
        assert all(lo[0] < 128 < hi[0] for lo, hi in cases), "the boxes cross x = 128"
    if route == "general":
        assert all(lo[0] % 16 and hi[0] % 16 for lo, hi in cases)


def test_supercell_boundaries_of_each_world():
    assert {w: [run_boundaries(n) for n in d] for w, d in WORLDS.items()} == {
        "flat": [[128, 256], [128, 256], []], "tall": [[], [], [128, 256]], "cube": [[128], [128], [128]]}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("world", list(WORLDS))
def test_random_boxes(world, route):
    dims = WORLDS[world]
    cases = region_cases(world, route, "random")
    boxes, outside, around = cases[:-2], cases[-2], cases[-1]
    assert len(boxes) >= 300
    faces = [clipping_faces(dims, lo, hi) for lo, hi in boxes]
    assert all(hi[k] > max(lo[k], 0) and lo[k] < dims[k] for lo, hi in boxes for k in range(3)), "every box keeps a part inside the world"
    assert set().union(*faces) == set(range(6)), "every face clips a box"
    assert all(sum(f == {k} for f in faces) >= 10 for k in range(6))
    assert 0.3 <= sum(bool(f) for f in faces) / len(boxes) <= 0.4, "about a third of the boxes are clipped"
    assert clipping_faces(dims, *outside) == set() and any(outside[0][k] >= dims[k] for k in range(3)), "a box wholly outside"
    assert clipping_faces(dims, *around) == set(range(6)), "a box that contains the world"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("world", list(WORLDS))
def test_cases_fit_the_slab_and_the_route(world, route):
    for sweep in SWEEPS:
        cases = region_cases(world, route, sweep)
        big = [c for c in cases if any(h - l > m for l, h, m in zip(c[0], c[1], Slab.CASE[::-1]))]
        assert len(big) == (1 if sweep == "random" else 0), "only the box round the world is larger than the slab's ordinary case"
        for lo, hi in cases:
            assert all(h > l for l, h in zip(lo, hi))
            if route == "aligned":  # (a box one row thick has its length as row pitch)
                assert lo[0] % 16 == 0 and (hi[1] - lo[1] > 1 or (hi[0] - lo[0]) % 16 == 0), (lo, hi)


def test_the_streaming_sweeps_stand_at_the_holes_wall():
    """in the cubic and the flat world the x, y and z sweeps (around the first boundary) lie in front of the hole's -x wall, between its
    other walls, and reach from the wall's cells to cells three and more cells behind it: cells that a camera inside the hole loads,
    and cells that it does not"""
    for world in ("cube", "flat"):
        dims = WORLDS[world]
        (x0, x1), (y0, y1), (z0, z1) = HOLES[world]
        for route in ROUTES:
            for sweep in ("x", "y", "z"):
                cases = [c for c in region_cases(world, route, sweep) if all(c[1][k] <= 192 for k in range(3))]
                assert len(cases) >= 128
                for lo, hi in cases:
                    lo, hi = clipped(dims, lo, hi)
                    assert y0 <= lo[1] and hi[1] <= y1 and z0 <= lo[2] and hi[2] <= z1 and hi[0] <= x1, (world, route, sweep, lo, hi)
                assert sum(x0 - hi[0] < 16 for lo, hi in cases) * 4 >= len(cases) and sum(lo[0] < x0 - 24 for lo, hi in cases) * 4 >= len(cases)


def test_layout_of_the_big_volume_batch(bm):
    dims = WORLDS["cube"]
    base, zero = base_batch(bm), zero_item_records(bm, dims)
    assert len(base) == 4099 and len(base) % 256 != 0 and items_of(base[:1], dims)[0] > 0
    assert (items_of(zero, dims) == 0).all() and len(zero) == 7
    kinds = items_of(base, dims)
    assert (kinds == 0).sum() > 200 and (kinds == 1).sum() > 1000 and (kinds > 16).sum() > 10 and (base["shape"] == SPHERE).sum() > 500
    assert tuple(base["hi"][(base["shape"] == BOX) & (base["lo"] == 0).all(1)].max(0)) == dims, "the whole world is one of the records"
    blank = np.zeros(len(base), bm.VOLUME_RESULT_DTYPE), np.zeros(len(zero), bm.VOLUME_RESULT_DTYPE)
    for empty_tail in (False, True):
        recs, _ = big_batch(bm, base, blank[0], zero, blank[1], empty_tail)
        n = len(recs)
        nblocks = (n + 255) // 256
        assert n == BIG_RECORDS == 3 * 65536 + 77 and nblocks == 769
        per = (nblocks + 255) // 256
        assert per == 4 and 255 * per >= nblocks, "each thread of volume_scan owns 4 workgroups and the last ones none"
        per_block = np.add.reduceat(items_of(recs, dims), np.arange(0, n, 256))
        empty = np.nonzero(per_block == 0)[0].tolist()
        assert empty == [0, 300, 301, 302, 511, 767] + ([768] if empty_tail else [])
        assert [w for w, k in BIG_RUNS for _ in range(k)] == [0, 300, 300, 300, 511, 767]
        assert n - 256 * 768 == 77


def test_run_records_cover_the_run_boundaries(bm):
    for world in ("cube", "flat"):
        dims = WORLDS[world]
        recs = run_records(bm, dims)
        box, ball = recs[0::2], recs[1::2]
        assert (box["shape"] == BOX).all() and (ball["shape"] == SPHERE).all()
        lo, hi = box["lo"][:, 0], box["hi"][:, 0]
        for B in run_boundaries(dims[0]):
            near = (lo >= B - 8) & (lo <= B + 8)
            assert set((lo[near] % 8).tolist()) == set(range(8)) and set((hi[near] % 8).tolist()) == set(range(8))
            assert ((lo < B) & (hi == B)).sum() >= 10, "boxes that end on the run boundary"
        assert {0, 1, 63, 64, 126, 127} <= set((lo % 128).tolist()) and {0, 1, 127} <= set((hi % 128).tolist())
        items = items_of(box, dims)
        assert {1, 2, 4, 5} <= set(items.tolist()) and items.max() >= 2 * 5
        assert (ball["center"][:, 0] + ball["radius"] + 1 == hi).all(), "the sphere ends where its box ends"
        same = ball["center"][:, 0] - ball["radius"] == lo
        assert same.sum() > 100 and (items_of(ball, dims) > 0).all()


def test_tall_sweeps_pass_the_supercell_boundaries():
    vox = world_voxels("tall")
    lo, hi, sign, dist = tall_sweeps()
    want = model_sweep(vox, lo, hi, np.full(len(lo), 2), sign, dist)
    a, b = np.where(sign > 0, lo[:, 2], lo[:, 2] - want), np.where(sign > 0, hi[:, 2] + want, hi[:, 2])
    moved = want > 0
    assert len(lo) >= 300 and all((moved & (a < p) & (b > p)).sum() >= 20 for p in (128, 256)) and (moved & (b > 384)).sum() >= 20
    assert ((want < dist) & moved).sum() >= 20 and (want == 0).sum() >= 20


# ---------------------------------------------------------------- the models against brute force
def test_models_agree_with_brute_force_on_a_tiny_world(bm):
    rng = np.random.default_rng(5)
    X, Y, Z = 24, 16, 8
    vol = (rng.random((Z, Y, X)) < 0.4).astype(np.uint8)
    for lo, shape in (((3, 2, 1), (4, 5, 6)), ((-2, 10, -3), (7, 9, 8)), ((20, -1, 5), (6, 4, 9)), ((30, 0, 0), (2, 2, 2)), ((-3, -3, -3), (14, 22, 30))):
        V = (rng.random(shape) < 0.5).astype(np.uint8) * 7
        hi = tuple(l + n for l, n in zip(lo, shape[::-1]))
        read = np.zeros(shape, np.uint8)
        written = {op: vol.copy() for op in ("replace", "set", "clear")}
        for k in range(shape[0]):
            for j in range(shape[1]):
                for i in range(shape[2]):
                    x, y, z = lo[0] + i, lo[1] + j, lo[2] + k
                    if 0 <= x < X and 0 <= y < Y and 0 <= z < Z:
                        read[k, j, i] = vol[z, y, x]
                        s = V[k, j, i] != 0
                        written["replace"][z, y, x] = s
                        written["set"][z, y, x] |= s
                        written["clear"][z, y, x] &= not s
        assert np.array_equal(model_read(vol, lo, hi), read)
        for op, want in written.items():
            assert np.array_equal(model_write(vol, lo, V, op), want), op
    # volume results: count, bounds and unresolved cells of boxes and spheres, voxel by voxel
    vol = (rng.random((16, 16, 16)) < 0.3).astype(np.uint8)
    vol[8:16, 0:8, 0:8] = 0
    resident = rng.random((2, 2, 2)) < 0.5
    recs = np.concatenate([bm.volume_box([(1, 2, 3), (-4, 5, 6), (0, 0, 0), (9, 9, 9), (3, 3, 3), (0, 0, 8)], [(9, 12, 8), (3, 30, 9), (16, 16, 16), (9, 12, 12), (2, 5, 5), (8, 8, 16)]),
                           bm.volume_sphere([(8, 8, 8), (-2, 3, 17), (4, 4, 4), (40, 4, 4), (3, 3, 3)], [5, 6, 0, 3, -1])])
    for res in (None, resident):
        got = model_results(bm, vol, recs, res)
        for i, rec in enumerate(recs):
            if i in (4, 10):
                assert got["status"][i] == 1 and got["solid"][i] == 0
                continue
            inside = np.zeros(vol.shape, bool)
            for z in range(16):
                for y in range(16):
                    for x in range(16):
                        if rec["shape"] == BOX:
                            inside[z, y, x] = all(rec["lo"][k] <= v < rec["hi"][k] for k, v in enumerate((x, y, z)))
                        else:
                            inside[z, y, x] = sum((int(v) - int(rec["center"][k])) ** 2 for k, v in enumerate((x, y, z))) <= int(rec["radius"]) ** 2
            seen = inside & (vol != 0) & (True if res is None else np.kron(res, np.ones((8, 8, 8), bool)).astype(bool))
            assert got["status"][i] == 0 and got["solid"][i] == seen.sum(), i
            if seen.any():
                zs, ys, xs = np.nonzero(seen)
                assert tuple(got["lo"][i]) == (xs.min(), ys.min(), zs.min()) and tuple(got["hi"][i]) == (xs.max() + 1, ys.max() + 1, zs.max() + 1), i
            else:
                assert tuple(got["lo"][i]) == tuple(got["hi"][i]) == (-1, -1, -1)
            want_unres = 0 if res is None else int((occupancy(inside) & occupancy(vol) & ~res).sum())
            assert got["unresolved"][i] == want_unres, i
            # the work items: one per run of 128 voxels, cell row and cell slice of the clipped bounding box
            if rec["shape"] == BOX:
                a, b = np.clip(rec["lo"], 0, 16), np.clip(rec["hi"], 0, 16)
            else:
                a, b = np.clip(rec["center"] - rec["radius"], 0, 16), np.clip(rec["center"] + rec["radius"] + 1, 0, 16)
            cells = {(x >> 7, y >> 3, z >> 3) for x in range(a[0], b[0]) for y in range(a[1], b[1]) for z in range(a[2], b[2])}
            assert items_of(recs[i:i + 1], (16, 16, 16))[0] == len(cells), i
