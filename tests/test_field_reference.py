"""CPU tests of tests/_edit_model.py::reference_field, the cube-field reference of the GPU edit tests, and through it of the host build
(World::build_cube_field): every byte of a generated world's field, a brute-force loop over a random occupancy, and the cap at 254 on a
grid wide enough to reach it."""
import numpy as np

from _edit_model import reference_field, update_box


def brute_force(occ, x, y, z, o):
    """the loop of test_jump.py::test_cube_field_matches_bruteforce: the largest cube of empty in-grid cells anchored at (x, y, z)"""
    nz, ny, nx = occ.shape
    dx, dy, dz = (-1 if o & 1 else 1), (-1 if o & 2 else 1), (-1 if o & 4 else 1)
    e = 0
    while True:
        m = e + 1
        xs = sorted((x, x + dx * (m - 1)))
        ys = sorted((y, y + dy * (m - 1)))
        zs = sorted((z, z + dz * (m - 1)))
        if xs[0] < 0 or ys[0] < 0 or zs[0] < 0 or xs[1] >= nx or ys[1] >= ny or zs[1] >= nz:
            break
        if occ[zs[0]:zs[1] + 1, ys[0]:ys[1] + 1, xs[0]:xs[1] + 1].any():
            break
        e = m
    return min(e, 254)


def test_reference_equals_the_host_build_at_every_byte(bm):
    G = 256
    occ = np.zeros((32, 32, 32), bool)
    for sc in range(8):
        sx, sy, sz = sc & 1, (sc >> 1) & 1, sc >> 2
        words, _ = bm.host_generate_supercell(G, G, sx, sy, sz)
        occ[sz * 16:sz * 16 + 16, sy * 16:sy * 16 + 16, sx * 16:sx * 16 + 16] = (words != 0).reshape(16, 16, 16)
    assert 0 < occ.sum() < occ.size
    want = reference_field(occ)
    got = bm.host_cube_field(G, G)
    assert got.shape == want.shape == (8, 34, 34, 34)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {got.size} field bytes differ"
    # the sampling form gives the same values
    rng = np.random.default_rng(0)
    cells = rng.integers(0, 32, (500, 3))
    assert np.array_equal(reference_field(occ, cells), want[:, cells[:, 2] + 1, cells[:, 1] + 1, cells[:, 0] + 1])


def test_reference_equals_the_brute_force_loop():
    rng = np.random.default_rng(20)
    n = 20
    occ = rng.random((n, n, n)) < 0.02
    assert 100 < occ.sum() < 250
    field = reference_field(occ)
    border = np.ones(field.shape[1:], bool)
    border[1:-1, 1:-1, 1:-1] = False
    for o in range(8):
        assert (field[o][border] == 255).all()
        inner = field[o, 1:-1, 1:-1, 1:-1]
        assert np.array_equal(inner == 0, occ)
        want = np.zeros((n, n, n), np.uint8)
        for z in range(n):
            for y in range(n):
                for x in range(n):
                    want[z, y, x] = 0 if occ[z, y, x] else brute_force(occ, x, y, z, o)
        assert np.array_equal(inner, want), f"octant {o}: {np.count_nonzero(inner != want)} cells differ"
    assert field[:, 1:-1, 1:-1, 1:-1].max() > 5  # cubes of some size exist


def test_the_cap_at_254_and_the_border_value():
    n = 300
    occ = np.zeros((n, n, n), bool)
    p = n - 1
    occ[p, p, p] = True  # the far corner: along +x +y +z the uncapped value of cell (c, c, c) is p - c, the distance to it
    # cells on the diagonal whose uncapped value is 253, 254, 255 and 299
    diag = np.array([[p - 253] * 3, [p - 254] * 3, [p - 255] * 3, [p - 299] * 3])
    assert np.array_equal(reference_field(occ, diag)[0], [253, 254, 254, 254])
    # off the diagonal the cube may pass the occupied cell: the grid's far faces limit it instead (n - coordinate)
    off = np.array([[p - 253, 10, 10], [10, p - 254, 10], [10, 10, p - 255], [0, 0, 1]])
    assert np.array_equal(reference_field(occ, off)[0], [254, 254, 254, 254])
    near = np.array([[p - 253, p - 100, p - 100], [p - 1, p - 1, p - 1], [p, p, p], [p - 1, p, p]])
    assert np.array_equal(reference_field(occ, near)[0], [101, 1, 0, 1])  # the first: 101 cells to the far y and z faces
    # along -x -y -z the corner cell is never in the way: the value is the distance to the near faces, coordinate + 1
    assert np.array_equal(reference_field(occ, diag)[7], [p - 253 + 1, p - 254 + 1, p - 255 + 1, 1])
    assert np.array_equal(reference_field(occ, np.array([[252, 260, 270], [253, 260, 270], [254, 299, 299], [298, 298, 298]]))[7], [253, 254, 254, 254])
    # no interior value is 255, whatever the octant: the three planes through the occupied cell, the planes through the grid's centre
    # and near faces, and 300 000 random cells
    rng = np.random.default_rng(254)
    g = np.arange(n)
    parts = [rng.integers(0, n, (300_000, 3))]
    for axis in range(3):
        for v in (0, 1, 45, 46, 150, 253, 254, 255, p - 1, p):
            grid = [g, g, g]
            grid[axis] = np.array([v])
            parts.append(np.stack([a.reshape(-1) for a in np.meshgrid(*grid, indexing="ij")], 1))
    cells = np.concatenate(parts)
    values = reference_field(occ, cells)
    assert values.max() == 254 and (values == 254).sum() > 1000
    occupied = (cells == p).all(1)
    assert occupied.any() and (values[:, occupied] == 0).all() and (values[:, ~occupied] > 0).all()


def test_update_box_formula():
    """the box of scene.cpp's field_update_box, in bordered coordinates, for cases worked out by hand"""
    b = update_box([[256, 256, 8]], 512, 16)
    assert (b["rx0"], b["rx1"], b["ry0"], b["ry1"], b["rz0"], b["rz1"]) == (3, 512, 3, 512, 1, 17)
    assert (b["ay0"], b["ay1"], b["bz0"], b["bz1"]) == (1, 513, 1, 17)
    b = update_box([[0, 0, 0], [300, 2, 0]], 512, 16)
    assert (b["rx0"], b["rx1"], b["ry0"], b["ry1"]) == (1, 513, 1, 258) and (b["ay0"], b["ay1"]) == (1, 512)
    b = update_box([[5, 5, 5]], 272, 272)
    assert (b["rx0"], b["rx1"], b["rz0"], b["rz1"], b["bz0"], b["bz1"]) == (1, 261, 1, 261, 1, 273)


def test_field_update_plans_reach_what_they_are_for():
    """The batches of tests/test_gpu_edit_device.py's field cases, on the model alone: every update box is partial where its case says
    (FieldModel.apply asserts it), the cubic world keeps cubes of 254 cells, and the scratch buffer of the growth case grows."""
    from _edit_model import (CUBIC_CELLS, FieldModel, cubic_field_plan, field_update_tmp_bytes, flat_field_plan, scratch_growth_plan, tall_field_plan)
    for cells in (512, 272):
        m = FieldModel(cells, 16)
        for name, ops, want in flat_field_plan(cells):
            if ops:
                m.apply(ops, want)
        assert not m.occ.any()
        m = FieldModel(cells, 16)
        sizes = [field_update_tmp_bytes(m.apply(ops, want)[1]) for _, ops, want in scratch_growth_plan(cells)]
        assert sizes[0] < sizes[1] > sizes[2]
    m = FieldModel(16, 512)
    for name, ops, want in tall_field_plan():
        if ops:
            m.apply(ops, want)
    assert not m.occ.any()
    m = FieldModel(CUBIC_CELLS, CUBIC_CELLS)
    for name, ops, want in cubic_field_plan():
        m.apply(ops, want)
    assert m.occ.sum() == 2 and m.occ[5, 5, 5] and m.occ[266, 266, 266]
    assert reference_field(m.occ, [[6, 0, 0]])[0, 0] == 254  # a cube of 254 cells that avoids both voxels


def test_random_edit_plan_frees_reuses_and_grows(bm):
    """The randomised batches of the device-world test, on the model alone: whole bricks empty (at least 100 device slots are freed),
    a brick appears in a supercell that has a freed slot (reuse), and a supercell ends up with more bricks than it was built with (a
    preloaded pool is an exact fit, so it must grow)."""
    from _edit_model import apply_to_model, occupancy, random_batches
    from _load_model import expand_supercell
    G = 256
    vol = np.zeros((G, G, G), np.uint8)
    for sc in range(8):
        sx, sy, sz = sc & 1, (sc >> 1) & 1, sc >> 2
        expand_supercell(vol, sx, sy, sz, *bm.host_generate_supercell(G, G, sx, sy, sz))
    vol = vol != 0
    batches = random_batches()
    assert len(batches) >= 30 and all(1 <= len(b) <= 4 for b in batches)
    kinds = {e[0] for b in batches for e in b}
    assert kinds == {"box", "sphere", "voxels"}

    def per_supercell(occ):
        return occ.reshape(2, 16, 2, 16, 2, 16).transpose(0, 2, 4, 1, 3, 5).reshape(8, -1)
    occ = per_supercell(occupancy(vol))
    built = occ.sum(1)
    free = np.zeros(8, int)
    freed = reused = 0
    peak = built.copy()
    for batch in batches:
        apply_to_model(vol, batch)
        now = per_supercell(occupancy(vol))
        gone, new = (occ & ~now).sum(1), (~occ & now).sum(1)
        freed += gone.sum()
        free += gone
        take = np.minimum(free, new)
        reused += take.sum()
        free -= take
        peak = np.maximum(peak, now.sum(1))
        occ = now
    assert freed >= 100 and reused >= 1 and (peak > built).any(), (freed, reused, peak - built)
