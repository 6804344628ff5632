"""Helpers of the edit tests (no tests here): a reference for the octant cube field written from its definition, the box of the field
that Scene::edit recomputes for a batch, and an exhaustive check of the device world (index words, bricks, LoD masks, slots, flags)
against a numpy model of the voxels."""
import numpy as np

from _load_model import canonical_supercell

LOADED, UNLOADED, REQUESTED = 0x80000000, 0x40000000, 0x20000000
FIELD_CAP = 254   # largest cube edge the field stores; 255 marks the border shell
FIELD_REACH = 254  # cells by which Scene::edit grows the changed cells' bounding box (scene.cpp field_update_box)


# ---------------------------------------------------------------- the cube field, from its definition
def reference_field(occ, cells=None):
    """The octant cube field of the occupancy `occ` (bool [z, y, x] of brick cells).  Value at an empty cell, plane o: the edge of the
    largest cube of empty in-grid cells anchored at the cell and extending along -x if o & 1 else +x, -y if o & 2 else +y, -z if o & 4
    else +z, capped at 254; 0 at an occupied cell.  Without `cells`: uint8 [8, Z + 2, Y + 2, X + 2] with the border shell at 255 (the
    layout of Scene.device_cube_field()).  With `cells` (N x 3 integer cell coordinates x, y, z): uint8 [8, N], the values there.

    By a summed-area table of `occ` and a bisection on the edge: "the cube of edge n lies in the grid and is empty" is monotone in n."""
    occ = np.asarray(occ) != 0
    Z, Y, X = occ.shape
    sat = np.zeros((Z + 1, Y + 1, X + 1), np.int32)
    sat[1:, 1:, 1:] = occ.astype(np.int32).cumsum(0, dtype=np.int32).cumsum(1, dtype=np.int32).cumsum(2, dtype=np.int32)
    flat = sat.reshape(-1)
    sz, sy = np.int64((Y + 1) * (X + 1)), np.int64(X + 1)
    full = cells is None
    if full:
        z, y, x = (a.reshape(-1) for a in np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij"))
    else:
        c = np.asarray(cells, np.int64).reshape(-1, 3)
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        assert (x >= 0).all() and (x < X).all() and (y >= 0).all() and (y < Y).all() and (z >= 0).all() and (z < Z).all()
    x, y, z = x.astype(np.int64), y.astype(np.int64), z.astype(np.int64)

    def is_empty(sel, n, neg):
        """is the cube of edge n[i] anchored at cell sel[i] empty?  (n is small enough for the cube to lie in the grid)"""
        lo, hi = [], []
        for c, s in zip((x[sel], y[sel], z[sel]), neg):
            lo.append(c - n + 1 if s else c)
            hi.append(c + 1 if s else c + n)
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        z0, z1, y0, y1 = z0 * sz, z1 * sz, y0 * sy, y1 * sy
        g = lambda k, j, i: flat[k + j + i]
        return (g(z1, y1, x1) - g(z0, y1, x1) - g(z1, y0, x1) - g(z1, y1, x0) + g(z0, y0, x1) + g(z0, y1, x0) + g(z1, y0, x0) - g(z0, y0, x0)) == 0

    out = np.zeros((8, len(x)), np.uint8)
    for o in range(8):
        neg = (bool(o & 1), bool(o & 2), bool(o & 4))
        room = np.minimum(np.minimum(x + 1 if neg[0] else X - x, y + 1 if neg[1] else Y - y), z + 1 if neg[2] else Z - z)
        good = np.zeros(len(x), np.int64)                # the cube of this edge is empty (edge 0: no cell)
        bad = np.minimum(room, FIELD_CAP) + 1            # the cube of this edge is not allowed: outside the grid or over the cap
        # the largest edge allowed first (in a sparse grid it settles most cells), then the bisection on the cells still open
        sel = np.arange(len(x))
        mid = bad - 1
        while len(sel):
            empty = is_empty(sel, mid, neg)
            good[sel[empty]] = mid[empty]
            bad[sel[~empty]] = mid[~empty]
            sel = sel[bad[sel] - good[sel] > 1]
            mid = (good[sel] + bad[sel]) // 2
        out[o] = good
    if not full:
        return out
    field = np.full((8, Z + 2, Y + 2, X + 2), 255, np.uint8)
    field[:, 1:-1, 1:-1, 1:-1] = out.reshape(8, Z, Y, X)
    return field


def occupancy(volume):
    """brick cells [z, y, x] of a voxel volume [z, y, x] that hold a solid voxel"""
    Z, Y, X = volume.shape
    return (np.asarray(volume) != 0).reshape(Z // 8, 8, Y // 8, 8, X // 8, 8).any(axis=(1, 3, 5))


def update_box(changed_cells, cells, cells_height):
    """The box of the field that Scene::edit recomputes when the occupancy of `changed_cells` (N x 3: x, y, z) changes, in the field's
    bordered coordinates (interior cells are 1 ... cells): dict rx0, rx1, ry0, ry1, rz0, rz1 (the box, upper bounds exclusive) and
    ay0, ay1, bz0, bz1 (the rows and slices that the x and y passes cover for it).  The formula of scene.cpp's field_update_box."""
    c = np.asarray(changed_cells, np.int64).reshape(-1, 3)
    assert len(c) > 0
    lim = (cells, cells, cells_height)
    r0 = [max(1, int(c[:, k].min()) + 1 - FIELD_REACH) for k in range(3)]
    r1 = [min(lim[k] + 1, int(c[:, k].max()) + 1 + FIELD_REACH + 1) for k in range(3)]
    return dict(rx0=r0[0], rx1=r1[0], ry0=r0[1], ry1=r1[1], rz0=r0[2], rz1=r1[2],
                ay0=max(1, r0[1] - FIELD_REACH), ay1=min(cells + 1, r1[1] + FIELD_REACH),
                bz0=max(1, r0[2] - FIELD_REACH), bz1=min(cells_height + 1, r1[2] + FIELD_REACH))


def field_sample_cells(shape, box, changed_cells, rng, n_random=200_000):
    """Cells (N x 3: x, y, z, unbordered) at which an updated field is compared with reference_field: the three axis planes through every
    changed cell, every cell within 2 cells of the update box's faces on either side, and n_random random cells."""
    Z, Y, X = shape
    dims = (X, Y, Z)
    parts = []
    grids = [np.arange(n) for n in dims]

    def slab(axis, values):
        values = np.unique([v for v in values if 0 <= v < dims[axis]])
        if len(values) == 0:
            return
        g = list(grids)
        g[axis] = values
        parts.append(np.stack([a.reshape(-1) for a in np.meshgrid(*g, indexing="ij")], 1))

    changed_cells = np.asarray(changed_cells).reshape(-1, 3)
    for axis in range(3):
        slab(axis, changed_cells[:, axis])
    # the box in unbordered coordinates: lo = r0 - 1 is its first cell, hi = r1 - 1 the first cell behind it
    for axis, (k0, k1) in enumerate((("rx0", "rx1"), ("ry0", "ry1"), ("rz0", "rz1"))):
        lo, hi = box[k0] - 1, box[k1] - 1
        slab(axis, list(range(lo - 2, lo + 2)) + list(range(hi - 2, hi + 2)))
    parts.append(np.stack([rng.integers(0, n, n_random) for n in dims], 1))
    cells = np.concatenate(parts).astype(np.int64)
    linear = np.unique((cells[:, 2] * Y + cells[:, 1]) * X + cells[:, 0])
    return np.stack([linear % X, linear // X % Y, linear // (X * Y)], 1)


# ---------------------------------------------------------------- the device world, cell by cell
def model_lod_and_bricks(volume, sx, sy, sz):
    """(occupied[4096], lod[4096], bricks[4096, 16]) of a supercell of the model volume, by the rules of canonical_supercell"""
    words, bricks = canonical_supercell(volume, sx, sy, sz)
    occupied = words != 0
    per_cell = np.zeros((4096, 16), np.uint32)
    per_cell[occupied] = bricks
    return occupied, (words >> np.uint32(12)) & np.uint32(0xFF), per_cell


def assert_device_world(scene, volume, changed=None):
    """Every cell of every supercell of the device world, and of the host world, against the model `volume` ([z, y, x], non-zero = solid),
    whatever slots the bricks stand in.  `changed`: global brick cells (N x 3: x, y, z) whose bricks the last batch changed -- a word of
    theirs that is not loaded must not carry the requested bit (the brick is asked for again).  Returns the number of loaded words."""
    info = scene.info()
    sg = info["supergrid_xy"]
    assert not info["failed"]
    changed_set = set()
    if changed is not None:
        changed_set = {(int(x), int(y), int(z)) for x, y, z in np.asarray(changed).reshape(-1, 3)}
    loaded_total = model_total = 0
    for sc in range(info["supercells"]):
        sx, sy, sz = sc % sg, (sc // sg) % sg, sc // (sg * sg)
        occupied, lod, want = model_lod_and_bricks(volume, sx, sy, sz)
        model_total += int(occupied.sum())
        w = scene.device_indices(sc)
        assert np.array_equal(w != 0, occupied), f"supercell {sc}: device words are non-zero at {np.count_nonzero((w != 0) != occupied)} wrong cells"
        got_lod = (w >> np.uint32(12)) & np.uint32(0xFF)
        assert np.array_equal(got_lod[occupied], lod[occupied]), f"supercell {sc}: LoD masks of {np.count_nonzero(got_lod[occupied] != lod[occupied])} device words differ from the model"
        is_loaded = (w & np.uint32(LOADED)) != 0
        rest = occupied & ~is_loaded
        assert not (w[is_loaded] & np.uint32(UNLOADED | REQUESTED)).any(), f"supercell {sc}: a loaded word also has the unloaded or requested bit"
        assert ((w[rest] & np.uint32(UNLOADED)) != 0).all(), f"supercell {sc}: a word that is neither loaded nor unloaded"
        assert not (w[rest] & np.uint32(0xFFF)).any(), f"supercell {sc}: slot bits in a word that is not loaded"
        assert not (w[occupied] & np.uint32(0x1FF00000)).any(), f"supercell {sc}: bits that mean nothing are set"
        slots = w[is_loaded] & np.uint32(0xFFF)
        assert len(np.unique(slots)) == len(slots), f"supercell {sc}: two cells share a device slot"
        for cell in np.nonzero(is_loaded)[0]:
            brick = scene.device_brick(sc, int(w[cell] & np.uint32(0xFFF)))
            assert np.array_equal(brick, want[cell]), f"supercell {sc} cell {cell} (device slot {w[cell] & 0xFFF}): the device brick differs from the model"
        if changed_set:
            for cell in np.nonzero(rest)[0]:
                g = (sx * 16 + (cell & 15), sy * 16 + ((cell >> 4) & 15), sz * 16 + (cell >> 8))
                if g in changed_set:
                    assert not (w[cell] & np.uint32(REQUESTED)), f"supercell {sc} cell {cell}: a changed brick that is not resident still carries the requested bit"
        loaded_total += int(is_loaded.sum())
        # the host world in the same pass (check_consistent of test_edit_host.py)
        hw, hb = scene.host_supercell(sc)
        assert len(hb) <= 4096
        assert np.array_equal(hw != 0, occupied), f"supercell {sc}: host words"
        live = hw[occupied]
        assert ((live & np.uint32(LOADED)) != 0).all() and not (live & np.uint32(0x70000000)).any(), f"supercell {sc}: host flags"
        hs = live & np.uint32(0xFFF)
        assert len(np.unique(hs)) == len(hs) and (hs < len(hb)).all(), f"supercell {sc}: host slots"
        assert np.array_equal(hb[hs], want[occupied]), f"supercell {sc}: host bricks differ from the model"
        assert np.array_equal((live >> np.uint32(12)) & np.uint32(0xFF), lod[occupied]), f"supercell {sc}: host LoD masks"
    assert info["resident_bricks"] == loaded_total, f"resident_bricks {info['resident_bricks']}, loaded words {loaded_total}"
    assert info["total_bricks"] == model_total, f"total_bricks {info['total_bricks']}, model {model_total}"
    return loaded_total


def all_device_words(scene):
    return np.concatenate([scene.device_indices(sc) for sc in range(scene.info()["supercells"])])


def cell_of(scene_info, sc, local):
    """global brick cell (x, y, z) of local cell `local` of supercell `sc`"""
    sg = scene_info["supergrid_xy"]
    return ((sc % sg) * 16 + (local & 15), ((sc // sg) % sg) * 16 + ((local >> 4) & 15), (sc // (sg * sg)) * 16 + (local >> 8))


# ---------------------------------------------------------------- edits on the numpy model
def model_box(volume, op, lo, hi):
    lo = [max(0, int(v)) for v in lo]
    hi = [min(n, int(v)) for v, n in zip(hi, volume.shape[::-1])]
    if all(h > l for l, h in zip(lo, hi)):
        volume[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = op == "set"


def model_sphere(volume, op, center, radius):
    Z, Y, X = volume.shape
    cx, cy, cz = (int(v) for v in center)
    r = int(radius)
    x0, x1, y0, y1, z0, z1 = max(0, cx - r), min(X, cx + r + 1), max(0, cy - r), min(Y, cy + r + 1), max(0, cz - r), min(Z, cz + r + 1)
    if x1 <= x0 or y1 <= y0 or z1 <= z0:
        return
    z, y, x = np.ogrid[z0:z1, y0:y1, x0:x1]
    m = (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r
    volume[z0:z1, y0:y1, x0:x1][m] = op == "set"


def model_voxels(volume, coords, values):
    """set_voxels on the model: coordinates outside the world are ignored, later entries win"""
    Z, Y, X = volume.shape
    c = np.asarray(coords).reshape(-1, 3)
    v = np.broadcast_to(np.asarray(values) != 0, (len(c),))
    ok = (c >= 0).all(1) & (c[:, 0] < X) & (c[:, 1] < Y) & (c[:, 2] < Z)
    for (x, y, z), s in zip(c[ok], v[ok]):
        volume[z, y, x] = s


def changed_bricks(before, after):
    """global brick cells (N x 3: x, y, z) whose voxels differ between two model volumes"""
    Z, Y, X = before.shape
    d = (before != after).reshape(Z // 8, 8, Y // 8, 8, X // 8, 8).any(axis=(1, 3, 5))
    z, y, x = np.nonzero(d)
    return np.stack([x, y, z], 1)


def field_update_tmp_bytes(box):
    """bytes of scratch that the field update of `box` needs (field_update_tmp_bytes, edit.hip)"""
    nx, nz = box["rx1"] - box["rx0"], box["bz1"] - box["bz0"]
    return 2 * nz * (box["ay1"] - box["ay0"]) * nx + 4 * nz * (box["ry1"] - box["ry0"]) * nx


# ---------------------------------------------------------------- field-update cases: sparse worlds changed by box edits
class FieldModel:
    """Cell occupancy of a sparse world under box edits.  A set box must cover empty cells only and a clear box must be one that was
    set (or the whole world), so that the occupancy follows from the boxes alone, without a voxel volume of the whole world."""

    def __init__(self, cells, cells_height):
        self.cells, self.cells_height = cells, cells_height
        self.occ = np.zeros((cells_height, cells, cells), bool)
        self.live = {}

    def apply(self, ops, want):
        """ops: [(op, lo, hi)] voxel boxes.  Returns (changed cells N x 3, the update box); asserts the box is what `want` says: per
        axis "inside" (free on both sides), "low" (clipped at the low side, free at the high), "high", "full", and under "check" a
        predicate on the box."""
        before = self.occ.copy()
        for op, lo, hi in ops:
            lo, hi = tuple(int(v) for v in lo), tuple(int(v) for v in hi)
            if op == "clear" and lo == (0, 0, 0) and hi == (self.cells * 8, self.cells * 8, self.cells_height * 8):
                self.occ[:] = False
                self.live.clear()
                continue
            sl = tuple(slice(lo[k] // 8, (hi[k] - 1) // 8 + 1) for k in (2, 1, 0))
            if op == "set":
                assert not self.occ[sl].any(), "a set box must cover empty cells only"
                self.live[(lo, hi)] = sl
                self.occ[sl] = True
            else:
                assert (lo, hi) in self.live, "a clear box must be a box that was set"
                self.occ[self.live.pop((lo, hi))] = False
        z, y, x = np.nonzero(before != self.occ)
        changed = np.stack([x, y, z], 1)
        assert len(changed) > 0, "the batch changes no cell's occupancy"
        box = update_box(changed, self.cells, self.cells_height)
        lim = dict(x=self.cells, y=self.cells, z=self.cells_height)
        for axis, kind in want.items():
            if axis == "check":
                assert kind(box), f"the update box {box} is not what the case is for"
                continue
            r0, r1 = box[f"r{axis}0"], box[f"r{axis}1"]
            got = {(True, True): "inside", (False, True): "low", (True, False): "high", (False, False): "full"}[(r0 > 1, r1 < lim[axis] + 1)]
            assert got == kind, f"the update box is '{got}' on {axis} ([{r0}, {r1}) of 1 ... {lim[axis]}), the case is for '{kind}'"
        return changed, box


def voxel_in_cell(cx, cy, cz, off=(3, 4, 5)):
    """(op-less) one-voxel box inside brick cell (cx, cy, cz)"""
    lo = (cx * 8 + off[0], cy * 8 + off[1], cz * 8 + off[2])
    return lo, (lo[0] + 1, lo[1] + 1, lo[2] + 1)


def flat_field_plan(cells):
    """Batches of the wide and flat world (cells x cells x 16 brick cells; cells = 512, or 272 when memory is short): a list of
    (name, ops, want).  Names ending in '=NAME' must reproduce the field bytes kept under NAME, names ending in '>NAME' keep theirs."""
    wide = cells == 512
    assert wide or cells == 272
    size = cells * 8
    mid = 256 if wide else 5
    k = "inside" if wide else "low"
    centre, corner, far = voxel_in_cell(mid, mid, 8), voxel_in_cell(0, 0, 0), voxel_in_cell(cells - 1, cells - 1, 15)
    ys, zs = (mid - 1) * 8 + 2, 3 * 8 + 1
    slab_x = ((0, ys, zs), (size, ys + 1, zs + 1))
    xs, zs = (mid - 1) * 8 + 5, 5 * 8 + 6
    slab_y = ((xs, 0, zs), (xs + 1, size, zs + 1))
    plan = [
        ("empty>F0", [], {}),
        ("one voxel at the centre", [("set", *centre)], dict(x=k, y=k, z="full")),
        ("one voxel in cell (0, 0, 0)", [("set", *corner)], dict(x="low", y="low", z="full")),
        ("one voxel in the far corner", [("set", *far)], dict(x="high", y="high", z="full", check=lambda b: b["ay0"] > 1 or not wide)),
        ("a slab across x", [("set", *slab_x)], dict(x="full", y=k, z="full")),
        ("a slab across y", [("set", *slab_y)], dict(x=k, y="full", z="full")),
    ]
    if wide:
        a, b = voxel_in_cell(100, 255, 10), voxel_in_cell(400, 256, 10)
        plan += [
            ("two changes 300 cells apart", [("set", *a), ("set", *b)], dict(x="full", y="inside", z="full")),
            ("the clear of one of them", [("clear", *b)], dict(x="high", y="inside", z="full")),
        ]
    plan += [
        ("before the clear of the first voxel>F5", [], {}),
        ("the clear of the first voxel>F6", [("clear", *centre)], dict(x=k, y=k, z="full")),
        ("the first voxel again=F5", [("set", *centre)], dict(x=k, y=k, z="full")),
        ("and cleared again=F6", [("clear", *centre)], dict(x=k, y=k, z="full")),
        ("everything cleared=F0", [("clear", (0, 0, 0), (size, size, 128))], dict(x="full", y="full", z="full")),
    ]
    return plan


def scratch_growth_plan(cells):
    """On a fresh scene: a small box, one that spans the width (the scratch buffer grows), a small one again"""
    mid = 256 if cells == 512 else 5
    size = cells * 8
    corner = voxel_in_cell(0, 0, 0)
    ys, zs = (mid - 1) * 8 + 2, 3 * 8 + 1
    slab_x = ((0, ys, zs), (size, ys + 1, zs + 1))
    k = "inside" if cells == 512 else "low"
    return [
        ("a small box", [("set", *corner)], dict(x="low", y="low", z="full")),
        ("a box that spans the width", [("set", *slab_x)], dict(x="full", y=k, z="full")),
        ("a small box again", [("clear", *corner)], dict(x="low", y="low", z="full")),
    ]


def tall_field_plan():
    """Batches of the tall and thin world (16 x 16 x 512 brick cells)"""
    centre, corner, far = voxel_in_cell(8, 8, 256), voxel_in_cell(0, 0, 0), voxel_in_cell(15, 15, 511)
    a, b = voxel_in_cell(3, 4, 100), voxel_in_cell(12, 9, 400)
    halo = lambda box: box["bz1"] - box["bz0"] != box["rz1"] - box["rz0"]
    return [
        ("empty>F0", [], {}),
        ("one voxel at the centre>F1", [("set", *centre)], dict(x="full", y="full", z="inside", check=halo)),
        ("one voxel in cell (0, 0, 0)", [("set", *corner)], dict(x="full", y="full", z="low", check=halo)),
        ("one voxel in the far corner", [("set", *far)], dict(x="full", y="full", z="high", check=lambda box: box["rz0"] > 1 and box["bz0"] > 1 and halo(box))),
        ("two changes 300 cells apart", [("set", *a), ("set", *b)], dict(x="full", y="full", z="full")),
        ("the clear of the upper one", [("clear", *b)], dict(x="full", y="full", z="high", check=halo)),
        ("the clear of the lower one", [("clear", *a)], dict(x="full", y="full", z="low", check=halo)),
        ("the clear of the corners", [("clear", *corner), ("clear", *far)], dict(x="full", y="full", z="full")),
        ("back to the first voxel alone=F1", [], {}),
        ("the clear of the first voxel=F0", [("clear", *centre)], dict(x="full", y="full", z="inside", check=halo)),
    ]


CUBIC_CELLS = 272
CUBIC_VOXELS = ((43, 44, 45), (2131, 2132, 2133))  # in cells (5, 5, 5) and (266, 266, 266)


def cubic_field_plan():
    """Batches of the cubic world (272^3 brick cells): each box is partial on all three axes at once"""
    a, b = CUBIC_VOXELS
    return [
        ("one voxel in cell (5, 5, 5)", [("set", a, tuple(v + 1 for v in a))], dict(x="low", y="low", z="low")),
        ("one voxel in cell (266, 266, 266)", [("set", b, tuple(v + 1 for v in b))], dict(x="high", y="high", z="high", check=lambda box: box["ay0"] == 1 and box["bz0"] == 1)),
    ]


def cubic_rays():
    """Axis-parallel rays through the cubic world with both voxels set: (origins, directions, hit voxel or None, geometric distance).
    From voxel centres on the faces towards the voxels, through 266 empty brick cells, and the same rays moved by one voxel sideways."""
    size = CUBIC_CELLS * 8
    a, b = (np.array(v) for v in CUBIC_VOXELS)
    origins, directions, voxels, distances = [], [], [], []
    for target, sign in ((b, 1), (a, -1)):  # towards b from the low faces along +axis, towards a from the high faces along -axis
        for axis in range(3):
            d = np.zeros(3)
            d[axis] = sign
            o = target + 0.5
            o[axis] = 0.5 if sign > 0 else size - 0.5
            face = target[axis] if sign > 0 else target[axis] + 1
            origins.append(o.copy()), directions.append(d), voxels.append(tuple(int(v) for v in target)), distances.append(abs(face - o[axis]))
            for side in range(3):
                if side == axis:
                    continue
                for shift in (-1, 1):
                    m = o.copy()
                    m[side] += shift
                    origins.append(m), directions.append(d), voxels.append(None), distances.append(np.inf)
    return np.array(origins, np.float32), np.array(directions, np.float32), voxels, np.array(distances)


# ---------------------------------------------------------------- randomised edits of the 256^3 terrain
def apply_to_model(volume, batch):
    for e in batch:
        if e[0] == "box":
            model_box(volume, e[1], e[2], e[3])
        elif e[0] == "sphere":
            model_sphere(volume, e[1], e[2], e[3])
        else:
            model_voxels(volume, e[1], e[2])


def apply_to_scene(bm, scene, batch):
    """one call per batch: set_voxels for a batch that is a voxel list, else one edit list"""
    if batch[0][0] == "voxels":
        assert len(batch) == 1
        scene.set_voxels(np.asarray(batch[0][1], np.int32), np.asarray(batch[0][2], np.uint8))
        return
    scene.edit([bm.edit_box(e[1], e[2], e[3]) if e[0] == "box" else bm.edit_sphere(e[1], e[2], e[3]) for e in batch])


def random_batches(size=256, n=32, seed=2024):
    """A fixed lead-in (whole bricks emptied; sky filled where a supercell holds few bricks, so that its pool must grow; voxels into the
    emptied region, so that freed slots are reused), then n seeded batches of 1-4 edits: boxes and spheres, set and clear, across
    supercell borders and the world's faces, or a list of single voxels with duplicates and coordinates outside the world."""
    rng = np.random.default_rng(seed)
    batches = [
        [("box", "clear", (0, 0, 96), (64, 64, size))],
        [("box", "set", (10, 140, 200), (60, 200, 250))],
        [("voxels", np.stack([rng.integers(0, 64, 400), rng.integers(0, 64, 400), rng.integers(100, 200, 400)], 1), np.ones(400, np.uint8))],
        [("box", "clear", (120, 120, 0), (136, 136, size)), ("sphere", "set", (128, 128, 230), 20)],
        [("box", "set", (size - 20, size - 30, size - 10), (size + 40, size + 40, size + 40)), ("sphere", "clear", (-5, 128, 150), 30)],
    ]
    for _ in range(n):
        if rng.random() < 0.25:
            m = int(rng.integers(50, 600))
            c = rng.integers(-4, size + 4, (m, 3))
            c[: m // 4] = c[m // 2: m // 2 + m // 4]  # duplicates, with values of their own
            batches.append([("voxels", c, rng.integers(0, 2, m).astype(np.uint8))])
            continue
        batch = []
        for _ in range(int(rng.integers(1, 5))):
            op = "set" if rng.random() < 0.5 else "clear"
            if rng.random() < 0.5:
                lo = rng.integers(-10, size - 8, 3)
                ext = rng.integers(1, 70, 3)
                if rng.random() < 0.3:
                    lo, ext = lo // 8 * 8, (ext + 7) // 8 * 8  # whole bricks
                batch.append(("box", op, tuple(int(v) for v in lo), tuple(int(v) for v in lo + ext)))
            else:
                batch.append(("sphere", op, tuple(int(v) for v in rng.integers(-10, size + 10, 3)), int(rng.integers(1, 40))))
        batches.append(batch)
    return batches
