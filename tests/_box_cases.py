"""Helpers of the region-edge and volume-edge tests (no tests here): three small seeded worlds that are not all cubes, the boxes that
sweep every chunk, cell and run residue of csrc/region.hip, the record batches that reach the plan and addressing edges of
csrc/volume.hip, and the numpy models they are compared with.  The generators are plain functions of the world's dimensions, so that
tests/test_box_cases_host.py can check what they cover without a GPU."""
import functools

import numpy as np

LOADED = 0x80000000
RUN = 128  # voxels of a run of 16 brick cells, and of a supercell's edge
BOX, SPHERE = 1, 2

# name -> voxels (x, y, z); supergrids 3 x 3 x 1, 1 x 1 x 3 and 2 x 2 x 2
WORLDS = {"flat": (384, 384, 128), "tall": (128, 128, 384), "cube": (256, 256, 256)}
ROUTES = ("aligned", "general")
# a block of wholly empty cells, (x0, x1), (y0, y1), (z0, z1) in voxels: next to the sweeps' anchors in the flat and the cubic world (a
# camera inside it makes the cells of its walls resident and leaves those behind them unloaded), a shaft open to the top in the tall one
HOLES = {"flat": ((144, 192), (32, 160), (24, 96)), "tall": ((64, 104), (24, 88), (96, 384)), "cube": ((144, 192), (32, 160), (24, 144))}
# fully solid brick cells (cx, cy, cz); those of the tall world stand in its shaft, where they stop sweeps
SOLID_CELLS = {"flat": ((1, 1, 1), (14, 5, 4), (15, 16, 8), (47, 47, 15)), "tall": ((9, 5, 25), (11, 9, 40), (1, 1, 1), (15, 15, 47)),
               "cube": ((1, 1, 1), (14, 5, 4), (15, 15, 15), (16, 16, 16), (31, 31, 31))}
SEEDS = {"flat": 301, "tall": 302, "cube": 303}
# the axes a sweep does not vary stand at these residues (lo % 8, hi % 8 = 3, 6 on y and 3, 5 on z)
FIXED_Y, FIXED_Z = (43, 62), (35, 53)


@functools.lru_cache(maxsize=None)
def world_voxels(name):
    """uint8 [z, y, x] of the world `name`: 30 % of the voxels solid at random, the hole empty, a few cells solid.  Do not write to it."""
    X, Y, Z = WORLDS[name]
    rng = np.random.default_rng(SEEDS[name])
    vox = (rng.random((Z, Y, X), dtype=np.float32) < 0.3).astype(np.uint8)
    (x0, x1), (y0, y1), (z0, z1) = HOLES[name]
    vox[z0:z1, y0:y1, x0:x1] = 0
    for cx, cy, cz in SOLID_CELLS[name]:
        vox[cz * 8:cz * 8 + 8, cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] = 1
    vox.setflags(write=False)
    return vox


def volume_for(rng, shape, fill=0.5):
    """a volume [z, y, x] to write: non-zero = solid, any value"""
    return (rng.random(shape) < fill).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)


# ---------------------------------------------------------------- models
def model_read(vol, lo, hi):
    """numpy model of read_region: the voxels lo <= v < hi of `vol` [z, y, x], 0 outside the world"""
    Z, Y, X = vol.shape
    out = np.zeros((hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]), np.uint8)
    a = [max(0, int(lo[k])) for k in range(3)]
    b = [min(n, int(hi[k])) for k, n in enumerate((X, Y, Z))]
    if all(h > l for l, h in zip(a, b)):
        out[a[2] - lo[2]:b[2] - lo[2], a[1] - lo[1]:b[1] - lo[1], a[0] - lo[0]:b[0] - lo[0]] = vol[a[2]:b[2], a[1]:b[1], a[0]:b[0]] != 0
    return out


def cell_grid(values, info):
    """per-cell values in the order of the device index words (supercell by supercell) -> [cz, cy, cx]"""
    sg, sgz = info["supergrid_xy"], info["supergrid_z"]
    return values.reshape(sgz, sg, sg, 16, 16, 16).transpose(0, 3, 1, 4, 2, 5).reshape(sgz * 16, sg * 16, sg * 16)


def box_cells(grid, lo, hi):
    """the part of a per-cell grid [cz, cy, cx] that the box lo <= v < hi, clipped to the world, overlaps (empty when nothing is left)"""
    dims = [8 * n for n in grid.shape[::-1]]
    a = [max(0, int(lo[k])) for k in range(3)]
    b = [min(dims[k], int(hi[k])) for k in range(3)]
    if any(h <= l for l, h in zip(a, b)):
        return grid[:0, :0, :0]
    return grid[a[2] >> 3:((b[2] - 1) >> 3) + 1, a[1] >> 3:((b[1] - 1) >> 3) + 1, a[0] >> 3:((b[0] - 1) >> 3) + 1]


# ---------------------------------------------------------------- region cases: lists of (lo, hi), each (x, y, z), not clipped
def run_boundaries(n):
    """the multiples of 128 inside an axis of n voxels"""
    return list(range(RUN, n, RUN))


def x_sweep(dims, route):
    """Boxes over every pair (lo.x % 16, hi.x % 16) the route can see, around the run boundary x = 128 (and x = 256 where the world has
    one): inside one 16-byte chunk, inside one brick cell, ending on the boundary, across it with whole chunks in between.  aligned: lo.x
    is a multiple of 16 (so the pairs are (0, b)), and lo.x = -16 and -32 make the clipped lo.x differ from the volume's origin."""
    X = dims[0]
    boxes = []
    if route == "general":
        for a in range(16):
            for b in range(16):
                lo = RUN - 16 + a  # short: within the chunk when b > a, onto the boundary when b == 0, else just across it
                boxes.append((lo, RUN - 16 + b if b > a else RUN + b))
                boxes.append((RUN - 48 + a, RUN + 16 + b if b else RUN))  # long: whole chunks in between; b == 0 ends on the boundary
                for B in run_boundaries(X)[1:]:
                    boxes.append((B - 48 + a, B + 16 + b if b else B))
    else:
        for lo in [-32, -16, 0] + [B - d for B in run_boundaries(X) or [RUN] for d in (32, 16, 0) if B - d < X]:
            first = max(0, -lo // 16)
            for b in range(16):
                for w in (first, first + 1, first + 3):
                    hi = lo + 16 * w + b
                    boxes.append((lo, hi if hi > max(lo, 0) else hi + 16))
    return [((x0, FIXED_Y[0], FIXED_Z[0]), (x1, FIXED_Y[1], FIXED_Z[1])) for x0, x1 in boxes]


def fixed_x(dims, route, thin=False):
    """the x-range of a y or z sweep: across x = 128 where the world is wider than that.  aligned: from a multiple of 16, and a multiple of
    16 long when the box is one row thick (its row pitch is then its length)"""
    x0 = RUN - 16 if dims[0] > RUN else RUN - 32
    if route == "general":
        return x0 + 5, x0 + 27
    return x0, x0 + (32 if thin else 27)


def axis_sweep(dims, route, axis):
    """Boxes over every pair (lo % 8, hi % 8) on y (axis 1) or z (axis 2): one cell thick next to, and across, each supercell boundary of
    the axis (or the cell boundary at 64 where the axis is one supercell long)"""
    out = []
    for B in run_boundaries(dims[axis]) or [64]:
        for a in range(8):
            for b in range(8):
                thin = (B - 24 + a, B - 24 + b if b > a else B - 16 + b)   # in one cell when b > a or b == 0, else across one cell boundary
                cross = (B - 16 + a, B + 8 + b)                          # across B
                for v0, v1 in (thin, cross):
                    x0, x1 = fixed_x(dims, route, thin=axis == 1 and v1 - v0 == 1)
                    lo, hi = [x0, FIXED_Y[0], FIXED_Z[0]], [x1, FIXED_Y[1], FIXED_Z[1]]
                    lo[axis], hi[axis] = v0, v1
                    out.append((tuple(lo), tuple(hi)))
    return out


def clipping_faces(dims, lo, hi):
    """the faces (-x, +x, -y, +y, -z, +z as 0 ... 5) that clip a box which keeps a part inside the world; empty for a box wholly outside"""
    if any(hi[k] <= 0 or lo[k] >= dims[k] or hi[k] <= lo[k] for k in range(3)):
        return set()
    return {2 * k for k in range(3) if lo[k] < 0} | {2 * k + 1 for k in range(3) if hi[k] > dims[k]}


def random_boxes(dims, route, n=300, seed=0):
    """n seeded boxes of up to 72 x 40 x 40 voxels, every third one clipped by a face (the six faces in turn), then one box wholly outside
    the world and one that contains it"""
    rng = np.random.default_rng(1000 + seed)
    dims = np.asarray(dims)
    out = []
    for i in range(n):
        ext = rng.integers(2, [73, 41, 41])
        lo = rng.integers(0, dims - ext + 1)
        if i % 3 == 0:
            k, far = (i // 3) % 6 // 2, (i // 3) % 2
            if k == 0:
                ext[0] = max(ext[0], 18)
            cut = int(rng.integers(1, ext[k]))  # voxels left outside
            if k == 0 and route == "aligned":
                cut = 16
            lo[k] = dims[k] - ext[k] + cut if far else -cut
        if route == "aligned":
            lo[0] = lo[0] // 16 * 16
            if i % 3 == 0 and (i // 3) % 6 == 1:
                ext[0] = dims[0] - lo[0] + 16
        out.append((tuple(int(v) for v in lo), tuple(int(v) for v in lo + ext)))
    out.append(((int(dims[0]) + 16, 5, 5), (int(dims[0]) + 36, 15, 17)))
    x0 = -16 if route == "aligned" else -13
    out.append(((x0, -3, -2), (int(dims[0]) + 5, int(dims[1]) + 4, int(dims[2]) + 3)))
    return out


SWEEPS = ("x", "y", "z", "random")


def region_cases(world, route, sweep):
    dims = WORLDS[world]
    if sweep == "x":
        return x_sweep(dims, route)
    if sweep in ("y", "z"):
        return axis_sweep(dims, route, "xyz".index(sweep))
    return random_boxes(dims, route, seed=SEEDS[world] + ROUTES.index(route))


class Slab:
    """A device tensor larger than every ordinary case, and slices of it at the route's alignment.  aligned: the base, both pitches and
    the slice's x offset are multiples of 16; general: odd pitches and an odd x offset."""
    CASE = (48, 48, 96)  # the largest ordinary case [z, y, x]; the two whole-world cases get tensors of their own

    def __init__(self, torch, route, fill):
        self.torch, self.route, self.fill = torch, route, fill
        self.big = self.make((self.CASE[0] + 4, self.CASE[1] + 6, 128 if route == "aligned" else 107))

    def make(self, shape):
        return self.torch.full(shape, self.fill, dtype=self.torch.uint8, device="cuda:0")

    def offsets(self, i):
        return 1 + i % 3, 2 + i % 4, 16 * (i % 2) if self.route == "aligned" else 1 + 2 * (i % 4)

    def view(self, shape, i):
        """(the tensor the slice is cut from, the slice, its index) for a case of `shape` [z, y, x]"""
        big = self.big
        z0, y0, x0 = self.offsets(i)
        if any(n > m for n, m in zip(shape, self.CASE)):
            nx = shape[2] + 32
            big = self.make((shape[0] + 4, shape[1] + 6, nx // 16 * 16 if self.route == "aligned" else nx // 2 * 2 + 1))
        sl = np.s_[z0:z0 + shape[0], y0:y0 + shape[1], x0:x0 + shape[2]]
        return big, big[sl], sl


def assert_route(bm, route, lo, view):
    """the case takes the instantiation it is meant for: what aligned16 (region.hip) tests, on the region the library is given"""
    r, ptr, cuda = bm.region_of(lo, view)
    aligned = ptr % 16 == 0 and r.row_pitch % 16 == 0 and r.slice_pitch % 16 == 0 and lo[0] % 16 == 0
    assert cuda and aligned == (route == "aligned"), (route, lo, tuple(view.shape), ptr % 16, r.row_pitch, r.slice_pitch)


# ---------------------------------------------------------------- a streaming scene of one of the worlds, some bricks resident
def streaming_scene(bm, torch, world):
    """The world `world` with the residency a few frames leave: cameras inside the hole look along -x, +y, -y and down, so the cells of
    its walls are loaded and the cells behind them are not (as mixed_residency of test_gpu_region.py: frames, then the load queue)."""
    from test_gpu_edit import render
    X, Y, Z = WORLDS[world]
    scene = bm.Scene(X, Z, device=0)
    scene.set_queue_capacity(1 << 16)
    scene.load_voxels(world_voxels(world))
    scene.reset_residency().set_streaming_mode(0)
    centre = tuple(float(a + b) / 2 for a, b in HOLES[world])
    for h, v in ((-np.pi / 2, 0.0), (0.3, 0.2), (np.pi - 0.3, -0.2), (-np.pi / 2 + 0.5, -1.0)):
        cam = bm.Camera(position=centre, horizontal_angle=h, vertical_angle=v).update()
        for _ in range(2):
            render(bm, torch, scene, cam)
            scene.process_load_queue()
    info = scene.info()
    assert 0 < info["resident_bricks"] < info["total_bricks"] and not info["failed"]
    return scene


# ---------------------------------------------------------------- volume records
def items_of(recs, dims):
    """work items of each record (volume.hip load_shape): runs of 128 voxels per row x cell rows x cell slices of the clipped shape,
    0 for a malformed record and for one with nothing inside the world"""
    lo, hi = recs["lo"].astype(np.int64), recs["hi"].astype(np.int64)
    sphere = recs["shape"] == SPHERE
    ok = ((recs["shape"] == BOX) | sphere) & (recs["reserved"] == 0) & ~(sphere & (recs["radius"] < 0)) & (sphere | (hi >= lo).all(1))
    c, r = recs["center"].astype(np.int64), recs["radius"].astype(np.int64)[:, None]
    lo, hi = np.where(sphere[:, None], c - r, lo), np.where(sphere[:, None], c + r + 1, hi)
    top = np.asarray(dims, np.int64)
    lo, hi = np.clip(lo, 0, top), np.clip(hi, 0, top)
    inside = ok & (lo < hi).all(1)
    n = np.stack([((hi[:, 0] - 1) >> 7) - (lo[:, 0] >> 7) + 1, ((hi[:, 1] - 1) >> 3) - (lo[:, 1] >> 3) + 1, ((hi[:, 2] - 1) >> 3) - (lo[:, 2] >> 3) + 1], 1)
    return np.where(inside, n.prod(1), 0)


def zero_item_records(bm, dims):
    """seven records without a work item: outside the world, an empty box inside it, and malformed ones of each kind"""
    X, Y, Z = dims
    recs = np.concatenate([
        bm.volume_box((X + 3, 5, 5), (X + 40, 50, 50)), bm.volume_box((20, 30, 40), (20, 60, 70)), bm.volume_box((10, 10, 10), (20, 9, 20)),
        bm.volume_sphere((50, 50, 50), -1), bm.volume_sphere((40, 40, -90), 30), bm.volume_box((5, 5, 5), (9, 9, 9)), bm.volume_box((5, 5, 5), (9, 9, 9))])
    recs["shape"][5] = 3
    recs["reserved"][6] = 9
    return recs


def mixed_records(bm, rng, dims, n_small=3000):
    """The recipe of test_gpu_volume.py's mixed_records for a world of dims = (X, Y, Z): single voxels, boxes inside one cell, small boxes
    across cells and faces, boxes across a supercell corner, boxes clipped by each of the six faces, boxes outside, the whole world, one box
    per supercell that covers exactly that supercell, spheres of radius 0, 1, 7 and 40, spheres centred outside each face, and malformed
    records in between.  The last record is the whole world."""
    dims = np.asarray(dims)
    parts = []
    p = rng.integers(0, dims, (n_small // 4, 3))
    parts.append(bm.volume_box(p, p + 1))
    c = rng.integers(0, dims // 8, (n_small // 4, 3)) * 8
    a = rng.integers(0, 8, (n_small // 4, 3))
    parts.append(bm.volume_box(c + a, c + a + rng.integers(0, 9, a.shape).clip(0, 8 - a)))
    p = rng.integers(-20, dims + 10, (n_small // 2, 3))
    parts.append(bm.volume_box(p, p + rng.integers(0, 24, p.shape)))
    corner = np.minimum(RUN, dims - 1)  # a supercell corner, or the world's face where the axis is one supercell long
    p = corner - rng.integers(1, 40, (100, 3))
    parts.append(bm.volume_box(p, corner + rng.integers(1, 40, p.shape)))
    for k in range(3):
        for side in (0, 1):
            lo = rng.integers(20, dims - 60, (20, 3))
            hi = lo + rng.integers(1, 60, lo.shape)
            if side:
                hi[:, k] = dims[k] + rng.integers(0, 50, 20)
            else:
                lo[:, k] = -rng.integers(0, 50, 20)
            parts.append(bm.volume_box(lo, hi))
            centre = rng.integers(20, dims - 20, (4, 3))
            centre[:, k] = dims[k] + rng.integers(0, 30, 4) if side else -rng.integers(1, 30, 4)
            parts.append(bm.volume_sphere(centre, 60))                                       # centred outside this face
    far = rng.integers(dims.max() + 1, dims.max() + 1000, (50, 3)) * rng.choice([-1, 1], (50, 3))
    parts.append(bm.volume_box(far, far + 9))
    parts.append(bm.volume_box([(2 ** 31 - 10, 0, 0), (-2 ** 31, -2 ** 31, -2 ** 31)], [(2 ** 31 - 1, 9, 9), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]))
    sc = np.stack(np.meshgrid(*[np.arange(0, n, RUN) for n in dims], indexing="ij"), -1).reshape(-1, 3)
    parts.append(bm.volume_box(sc, sc + RUN))                                                # each supercell, exactly
    for radius, count in ((0, 300), (1, 300), (7, 300), (40, 24)):
        parts.append(bm.volume_sphere(rng.integers(-radius - 5, dims + radius + 5, (count, 3)), radius))
    # centres 2^25 and 2^31 voxels away: the first one's cap covers the lowest 21 slices, the second one ends at x = 0
    parts.append(bm.volume_sphere([(dims[0] // 2, dims[1] // 2, -2 ** 25), (-2 ** 31, 5, 5)], [2 ** 25 + 20, 2 ** 31 - 1]))
    recs = np.concatenate(parts)
    recs = recs[rng.permutation(len(recs))]
    bad = rng.choice(len(recs), 100, replace=False)
    for j, i in enumerate(bad):
        kind = j % 5
        if kind == 0:
            recs["shape"][i] = rng.choice([0, 3, -1, 77])
        elif kind == 1:
            recs[i] = bm.volume_box((10, 10, 10), (20, 9, 20))[0]
        elif kind == 2:
            recs[i] = bm.volume_sphere((50, 50, 50), -1)[0]
        elif kind == 3:
            recs["reserved"][i] = 1 + j
        else:
            recs[i] = bm.volume_box((10, 10, 10), (9, 20, 20))[0]
    return np.concatenate([recs, bm.volume_box((0, 0, 0), dims)])


BASE_RECORDS = 4099               # not a multiple of 256
BIG_RECORDS = 3 * 65536 + 77      # 769 workgroups of volume_plan: volume_scan's threads own 4 each, and the last 63 threads none
# first workgroup and number of workgroups of each spliced run of zero-item records (the last one: the last full workgroup)
BIG_RUNS = ((0, 1), (300, 3), (511, 1), (BIG_RECORDS // 256 - 1, 1))


def base_batch(bm):
    """4099 mixed records of the cubic world, the first of them with work items"""
    dims = WORLDS["cube"]
    recs = mixed_records(bm, np.random.default_rng(81), dims, n_small=3600)
    assert len(recs) >= BASE_RECORDS
    recs = recs[len(recs) - BASE_RECORDS:]  # (keeps the whole-world box)
    first = int(np.nonzero((items_of(recs, dims) > 0) & (recs["shape"] == BOX))[0][0])
    return np.roll(recs, -first)


def tiled(base, want, n):
    """the first n records of the base batch repeated, and of its model"""
    idx = np.arange(n) % len(base)
    return base[idx], want[idx]


def big_batch(bm, base, want, zero, zero_want, empty_tail):
    """(records, model) of the big batch: the base batch tiled, with BIG_RUNS -- and with `empty_tail` the 77 records of the last, partial
    workgroup -- replaced by zero-item records"""
    recs, res = tiled(base, want, BIG_RECORDS)
    recs, res = recs.copy(), res.copy()
    spans = [(256 * w, 256 * (w + k)) for w, k in BIG_RUNS] + ([(BIG_RECORDS // 256 * 256, BIG_RECORDS)] if empty_tail else [])
    for a, b in spans:
        idx = (np.arange(a, b) * 3) % len(zero)
        recs[a:b], res[a:b] = zero[idx], zero_want[idx]
    return recs, res


def run_records(bm, dims):
    """Boxes whose lo.x and hi.x sweep every residue mod 8 around each run boundary and residues mod 128 from 0 to 127, over 1, 2, 4 and
    5 rows of cells in turn, so that a record has 1 to 15 work items and the four items of a wave belong to one, two or four records (a
    clipped record has at most dims.x / 128 runs per row, so the item counts come from rows as well as from runs).  Each box is followed by
    a sphere with the same upper x bound and, where the box is at most 25 voxels long, the same x-range."""
    X = dims[0]
    los = set()
    for B in range(0, X, RUN):
        los |= {B + r for r in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 100, 119, 120, 121, 122, 123, 124, 125, 126, 127)}
        los |= {B + r for r in range(-8, 9)} if B else set()
    boxes = []
    for lo in sorted(los):
        his = {lo + k for k in range(1, 9)} | {B + r for B in range(RUN, X + 1, RUN) for r in (-1, 0, 1, 7, 8)} | {X + 3}
        for hi in sorted(h for h in his if h > lo):
            rows = (1, 2, 4, 5)[len(boxes) % 4]
            boxes.append(((lo, FIXED_Y[0], FIXED_Z[0]), (hi, FIXED_Y[0] + 8 * (rows - 1) + 3, FIXED_Z[0] + 3)))
    lo, hi = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
    radius = np.minimum((hi[:, 0] - lo[:, 0]) // 2, 12)
    centre = np.stack([hi[:, 0] - 1 - radius, (lo[:, 1] + hi[:, 1]) // 2, (lo[:, 2] + hi[:, 2]) // 2], 1)
    recs = np.zeros(2 * len(boxes), bm.VOLUME_DTYPE)
    recs[0::2], recs[1::2] = bm.volume_box(lo, hi), bm.volume_sphere(centre, radius)
    return recs


def tall_sweeps(n=300, seed=91):
    """(lo, hi, sign, dist) of n boxes in and around the tall world's shaft, swept along +z and -z by up to 300 voxels: through z = 128
    and z = 256, onto the shaft's floor and the solid cells in it, and out of the top"""
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1), (z0, z1) = HOLES["tall"]
    lo = np.stack([rng.integers(x0 - 4, x1 - 2, n), rng.integers(y0 - 4, y1 - 2, n), rng.integers(z0 - 6, z1 + 6, n)], 1)
    hi = lo + rng.integers(1, 9, (n, 3))
    sign = np.where(np.arange(n) % 2 == 0, 1, -1)
    dist = rng.integers(0, 301, n)
    return lo, hi, sign, dist


def model_sweep(vox, lo, hi, axis, sign, dist, pad=(16, 16, 320)):
    """translate and test on the world with pad = (x, y, z) empty voxels round it (more than any box reaches): the largest d <= dist such
    that the box moved by 1 ... d voxels meets nothing solid"""
    Z, Y, X = vox.shape
    pad = np.asarray(pad)
    world = np.zeros((Z + 2 * pad[2], Y + 2 * pad[1], X + 2 * pad[0]), np.uint8)
    world[pad[2]:pad[2] + Z, pad[1]:pad[1] + Y, pad[0]:pad[0] + X] = vox
    top = np.array([X, Y, Z]) + 2 * pad
    out = np.zeros(len(lo), np.int64)
    for i in range(len(lo)):
        for k in range(1, int(dist[i]) + 1):
            a, b = lo[i].copy(), hi[i].copy()
            a[axis[i]] += sign[i] * k
            b[axis[i]] += sign[i] * k
            a, b = np.clip(a + pad, 0, top), np.clip(b + pad, 0, top)
            if world[a[2]:b[2], a[1]:b[1], a[0]:b[0]].any():
                break
            out[i] = k
    return out
