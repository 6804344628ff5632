"""A numpy model of the surface-extraction contract (include/brickmap.h, "voxels -> the quads of their surface"), written from its
sentences: face arrays by shifting the volume, the world's 8^3 cells by floor division, an 8 x 8 boolean array per (cell, direction,
slice), and the greedy cover as a loop over array slices -- no bit tricks and none of the library's loops.  Slow and plain: the tests run it
on small volumes."""
import numpy as np

QUAD_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("shape", "<u4")])
RESULT_DTYPE = np.dtype([("quads", "<u8"), ("faces", "<u8")])
# direction -> (axis, step); axes are x = 0, y = 1, z = 2, arrays are [z, y, x]
DIRECTIONS = [(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]
IN_SLICE = {0: (1, 2), 1: (0, 2), 2: (0, 1)}   # the (u, v) axes of an axis: the other two, ascending


def face_arrays(volume, halo=False):
    """six bool arrays [z, y, x]: voxel p is solid, is meshed, and its neighbour p + d is empty (outside the volume: empty)"""
    solid = np.asarray(volume) != 0
    padded = np.pad(solid, 1)
    meshed = np.ones(solid.shape, bool)
    if halo:
        meshed[:] = False
        meshed[1:-1, 1:-1, 1:-1] = True
    out = []
    for axis, step in DIRECTIONS:
        neighbour = np.roll(padded, -step, axis=2 - axis)[1:-1, 1:-1, 1:-1]
        out.append(solid & meshed & ~neighbour)
    return out


def greedy_cover(mask, unit=False):
    """mask: bool [v, u], 8 x 8.  Yields (u0, v0, w, h) until the mask is empty."""
    mask = mask.copy()
    for _ in range(64):
        if not mask.any():
            return
        v0, u0 = (int(k) for k in np.argwhere(mask)[0])   # row-major: the lowest bit 8 v + u
        w = h = 1
        if not unit:
            while u0 + w < 8 and mask[v0, u0 + w]:
                w += 1
            while v0 + h < 8 and mask[v0 + h, u0:u0 + w].all():
                h += 1
        mask[v0:v0 + h, u0:u0 + w] = False
        yield u0, v0, w, h
    assert not mask.any(), "more than 64 rounds"


def model_mesh_quads(volume, lo=(0, 0, 0), halo=False, unit=False):
    """(quads, record) as bm_host_mesh_quads gives them"""
    volume = np.asarray(volume)
    nz, ny, nx = volume.shape
    extent = (nx, ny, nz)
    first = 1 if halo else 0
    faces = face_arrays(volume, halo)
    # the cells the meshed box spans, per axis, in world cells (Python's // is floor division)
    c0 = [(lo[a] + first) // 8 for a in range(3)]
    c1 = [(lo[a] + extent[a] - first - 1) // 8 for a in range(3)]
    # the face arrays on a grid that starts at the first cell's corner and ends at the last cell's
    origin = [8 * c0[a] - lo[a] for a in range(3)]   # volume index of that corner, <= 0 ... first
    size = [8 * (c1[a] - c0[a] + 1) for a in range(3)]
    grids = []
    for f in faces:
        g = np.zeros((size[2], size[1], size[0]), bool)
        # (with a halo the volume's shell may stick out of the cells of the meshed box: it holds no face)
        a = [max(origin[k], 0) for k in range(3)]
        b = [min(origin[k] + size[k], extent[k]) for k in range(3)]
        g[a[2] - origin[2]:b[2] - origin[2], a[1] - origin[1]:b[1] - origin[1], a[0] - origin[0]:b[0] - origin[0]] = f[a[2]:b[2], a[1]:b[1], a[0]:b[0]]
        grids.append(g)
    quads, total_faces = [], 0
    for cz in range(c1[2] - c0[2] + 1):
        for cy in range(c1[1] - c0[1] + 1):
            for cx in range(c1[0] - c0[0] + 1):
                corner = (8 * (c0[0] + cx), 8 * (c0[1] + cy), 8 * (c0[2] + cz))   # world voxel of the cell's (0, 0, 0)
                for d, (axis, _) in enumerate(DIRECTIONS):
                    block = grids[d][8 * cz:8 * cz + 8, 8 * cy:8 * cy + 8, 8 * cx:8 * cx + 8]
                    if not block.any():
                        continue
                    ua, va = IN_SLICE[axis]
                    for s in range(8):
                        # mask[v, u]: (y, z) -> [z, y] for x; (x, z) -> [z, x] for y; (x, y) -> [y, x] for z
                        mask = (block[:, :, s], block[:, s, :], block[s, :, :])[axis]
                        for u0, v0, w, h in greedy_cover(mask, unit):
                            p = [0, 0, 0]
                            p[axis], p[ua], p[va] = corner[axis] + s, corner[ua] + u0, corner[va] + v0
                            quads.append((p[0], p[1], p[2], d | w << 4 | h << 8))
                            total_faces += w * h
    rec = np.zeros((), RESULT_DTYPE)
    rec["quads"], rec["faces"] = len(quads), total_faces
    return np.array(quads, QUAD_DTYPE).reshape(-1), rec


def paint(quads, lo, shape):
    """six int arrays [z, y, x] over the volume: how many quads cover the face (voxel, direction)"""
    out = [np.zeros(shape, np.int32) for _ in range(6)]
    for q in quads:
        d, w, h = int(q["shape"]) & 15, (int(q["shape"]) >> 4) & 15, (int(q["shape"]) >> 8) & 15
        axis = DIRECTIONS[d][0]
        ua, va = IN_SLICE[axis]
        a = [int(q["x"]) - lo[0], int(q["y"]) - lo[1], int(q["z"]) - lo[2]]
        b = [v + 1 for v in a]
        b[ua], b[va] = a[ua] + w, a[va] + h
        assert min(a) >= 0 and b[0] <= shape[2] and b[1] <= shape[1] and b[2] <= shape[0], "a quad outside the volume"
        out[d][a[2]:b[2], a[1]:b[1], a[0]:b[0]] += 1
    return out


def model_triangles(quads):
    """float32 [2 n, 3, 3]: the plane at c_a (negative direction) or c_a + 1; corners c00, c10 = c00 + w e_u, c11, c01 = c00 + h e_v;
    (c00, c10, c11), (c00, c11, c01) if e_u x e_v points along d, else (c00, c01, c11), (c00, c11, c10)"""
    out = np.zeros((2 * len(quads), 3, 3), np.float32)
    for i, q in enumerate(quads):
        d, w, h = int(q["shape"]) & 15, (int(q["shape"]) >> 4) & 15, (int(q["shape"]) >> 8) & 15
        axis, step = DIRECTIONS[d]
        ua, va = IN_SLICE[axis]
        c00 = np.array([q["x"], q["y"], q["z"]], np.int64)
        c00[axis] += 1 if step > 0 else 0
        eu, ev, n = np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(3, np.int64)
        eu[ua], ev[va], n[axis] = 1, 1, step
        c10, c01 = c00 + w * eu, c00 + h * ev
        c11 = c10 + h * ev
        if np.dot(np.cross(eu, ev), n) > 0:
            out[2 * i], out[2 * i + 1] = (c00, c10, c11), (c00, c11, c01)
        else:
            out[2 * i], out[2 * i + 1] = (c00, c01, c11), (c00, c11, c10)
    return out
