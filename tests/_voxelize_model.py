"""The voxelization contract of bm_voxelize (include/brickmap.h) as a numpy model, an exact clipping truth for its surface rule, and mesh
makers.  The model follows the header's sentences, not the library's loops: tests are masks over whole index ranges, the crossing of a
column is one ceiling division of Python integers, and the parity rule is written for any axis so that x can be checked against y and z."""
from fractions import Fraction

import numpy as np

S = 256
SURFACE, SOLID, KEEP = 1, 2, 1
RESULT_DTYPE = np.dtype([("rejected", "<u4"), ("degenerate", "<u4"), ("open_columns", "<u8")])
CYCLE = {0: (1, 2), 1: (2, 0), 2: (0, 1)}


def snap(triangles, lo):
    """(q [n, 3, 3] int64 -- vertex, axis --, rejected [n] bool): the snap of the header, about the volume origin lo"""
    t = np.asarray(triangles, np.float32).reshape(-1, 3, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        p = t * np.float32(256)
        ok = np.isfinite(p) & (np.abs(p) <= np.float32(2 ** 30))
    q = np.where(ok, np.rint(np.where(ok, p, 0)), 0).astype(np.int64) - 256 * np.asarray(lo, np.int64)[None, None, :]
    good = ok.all(axis=(1, 2)) & (np.abs(q) <= 2 ** 22).all(axis=(1, 2)) & ((q.max(axis=1) - q.min(axis=1)) <= 2 ** 19).all(axis=1)
    return q, ~good


def normal(q):
    return np.cross(q[1] - q[0], q[2] - q[0])


def surface_mask(q, extent):
    """bool [nz, ny, nx]: the voxels one snapped triangle marks (tests 1, 2 and 3)"""
    n = normal(q)
    out = np.zeros(extent[::-1], bool)
    idx = []
    for a in range(3):
        k = np.arange(extent[a], dtype=np.int64)
        idx.append(k[(k * S <= q[:, a].max()) & ((k + 1) * S >= q[:, a].min())])
    if min(len(i) for i in idx) == 0:
        return out
    k = np.meshgrid(idx[0], idx[1], idx[2], indexing="ij")   # k[a][ix, iy, iz]
    d = sum(n[a] * (k[a] * S - q[0][a]) for a in range(3))
    ok = (d + sum(min(n[a] * S, 0) for a in range(3)) <= 0) & (0 <= d + sum(max(n[a] * S, 0) for a in range(3)))
    for ax in range(3):
        u, v = CYCLE[ax]
        sgn = 1 if n[ax] >= 0 else -1
        for i in range(3):
            p0, p1 = q[i], q[(i + 1) % 3]
            a, b = -(p1[v] - p0[v]) * sgn, (p1[u] - p0[u]) * sgn
            ok &= a * (k[u] * S - p0[u]) + b * (k[v] * S - p0[v]) + max(a * S, 0) + max(b * S, 0) >= 0
    ix, iy, iz = np.nonzero(ok)
    out[idx[2][iz], idx[1][iy], idx[0][ix]] = True
    return out


def crossings(q, extent, axis=0):
    """[(u, v, k)]: the columns along `axis` one snapped triangle covers -- (u, v) the cyclic other two axes -- and the crossing's position,
    clamped to 0 ... extent[axis]"""
    n = [int(c) for c in normal(q)]
    if n[axis] == 0:
        return []
    u, v = CYCLE[axis]
    sgn = 1 if n[axis] > 0 else -1
    cu, cv = np.arange(extent[u], dtype=np.int64), np.arange(extent[v], dtype=np.int64)
    cu = cu[(cu * S + 128 >= q[:, u].min()) & (cu * S + 128 <= q[:, u].max())]
    cv = cv[(cv * S + 128 >= q[:, v].min()) & (cv * S + 128 <= q[:, v].max())]
    if len(cu) == 0 or len(cv) == 0:
        return []
    U, V = np.meshgrid(cu * S + 128, cv * S + 128, indexing="ij")
    covered = np.ones(U.shape, bool)
    for i in range(3):
        p0, p1 = q[i], q[(i + 1) % 3]
        a, b = -(p1[v] - p0[v]) * sgn, (p1[u] - p0[u]) * sgn
        E = a * (U - p0[u]) + b * (V - p0[v])
        covered &= (E > 0) | ((E == 0) & ((a > 0) or (a == 0 and b > 0)))
    out = []
    A = abs(n[axis])
    q0 = [int(c) for c in q[0]]
    for iu, iv in zip(*np.nonzero(covered)):
        Uc, Vc = int(U[iu, iv]), int(V[iu, iv])
        R = -sgn * (n[u] * (Uc - q0[u]) + n[v] * (Vc - q0[v]))
        # the smallest x with A (256 x + 128 - q0) >= R
        num, den = R - A * (128 - q0[axis]), 256 * A
        k = -((-num) // den)
        out.append((int(cu[iu]), int(cv[iv]), min(max(k, 0), extent[axis])))
    return out


def solid_volume(qs, extent, axis=0):
    """(bool [nz, ny, nx], open columns): the parity fill of the snapped triangles qs along `axis`"""
    u, v = CYCLE[axis]
    count = np.zeros((extent[u], extent[v], extent[axis] + 1), np.int64)
    for q in qs:
        for cu, cv, k in crossings(q, extent, axis):
            count[cu, cv, k] += 1
    run = np.cumsum(count, axis=2)
    inside = (run[:, :, : extent[axis]] & 1).astype(bool)    # [u, v, axis]
    order = [0, 0, 0]
    order[2 - axis], order[2 - u], order[2 - v] = 2, 0, 1    # -> [z, y, x]
    return np.transpose(inside, order), int((run[:, :, -1] & 1).sum())


def model_voxelize(triangles, lo, shape, mode=SURFACE | SOLID, keep=False, volume=None):
    """(volume uint8 [nz, ny, nx], record): what bm_voxelize leaves; `volume`: what the volume held (for keep)"""
    extent = tuple(int(v) for v in shape[::-1])
    q, rejected = snap(triangles, lo)
    rec = np.zeros((), RESULT_DTYPE)
    rec["rejected"] = rejected.sum()
    live = []
    for i in range(len(q)):
        if rejected[i]:
            continue
        if not normal(q[i]).any():
            rec["degenerate"] += 1
            continue
        live.append(q[i])
    bits = np.zeros(tuple(shape), bool)
    if mode & SURFACE:
        for t in live:
            bits |= surface_mask(t, extent)
    if mode & SOLID:
        inside, open_columns = solid_volume(live, extent, 0)
        bits |= inside
        rec["open_columns"] = open_columns
    out = bits.astype(np.uint8)
    if keep:
        out = out | np.asarray(volume, np.uint8)
    return out, rec


# ---- the truth of the surface rule: exact clipping (Sutherland-Hodgman in rationals) of the triangle against the voxel's closed cube
def triangle_meets_cube(q, k):
    poly = [tuple(Fraction(int(c)) for c in p) for p in q]
    for a in range(3):
        for bound, sign in ((k[a] * S, 1), ((k[a] + 1) * S, -1)):    # keep sign * (p_a - bound) >= 0
            if not poly:
                return False
            nxt = []
            for i, p in enumerate(poly):
                r = poly[(i + 1) % len(poly)]
                dp, dr = sign * (p[a] - bound), sign * (r[a] - bound)
                if dp >= 0:
                    nxt.append(p)
                if (dp > 0 and dr < 0) or (dp < 0 and dr > 0):
                    s = dp / (dp - dr)
                    nxt.append(tuple(p[c] + s * (r[c] - p[c]) for c in range(3)))
            poly = nxt
    return bool(poly)


def clipping_truth(triangles, lo, shape):
    """uint8 [nz, ny, nx]: 1 where a snapped, non-degenerate triangle meets the voxel's closed cube"""
    q, rejected = snap(triangles, lo)
    out = np.zeros(tuple(shape), np.uint8)
    nz, ny, nx = shape
    for i in range(len(q)):
        if rejected[i] or not normal(q[i]).any():
            continue
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    if not out[z, y, x] and triangle_meets_cube(q[i], (x, y, z)):
                        out[z, y, x] = 1
    return out


# ---- meshes: float32 [n, 3, 3], consistently oriented where closed
def box_mesh(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.array([[lo[0] if not i & 1 else hi[0], lo[1] if not i & 2 else hi[1], lo[2] if not i & 4 else hi[2]] for i in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # outward
    faces = [f for a, b, cc, d in quads for f in ((a, b, cc), (a, cc, d))]
    return c[np.array(faces)].astype(np.float32)


def icosphere(center, radius, subdivisions):
    """20 * 4^subdivisions triangles; (vertices float64 [m, 3] on the unit sphere, faces) are shared by every centre and radius"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.asarray(center, np.float64)[None, :] + radius * np.array(v)
    return verts[np.array(f)].astype(np.float32)


def torus(center, major, minor, nu=24, nv=12):
    """a torus around the z axis through `center`: 2 nu nv triangles"""
    a = 2 * np.pi * np.arange(nu) / nu
    b = 2 * np.pi * np.arange(nv) / nv
    A, B = np.meshgrid(a, b, indexing="ij")
    p = np.stack(((major + minor * np.cos(B)) * np.cos(A), (major + minor * np.cos(B)) * np.sin(A), minor * np.sin(B)), axis=-1) + np.asarray(center, np.float64)
    tris = []
    for i in range(nu):
        for j in range(nv):
            i1, j1 = (i + 1) % nu, (j + 1) % nv
            tris += [(p[i, j], p[i1, j], p[i1, j1]), (p[i, j], p[i1, j1], p[i, j1])]
    return np.array(tris).astype(np.float32)


def open_hemisphere(center, radius, subdivisions):
    """the triangles of the icosphere whose centroid lies on the +x side: a bowl that opens towards -x, so columns along x cross it once"""
    t = icosphere(center, radius, subdivisions)
    return t[t.mean(axis=1)[:, 0] > center[0]]


def quarter_triangles(seed, n, lo, hi):
    """n random triangles with coordinates in quarter voxels inside [lo, hi)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(4 * lo, 4 * hi, size=(n, 3, 3)) / 4.0).astype(np.float32)
