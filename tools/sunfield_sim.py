"""CPU estimate of what the sun plane (csrc/sunfield.h) saves the shadow rays of a scene: the oracle renders the frame and reports every
ray (orc_set_ray_probe), and every SHADOW ray is replayed stop by stop -- the reference's move cell by cell, and at every cell the walk
looks a byte up in, what the byte makes of it: a candidate (0; a ray the brick does not stop moves on), the end (255, or the start column's quadrant threshold of csrc/escape.h
on the octant plane), a jump (byte >= BM_JUMP_MIN = 4: on until one axis has moved that many cells) or a single move -- once on the ray's
octant plane of the cube field with the escape rule (what the kernel did before) and once on the sun plane, which
tools/sim/sunfield_plane.cpp builds with the functions of the rule header itself.  A jump that stops at a binade end of tmax (jump.h) is
counted as one jump: both columns are a little low by the same rays.
usage: python tools/sunfield_sim.py [grid_size] [width] [height]   (default: bench config 2's world and camera at 160 x 90, 1 spp, 4 segments)
No GPU.  Rays that start outside the world are skipped and counted."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402

G = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
W = int(sys.argv[2]) if len(sys.argv) > 2 else 160
H = int(sys.argv[3]) if len(sys.argv) > 3 else 90
JUMP_MIN = 4
SUN = (0.05, 0.1)  # FrameParams' default sun_position
oracle.build()
L = oracle.lib()
world = oracle.World(G, G)
world.reset_device(True)
cells, sg = G // 8, G // 128
occ = np.zeros((cells, cells, cells), bool)
for sc in range(world.nsc):
    sx, sy, sz = sc % sg, (sc // sg) % sg, sc // (sg * sg)
    occ[sz * 16:sz * 16 + 16, sy * 16:sy * 16 + 16, sx * 16:sx * 16 + 16] = world.sc_indices(sc).reshape(16, 16, 16) != 0

# the frame's shadow rays
rays = []
PROBE = C.CFUNCTYPE(None, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float))
probe = PROBE(lambda pixel, sample, kind, o, d: rays.append((kind, o[0], o[1], o[2], d[0], d[1], d[2])))
L.orc_set_ray_probe.argtypes, L.orc_set_ray_probe.restype = [PROBE], None
L.orc_set_ray_probe(probe)
world.render(oracle.make_camera((G / 2, G / 8, 0.8 * G), oracle.camera_direction(0.8, -0.5)), oracle.make_frame(W, H, spp=1, max_bounces=3), want_dbg=False)
L.orc_set_ray_probe(PROBE(0))
rays = np.array(rays, np.float32)
total = len(rays)
rays = rays[rays[:, 0] == 1]
mean_dir = rays[:, 4:7].mean(axis=0)
mean_dir /= np.linalg.norm(mean_dir)
spread = np.degrees(np.arccos(np.clip(rays[:, 4:7] @ mean_dir / np.linalg.norm(rays[:, 4:7], axis=1), -1, 1))).max()
print(f"world {G}^3, {W}x{H}, 1 spp, 4 segments: {total} rays, {len(rays)} of them shadow rays around ({mean_dir[0]:.3f}, {mean_dir[1]:.3f}, {mean_dir[2]:.3f}) +- {spread:.2f} degrees")

# ---- the two planes
octant = int(mean_dir[0] < 0) | int(mean_dir[1] < 0) << 1 | int(mean_dir[2] < 0) << 2
assert not octant & 4 and ((rays[:, 4:7] < 0) == (mean_dir < 0)).all(), "the sun plane is for cones inside one octant above the horizon"


def directed(a):  # flip so that the octant's direction is +x +y +z
    for axis in range(3):
        if octant >> axis & 1:
            a = np.flip(a, 2 - axis)
    return a


# the octant plane: edge of the largest empty cube ahead of the cell (csrc/traverse.h "cube-field walk"), cells outside the grid count as full
o_d = directed(occ)
cube = np.zeros((cells + 1,) * 3, np.int64)
for z in range(cells - 1, -1, -1):
    for y in range(cells - 1, -1, -1):
        nb = np.minimum.reduce([cube[z + 1, y + 1, 1:], cube[z + 1, y + 1, :-1], cube[z + 1, y, 1:], cube[z + 1, y, :-1], cube[z, y + 1, 1:], cube[z, y + 1, :-1]])
        row = np.zeros(cells + 1, np.int64)
        for x in range(cells - 1, -1, -1):  # (the x neighbour of the same row is the one dependence a row cannot vectorise)
            row[x] = 0 if o_d[z, y, x] else min(254, 1 + min(nb[x], row[x + 1]))
        cube[z, y] = row
old_plane = directed(cube[:cells, :cells, :cells]).astype(np.uint8)
zz = np.arange(cells).reshape(-1, 1, 1)
top = np.where(occ, zz, -1).max(axis=0)
quad = directed(np.maximum.accumulate(np.maximum.accumulate(directed(top[None])[0][::-1, ::-1], axis=0), axis=1)[::-1, ::-1][None])[0]
with tempfile.TemporaryDirectory() as tmp:
    exe, fin, fout = os.path.join(tmp, "sunfield_plane"), os.path.join(tmp, "occ.bin"), os.path.join(tmp, "plane.bin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "sim", "sunfield_plane.cpp")])
    occ.astype(np.uint8).tofile(fin)
    px, py = SUN[0] * 6.28, (SUN[1] - 0.5) * 3.14
    sun = (np.cos(px) * np.sin(py), np.sin(px) * np.sin(py), np.cos(py))
    extent = 1.0 - np.cos(np.float32(1.5 * np.pi / 180))
    print(subprocess.check_output([exe, str(cells), str(cells), *(repr(float(v)) for v in sun), repr(float(extent)), fin, fout], text=True).strip())
    new_plane = np.fromfile(fout, np.uint8).reshape(cells, cells, cells)
print(f"octant plane: mean byte of the empty cells {old_plane[~occ].mean():.1f}; sun plane: {100 * (new_plane == 255).mean():.1f} % of the cells read 255, mean byte of the rest {new_plane[(new_plane != 255) & ~occ].mean():.1f}; "
      f"mean column top {top.mean():.1f}, mean quadrant threshold {quad.mean():.1f}, mean first stamped cell {np.where(new_plane == 255, zz, cells).min(axis=0).mean():.1f}")


# ---- replay
def replay(o, d, plane, quadrant_rule, loads):
    """stops of one ray by kind: [single moves, jumps, candidates], cells crossed, whether it ended early; loads = cells the reference visits"""
    c = [int(v) for v in o]
    if not all(0 <= v < cells for v in c):
        return None
    sgn = [int(np.sign(v)) for v in d]
    inv = [np.float32(1) / v if v != 0 else np.float32(0) for v in d]
    t = [(np.float32(c[k] + (1 if d[k] > 0 else 0)) - o[k]) * inv[k] if d[k] != 0 else np.float32(1e6) for k in range(3)]
    delta = [np.float32(sgn[k]) * inv[k] for k in range(3)]
    esc = quad[c[1], c[0]] if quadrant_rule else cells
    kinds, visited, budget, ended = [0, 0, 0], 0, None, False
    while visited < loads and all(0 <= v < cells for v in c):
        visited += 1
        if budget is None:  # a stop: the walk reads this cell's byte
            b = int(plane[c[2], c[1], c[0]])
            if b == 255 or c[2] > esc:
                ended = True
                break
            if b == 0:  # the brick is tested; a ray it does not stop moves on by one plain move
                kinds[2] += 1
                kinds[0] += visited < loads
            elif b >= JUMP_MIN:
                kinds[1] += 1
                budget = [b, b, b]
            else:
                kinds[0] += 1
        axis = 0 if t[0] < t[1] and t[0] < t[2] else (1 if t[1] <= t[0] and t[1] < t[2] else 2)
        c[axis] += sgn[axis]
        t[axis] = np.float32(t[axis] + delta[axis])
        if budget is not None:
            budget[axis] -= 1
            if budget[axis] == 0:
                budget = None
    return kinds, visited, ended


cols = {"octant plane + escape rule": (old_plane, True), "sun plane": (new_plane, False)}
res = {k: np.zeros(6) for k in cols}
skipped = 0
campos = [int(v / 8) for v in (G / 2, G / 8, 0.8 * G)]
hits = 0
for r in rays:
    o, d = (r[1:4] / np.float32(8)).astype(np.float32), r[4:7]
    ref = world.intersect_voxel(r[1:4], r[4:7], campos)
    hits += bool(ref.get("hit", 0))
    out = {k: replay(o, d, *v, ref["index_loads"]) for k, v in cols.items()}
    if out["sun plane"] is None:
        skipped += 1
        continue
    for k, (kinds, visited, ended) in out.items():
        res[k] += np.array(kinds + [visited, ended, 1])
print(f"{skipped} rays skipped (start outside), {hits} of the rest occluded; per shadow ray:")
for k, v in res.items():
    n = v[5]
    print(f"  {k:27s}: {v[0] / n:5.2f} single moves + {v[1] / n:5.2f} jumps + {v[2] / n:5.2f} candidates = {(v[0] + v[1] + v[2]) / n:5.2f} stops, {v[3] / n:6.1f} cells crossed, {int(v[4])} rays ended by 255 / escape")
a, b = res["octant plane + escape rule"], res["sun plane"]
print(f"stops removed: {100 * (1 - (b[0] + b[1] + b[2]) / (a[0] + a[1] + a[2])):.1f} %; jump stops {a[1] / a[5]:.2f} -> {b[1] / b[5]:.2f}; cells crossed {a[3] / a[5]:.1f} -> {b[3] / b[5]:.1f}")
