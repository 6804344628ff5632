"""CPU estimate of what the walk's escape rule (csrc/escape.h) saves on a scene, before anything is built for it: the oracle renders the
frame and reports every ray (orc_set_ray_probe), orc_intersect_voxel says how many cells the reference visits for it, and the visits are
replayed cell by cell (the reference's move, vectorised over the rays) against three rules:
  global   above the highest occupied cell of the world, not moving down (below the lowest, moving down)
  start    the threshold of the ray's octant at the column it STARTS in, looked up once (what the kernel does)
  ideal    the threshold at the column the ray is in, looked up in every cell
usage: python tools/escape_sim.py [grid_size] [width] [height]      (default: bench config 2's world and camera at 240 x 135, 1 spp, 4 segments)
No GPU.  Rays that start outside the world are walked from where they enter it by the reference; here they are skipped and counted."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402

G = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
W = int(sys.argv[2]) if len(sys.argv) > 2 else 240
H = int(sys.argv[3]) if len(sys.argv) > 3 else 135
oracle.build()
L = oracle.lib()
world = oracle.World(G, G)
world.reset_device(True)
cells = G // 8
sg = G // 128

# occupancy [z, y, x] over brick cells and the table [8, y, x] (the definition of csrc/escape.h, as running maxima / minima)
occ = np.zeros((cells, cells, cells), bool)
for sc in range(world.nsc):
    sx, sy, sz = sc % sg, (sc // sg) % sg, sc // (sg * sg)
    occ[sz * 16:sz * 16 + 16, sy * 16:sy * 16 + 16, sx * 16:sx * 16 + 16] = world.sc_indices(sc).reshape(16, 16, 16) != 0
zz = np.arange(cells).reshape(-1, 1, 1)
top, bottom = np.where(occ, zz, -1).max(axis=0), np.where(occ, zz, cells).min(axis=0)
table = np.zeros((8, cells, cells), np.int32)
for o in range(8):
    a, fold = (bottom, np.minimum) if o & 4 else (top, np.maximum)
    fx, fy = (slice(None), slice(None, None, -1)) if not o & 1 else (slice(None), slice(None)), (slice(None, None, -1), slice(None)) if not o & 2 else (slice(None), slice(None))
    a = fold.accumulate(fold.accumulate(a[fx][fy], axis=0), axis=1)[fy][fx]
    table[o] = a

# the frame's rays
rays = []
PROBE = C.CFUNCTYPE(None, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float))
probe = PROBE(lambda pixel, sample, kind, o, d: rays.append((kind, o[0], o[1], o[2], d[0], d[1], d[2])))
L.orc_set_ray_probe.argtypes, L.orc_set_ray_probe.restype = [PROBE], None
position = (G / 2, G / 8, 0.8 * G)
direction = oracle.camera_direction(0.8, -0.5)
L.orc_set_ray_probe(probe)
world.render(oracle.make_camera(position, direction), oracle.make_frame(W, H, spp=1, max_bounces=3), want_dbg=False)
L.orc_set_ray_probe(PROBE(0))
rays = np.array(rays, np.float32)
campos = [int(v / 8) for v in position]
loads = np.array([world.intersect_voxel(r[1:4], r[4:7], campos)["index_loads"] for r in rays], np.int64)

# replay: the reference's set-up (voxel.cuh:160-189) for origins inside the world, then its move, for every ray at once
o, d = rays[:, 1:4] / np.float32(8), rays[:, 4:7]
inside = ((rays[:, 1:4] > 0) & (rays[:, 1:4] < G)).all(axis=1)
c = o.astype(np.int32)
sgn = np.sign(d).astype(np.int32)
with np.errstate(divide="ignore", invalid="ignore"):
    inv = np.where(d == 0, np.float32(0), np.float32(1) / d).astype(np.float32)
cb = np.where(d > 0, c + 1, c).astype(np.float32)
t = np.where(d != 0, (cb - o) * inv, np.float32(1e6)).astype(np.float32)
delta = (sgn * inv).astype(np.float32)
octant = (d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4
down = d[:, 2] < 0
cc = np.clip(c, 0, cells - 1)
start_e = table[octant, cc[:, 1], cc[:, 0]]
glob_e = np.where(down, bottom.min(), top.max())
first = {k: np.full(len(rays), -1, np.int64) for k in ("global", "start", "ideal")}
n = np.zeros(len(rays), np.int64)
live = inside & (loads > 0)
while live.any():
    i = np.nonzero(live)[0]
    z = c[i, 2]
    e_ideal = table[octant[i], np.clip(c[i, 1], 0, cells - 1), np.clip(c[i, 0], 0, cells - 1)]
    for k, e in (("global", glob_e[i]), ("start", start_e[i]), ("ideal", e_ideal)):
        esc = np.where(down[i], z < e, z > e) & (first[k][i] < 0)
        first[k][i[esc]] = n[i[esc]]
    n[i] += 1
    tx, ty, tz = t[i, 0], t[i, 1], t[i, 2]
    mx = (tx < ty) & (tx < tz)
    my = (ty <= tx) & (ty < tz)
    axis = np.where(mx, 0, np.where(my, 1, 2))
    c[i, axis] += sgn[i, axis]
    t[i, axis] += delta[i, axis]
    live[i] = n[i] < loads[i]

visits = int(loads[inside].sum())
kinds = rays[:, 0].astype(int)
print(f"world {G}^3, {W}x{H}, 1 spp, 4 segments: {len(rays)} rays ({int((kinds == 0).sum())} extend, {int((kinds == 1).sum())} shadow), "
      f"{int((~inside).sum())} skipped (start outside), {visits} reference cell visits = {visits / max(1, inside.sum()):.1f} per ray")
print(f"occupied cells z = {int(np.nonzero(occ)[0].min())} ... {int(top.max())}; camera in cell z = {campos[2]}; column tops {int(top.min())} ... {int(top.max())}, mean {top.mean():.1f}")
for k in ("global", "start", "ideal"):
    f = first[k]
    ended = f >= 0
    after = int((loads[ended] - f[ended]).sum())
    print(f"{k:7s}: {int(ended.sum()):7d} rays ended early ({100 * ended.sum() / len(rays):.1f} %), {int((f == 0).sum()):6d} at set-up, "
          f"{after:9d} cell visits after the escape point = {100 * after / max(1, visits):.1f} % of all")
