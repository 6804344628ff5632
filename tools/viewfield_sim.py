"""CPU estimate of what the view plane (csrc/viewfield.h) saves the primary rays of a scene: the oracle renders the frame and reports every
ray (orc_set_ray_probe), and every PRIMARY ray is replayed stop by stop -- the reference's move cell by cell, and at every cell the walk
looks a byte up in, what the byte makes of it: a candidate (0; a ray the brick does not stop moves on), the end (255, or the start
column's quadrant threshold of csrc/escape.h, tested where the kernel tests it on either plane: at set-up and where a jump lands), a
jump (byte >= BM_JUMP_MIN = 4: on until one axis has moved that many cells, or to the binade end of the smallest tmax, as jump.h cuts
it) or a single move -- once on the ray's octant plane of the cube field with the escape rule (what the kernel did before) and once on
the view plane, which tools/sim/viewfield_plane.cpp builds with the functions of the rule header itself.  Bounce and shadow rays do not
read the plane; their numbers are the octant plane's (shadow rays: without the sun plane and the shadow heights, tools/sunfield_sim.py).
usage: python tools/viewfield_sim.py [grid_size] [width] [height] [x y z of the camera]
(default: bench config 2's world and camera at 160 x 90, 1 spp, 4 segments).  No GPU."""
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
POS = tuple(float(v) for v in sys.argv[4:7]) if len(sys.argv) > 6 else (G / 2, G / 8, 0.8 * G)
JUMP_MIN = 4
oracle.build()
L = oracle.lib()
world = oracle.World(G, G)
world.reset_device(True)
cells, sg = G // 8, G // 128
occ = np.zeros((cells, cells, cells), bool)
for sc in range(world.nsc):
    sx, sy, sz = sc % sg, (sc // sg) % sg, sc // (sg * sg)
    occ[sz * 16:sz * 16 + 16, sy * 16:sy * 16 + 16, sx * 16:sx * 16 + 16] = world.sc_indices(sc).reshape(16, 16, 16) != 0

rays = []
PROBE = C.CFUNCTYPE(None, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float))
probe = PROBE(lambda pixel, sample, kind, o, d: rays.append((kind, o[0], o[1], o[2], d[0], d[1], d[2])))
L.orc_set_ray_probe.argtypes, L.orc_set_ray_probe.restype = [PROBE], None
L.orc_set_ray_probe(probe)
world.render(oracle.make_camera(POS, oracle.camera_direction(0.8, -0.5)), oracle.make_frame(W, H, spp=1, max_bounces=3), want_dbg=False)
L.orc_set_ray_probe(PROBE(0))
rays = np.array(rays, np.float32)
origin = np.array(POS, np.float32)
primary = (rays[:, 0] == 0) & (rays[:, 1:4] == origin).all(axis=1)
kind_of = np.where(primary, 0, np.where(rays[:, 0] == 1, 2, 1))  # 0 primary, 1 bounce, 2 shadow
print(f"world {G}^3, {W}x{H}, 1 spp, 4 segments, camera {POS}: {len(rays)} rays: {int((kind_of == 0).sum())} primary, {int((kind_of == 1).sum())} bounce, {int((kind_of == 2).sum())} shadow")

with tempfile.TemporaryDirectory() as tmp:
    exe, fin, fout = os.path.join(tmp, "viewfield_plane"), os.path.join(tmp, "occ.bin"), os.path.join(tmp, "plane.bin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "sim", "viewfield_plane.cpp")])
    occ.astype(np.uint8).tofile(fin)
    print(subprocess.check_output([exe, str(cells), str(cells), *(repr(float(v)) for v in POS), fin, fout], text=True).strip())
    raw = np.fromfile(fout, np.uint8)
n3 = cells ** 3
view = raw[:n3].reshape(cells, cells, cells)
octants = raw[n3:9 * n3].reshape(8, cells, cells, cells)
thresholds = raw[9 * n3:].view(np.int32)
empty = ~occ
print(f"view plane: {100 * (view == 255).mean():.1f} % of the cells read 255; of the other empty cells, mean byte {view[empty & (view != 255)].mean():.1f}, "
      f"{100 * (view[empty & (view != 255)] > octants.max(axis=0)[empty & (view != 255)]).mean():.1f} % above every octant's byte")


def exponent(t):
    return int(np.float32(t).view(np.uint32)) >> 23


def replay(o, d, plane, escape_rule, loads):
    """stops of one ray: [single moves, jumps, candidates, jumps cut at a binade end, stops before the first candidate], cells visited"""
    c = [int(v) for v in o]
    if not all(0 <= v < cells for v in c):
        return None
    sgn = [int(np.sign(v)) for v in d]
    inv = [np.float32(1) / v if v != 0 else np.float32(0) for v in d]
    t = [(np.float32(c[k] + (1 if d[k] > 0 else 0)) - o[k]) * inv[k] if d[k] != 0 else np.float32(1e6) for k in range(3)]
    delta = [np.float32(sgn[k]) * inv[k] for k in range(3)]
    octant = int(d[0] < 0) | int(d[1] < 0) << 1 | int(d[2] < 0) << 2
    esc = int(thresholds[octant])
    escaped = (lambda z: z < esc) if octant & 4 else (lambda z: z > esc)
    kinds, visited, budget, binade, landing, first_cand = [0, 0, 0, 0, 0], 0, None, 0, True, False
    while visited < loads and all(0 <= v < cells for v in c):
        visited += 1
        if budget is None:  # a stop: the walk reads this cell's byte
            b = int(plane[octant][c[2], c[1], c[0]]) if plane.ndim == 4 else int(plane[c[2], c[1], c[0]])
            if b == 255 or (escape_rule and landing and escaped(c[2])):
                break
            landing = False
            if not first_cand:
                kinds[4] += 1
            if b == 0:  # the brick is tested; a ray it does not stop moves on by one plain move
                kinds[2] += 1
                first_cand = True
                kinds[0] += visited < loads
            else:
                m = min(t)
                if b >= JUMP_MIN and 117 <= exponent(m) < 146:  # jump_possible: 2^-10 <= tmax < 2^19
                    kinds[1] += 1
                    budget, binade = [b, b, b], exponent(m)
                else:
                    kinds[0] += 1
        axis = 0 if t[0] < t[1] and t[0] < t[2] else (1 if t[1] <= t[0] and t[1] < t[2] else 2)
        c[axis] += sgn[axis]
        t[axis] = np.float32(t[axis] + delta[axis])
        if budget is not None:
            budget[axis] -= 1
            if budget[axis] == 0:
                budget, landing = None, True
            elif exponent(min(t)) != binade:  # the next move is past the binade end: the jump stops here, inside its cube
                budget, landing = None, True
                kinds[3] += 1
    return kinds, visited


cols = {"octant plane + escape rule": (octants, True), "view plane + escape rule": (view, True)}
res = {k: np.zeros(7) for k in cols}
others = np.zeros((3, 7))
campos = [int(v / 8) for v in POS]
skipped = 0
for r, kind in zip(rays, kind_of):
    o, d = (r[1:4] / np.float32(8)).astype(np.float32), r[4:7]
    loads = world.intersect_voxel(r[1:4], r[4:7], campos)["index_loads"]
    base = replay(o, d, octants, True, loads)
    if base is None:
        skipped += 1
        continue
    others[kind] += np.array(base[0] + [base[1], 1])
    if kind == 0:
        res["octant plane + escape rule"] += np.array(base[0] + [base[1], 1])
        new = replay(o, d, view, True, loads)
        res["view plane + escape rule"] += np.array(new[0] + [new[1], 1])
print(f"{skipped} rays skipped (start outside); per ray, on the octant planes:")
for k, name in enumerate(("primary", "bounce", "shadow")):
    v = others[k]
    n = max(v[6], 1)
    print(f"  {name:8s}: {int(v[6]):8d} rays, {(v[0] + v[1] + v[2]) / n:5.2f} stops = {v[0] / n:5.2f} single moves + {v[1] / n:5.2f} jumps ({v[3] / n:4.2f} cut at a binade end) + {v[2] / n:4.2f} candidates")
print("per primary ray:")
for k, v in res.items():
    n = max(v[6], 1)
    print(f"  {k:27s}: {v[0] / n:5.2f} single moves + {v[1] / n:5.2f} jumps ({v[3] / n:4.2f} cut at a binade end) + {v[2] / n:5.2f} candidates = {(v[0] + v[1] + v[2]) / n:5.2f} stops, "
          f"{v[4] / n:5.2f} before the first candidate, {v[5] / n:6.1f} cells visited")
a, b = res["octant plane + escape rule"], res["view plane + escape rule"]
sa, sb, tot = a[0] + a[1] + a[2], b[0] + b[1] + b[2], (others[:, 0] + others[:, 1] + others[:, 2]).sum()
print(f"stops removed: {100 * (1 - sb / sa):.1f} % of the primary rays' ({sa / a[6]:.2f} -> {sb / b[6]:.2f}), {100 * (sa - sb) / tot:.1f} % of the frame's (shadow rays on their octant planes)")
