"""CPU estimate of what shadow heights (csrc/shadowheight.h) save the shadow rays of a scene, in the manner of tools/sunfield_sim.py: the
oracle renders the frame and reports every ray, and every SHADOW ray is replayed stop by stop on the sun plane (what the kernel does
today), once as it is and once with the rule: a ray whose start cell is below its column's dark height ends at set-up, with no stop at all.
The last lines say, per path segment, how many shadow rays the rule ends: what the test in the shade block (shadow_origin) never draws.
tools/sim/sunfield_plane.cpp and tools/sim/shadowheight_slice.cpp build the plane and the dark heights with the functions of the rule
headers themselves.  Every ray the rule ends must be occluded in the reference's own trace, or the run fails.
usage: python tools/shadowheight_sim.py [grid_size] [width] [height]   (default: bench config 2's world and camera at 160 x 90, 1 spp, 4 segments)
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
full = np.zeros((cells, cells, cells), bool)
for sc in range(world.nsc):
    sx, sy, sz = sc % sg, (sc // sg) % sg, sc // (sg * sg)
    idx = world.sc_indices(sc)
    bricks = world.sc_bricks(sc)
    is_full = np.zeros(4096, bool)
    nz = np.flatnonzero(idx)
    if len(nz):
        is_full[nz] = (bricks[idx[nz] & 0xFFF] == 0xFFFFFFFF).all(axis=1)
    box = np.s_[sz * 16:sz * 16 + 16, sy * 16:sy * 16 + 16, sx * 16:sx * 16 + 16]
    occ[box] = idx.reshape(16, 16, 16) != 0
    full[box] = is_full.reshape(16, 16, 16)

rays = []
PROBE = C.CFUNCTYPE(None, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float))
segment = {}  # (pixel, sample) -> extend rays of the path so far: a shadow ray belongs to segment count - 1


def on_ray(pixel, sample, kind, o, d):
    if kind == 0:
        segment[(pixel, sample)] = segment.get((pixel, sample), 0) + 1
    rays.append((kind, o[0], o[1], o[2], d[0], d[1], d[2], segment.get((pixel, sample), 1) - 1))


probe = PROBE(on_ray)
L.orc_set_ray_probe.argtypes, L.orc_set_ray_probe.restype = [PROBE], None
L.orc_set_ray_probe(probe)
world.render(oracle.make_camera((G / 2, G / 8, 0.8 * G), oracle.camera_direction(0.8, -0.5)), oracle.make_frame(W, H, spp=1, max_bounces=3), want_dbg=False)
L.orc_set_ray_probe(PROBE(0))
rays = np.array(rays, np.float32)
total = len(rays)
rays = rays[rays[:, 0] == 1]
print(f"world {G}^3, {W}x{H}, 1 spp, 4 segments: {total} rays, {len(rays)} of them shadow rays; {100 * full.mean():.1f} % of the cells are full bricks, {100 * (occ & ~full).mean():.1f} % partly filled")

with tempfile.TemporaryDirectory() as tmp:
    px, py = SUN[0] * 6.28, (SUN[1] - 0.5) * 3.14
    sun = (np.cos(px) * np.sin(py), np.sin(px) * np.sin(py), np.cos(py))
    extent = 1.0 - np.cos(np.float32(1.5 * np.pi / 180))
    args = [str(cells), str(cells), *(repr(float(v)) for v in sun), repr(float(extent))]
    out = {}
    for name, grid in (("sunfield_plane", occ), ("shadowheight_slice", full)):
        exe, fin, fout = os.path.join(tmp, name), os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "sim", name + ".cpp")])
        grid.astype(np.uint8).tofile(fin)
        print(subprocess.check_output([exe, *args, fin, fout], text=True).strip())
        out[name] = np.fromfile(fout, np.uint8 if name == "sunfield_plane" else np.int32)
    plane = out["sunfield_plane"].reshape(cells, cells, cells)
    zd = out["shadowheight_slice"].reshape(cells, cells)
zz = np.arange(cells).reshape(-1, 1, 1)
top = np.where(occ, zz, -1).max(axis=0)
dark = zz < zd[None]
assert not (dark & (plane == 255)).any(), "a cell stamped 255 is dark"
print(f"mean column top {top.mean():.1f}, mean full top {np.cumprod(full, axis=0).sum(axis=0).mean():.1f}, mean dark height {zd.mean():.1f}; {100 * (zd > top).mean():.1f} % of the columns are dark up to their top cell")


def replay(o, d, loads):
    """stops of one ray on the sun plane by kind: [single moves, jumps, candidates]; loads = cells the reference visits"""
    c = [int(v) for v in o]
    if not all(0 <= v < cells for v in c):
        return None
    sgn = [int(np.sign(v)) for v in d]
    inv = [np.float32(1) / v if v != 0 else np.float32(0) for v in d]
    t = [(np.float32(c[k] + (1 if d[k] > 0 else 0)) - o[k]) * inv[k] if d[k] != 0 else np.float32(1e6) for k in range(3)]
    delta = [np.float32(sgn[k]) * inv[k] for k in range(3)]
    kinds, visited, budget = [0, 0, 0], 0, None
    while visited < loads and all(0 <= v < cells for v in c):
        visited += 1
        if budget is None:
            b = int(plane[c[2], c[1], c[0]])
            if b == 255:
                break
            if b == 0:
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
    return kinds


before, after = np.zeros(3), np.zeros(3)
SEGMENTS = 4
drawn_by_segment, ended_by_segment = np.zeros(SEGMENTS, int), np.zeros(SEGMENTS, int)
n = skipped = hits = ended = ended_hits = 0
campos = [int(v / 8) for v in (G / 2, G / 8, 0.8 * G)]
for r in rays:
    o, d = (r[1:4] / np.float32(8)).astype(np.float32), r[4:7]
    ref = world.intersect_voxel(r[1:4], r[4:7], campos)
    kinds = replay(o, d, ref["index_loads"])
    if kinds is None:
        skipped += 1
        continue
    n += 1
    hit = bool(ref.get("hit", 0))
    hits += hit
    before += kinds
    c = [int(v) for v in o]
    seg = min(int(r[7]), SEGMENTS - 1)
    drawn_by_segment[seg] += 1
    if c[2] < zd[c[1], c[0]]:
        ended += 1
        ended_by_segment[seg] += 1
        ended_hits += hit
        assert hit, f"the rule ends a ray that reaches the sun: origin {r[1:4]}, direction {r[4:7]}"
    else:
        after += kinds
print(f"{skipped} rays skipped (start outside), {hits} of the other {n} occluded")
print(f"ended at set-up: {ended} rays = {100 * ended / n:.1f} % of the shadow rays, {100 * ended_hits / max(hits, 1):.1f} % of the occluded ones (all {ended_hits} of them occluded in the reference)")
for k, v in (("sun plane", before), ("sun plane + shadow heights", after)):
    print(f"  {k:27s}: {v[0] / n:5.2f} single moves + {v[1] / n:5.2f} jumps + {v[2] / n:5.2f} candidates = {v.sum() / n:5.2f} stops per shadow ray")
print(f"stops removed: {100 * (1 - after.sum() / before.sum()):.1f} %; candidates removed: {100 * (1 - after[2] / before[2]):.1f} %")
# what ending these rays where they are DRAWN (the shade block, csrc/shadowheight.h shadow_origin) takes out of the scheduler: each is one ray set-up, one
# ST_CONN wait and one visit of a second shade pass; a ray of the path's last segment lets its lane start the next path in the same pass, any other
# lets it set up its bounce ray one pass earlier.  (Which of them an idle lane would have taken is the scheduler's business: tools/ring_stats.py counts
# connect lanes on the GPU.)
print(f"never drawn with the test in the shade block: {ended} of {n} shadow rays = {100 * ended / max(total, 1):.1f} % of all {total} rays")
for k in range(SEGMENTS):
    print(f"  segment {k}: {ended_by_segment[k]:6d} of {drawn_by_segment[k]:6d} shadow rays" + ("   (the path ends in the shade pass)" if k == SEGMENTS - 1 else "   (the bounce ray is set up one pass earlier)"))
