"""Cost of mesh voxelization (bm_voxelize, Scene.write_mesh) into a 256^3 volume, for three meshes: an icosphere of radius 120 at
subdivision 6 (81 920 small triangles), the same sphere at subdivision 2 (320 large triangles) and 10^6 sub-voxel triangles; mode
solid+surface, medians of 7 calls after 2 warm-up calls.  Per shape:
  - the stages from bm_debug_voxelize_times (hipEvents between them): zeroing the workspace, plan + scan, surface items, solid items, dense pass;
  - the whole call (events around Scene.voxelize into a given volume), held against
      bm_host_voxelize on 16 threads (16 slabs of 16 slices, one call each: slabs are independent by the contract) -- what a caller has today;
      a hipMemsetAsync of the volume's bytes -- the floor of the dense pass;
  - Scene.write_mesh end to end (wall clock, the host waits) against Scene.write_region alone of the finished volume, both on a scene that
    already holds the mesh (a region write that changes nothing still packs, copies and merges).
No bar is fixed; the file records the ratios.  usage: python tools/voxelize_time.py [repeats]  (-> profiles/voxelize_time.txt)"""
import ctypes as C, os, sys, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
N = 256


def icosphere(center, radius, subdivisions):
    t = (1 + 5 ** 0.5) / 2
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in
         [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(center, np.float64) + radius * np.array(v))[np.array(f)].astype(np.float32)


rng = np.random.default_rng(1)
tiny = (rng.uniform(1, N - 1, size=(1_000_000, 1, 3)) + rng.uniform(-0.4, 0.4, size=(1_000_000, 3, 3))).astype(np.float32)
MESHES = [("icosphere r 120, subdivision 6", icosphere((128.3, 127.9, 128.2), 120, 6)), ("icosphere r 120, subdivision 2", icosphere((128.3, 127.9, 128.2), 120, 2)),
          ("10^6 sub-voxel triangles", tiny)]
scene = bm.Scene.from_voxels(np.zeros((N, N, N), np.uint8))
L = scene._L
stream = torch.cuda.current_stream()
med = lambda xs: float(np.median(xs))


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host16(tri):
    out = np.zeros((N, N, N), np.uint8)
    with ThreadPoolExecutor(16) as pool:
        recs = list(pool.map(lambda k: bm.host_voxelize(tri, (0, 0, 16 * k), out=out[16 * k:16 * k + 16])[1], range(16)))
    return out, sum(int(r["open_columns"]) for r in recs)


lines = [f"{N}^3 volume, mode solid+surface; medians of {reps} calls after 2 warm-up calls; device times from hipEvents, wall times with the host waiting"]
for name, tri in MESHES:
    d_tri = torch.from_numpy(tri).cuda()
    vol = torch.empty((N, N, N), dtype=torch.uint8, device="cuda")
    stages, total, zero, mesh, region, host = [], [], [], [], [], []
    for i in range(reps + 2):
        _, res, ms = scene.voxelize_times(d_tri, (0, 0, 0), out=vol)
        t = events(lambda: scene.voxelize(d_tri, (0, 0, 0), out=vol))
        z = events(lambda: bm._lib.check(L.bm_buffer_zero(0, C.c_void_p(vol.data_ptr()), vol.numel(), C.c_void_p(stream.cuda_stream))))
        scene.voxelize(d_tri, (0, 0, 0), out=vol)
        lo, hi, _ = scene.write_mesh(d_tri)
        wm = wall(lambda: scene.write_mesh(d_tri))
        wr = wall(lambda: scene.write_region(lo, vol[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]], op="set"))  # the same box, already voxelized
        if i >= 2:
            stages.append(ms); total.append(t); zero.append(z); mesh.append(wm); region.append(wr)
    for i in range(3):
        t0 = time.perf_counter()
        want, open_columns = host16(tri)
        host.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(vol.cpu().numpy(), want) and res.open_columns == open_columns, "device and host differ"
    st = [med([s[k] for s in stages]) for k in range(5)]
    total, zero, mesh, region, host = med(total), med(zero), med(mesh), med(region), med(host)
    lines.append(f"{name}: {len(tri)} triangles, {int(want.sum())} voxels set, open columns {open_columns}, rejected {res.rejected}")
    lines.append(f"    stages                     zero {st[0]:.4f}  plan+scan {st[1]:.4f}  surface {st[2]:.4f}  solid {st[3]:.4f}  dense {st[4]:.4f} ms  (sum {sum(st):.4f})")
    lines.append(f"    voxelize                   {total:9.4f} ms")
    lines.append(f"    bm_host_voxelize, 16 threads {host:7.1f} ms wall; host / device = {host / total:.0f}")
    lines.append(f"    hipMemsetAsync of 16 MiB   {zero:9.4f} ms; voxelize / memset = {total / zero:.1f}, dense pass / memset = {st[4] / zero:.1f}")
    lines.append(f"    write_mesh end to end      {mesh:9.3f} ms wall; write_region alone {region:.3f} ms wall; write_mesh / write_region = {mesh / region:.2f}")
scene.close()
text = "\n".join(lines) + "\n"
print(text, end="")
out = os.environ.get("BM_VOXELIZE_TIME_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "voxelize_time.txt")
with open(out, "w") as f:
    f.write(text)
