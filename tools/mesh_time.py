"""Cost of surface extraction (bm_mesh_quads through bm_debug_mesh_times) on the config-2 world (1024^3 voxels, preloaded): boxes of 64^3,
256^3 and a 1024 x 1024 x 64 slab, each with the median terrain surface of its columns in its middle (the boxes of label_time.txt), and a
256^3 random volume of density 0.5, the worst case for the number of quads.  Medians of 7 calls after warm-up.  Per stage, from
hipEvents: count, scan and emit of the emitting call (the buffer sized by a counting call before), and bm_mesh_triangles.  Held against
  - read_region(device=True) of the same box: it reads the same bytes' source and writes the bytes meshing reads -- the floor;
  - what a caller had before: read_region to the host + bm_host_mesh_quads on 16 threads over 16 z-slabs (wall clock, once).
Device quads are checked against the host's where the slabs' cells are the box's cells.  No bar is fixed; the file records the ratios.
usage: python tools/mesh_time.py [repeats]  (-> profiles/mesh_time.txt)"""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
G = 1024
scene = bm.Scene(G, G, device=0).generate().preload_all()
stream = torch.cuda.current_stream()
lines = [f"config-2 world {G}^3, preloaded; medians of {reps} calls after 2 warm-up calls; device times from hipEvents; host: 16 threads, one z-slab each, wall clock, once"]
heights = np.block([[scene.column_heights(sx, sy) for sx in range(G // 128)] for sy in range(G // 128)])  # [y, x]
h64, h256, hslab = (int(np.median(heights[y0:y1, x0:x1])) for x0, x1, y0, y1 in ((480, 544, 480, 544), (256, 512, 256, 512), (0, G, 0, G)))
at = lambda h, n: max(0, min(G - n, h - n // 2))  # the box's first slice: the median surface height of its columns in its middle
BOXES = [("64^3", (480, 480, at(h64, 64)), (544, 544, at(h64, 64) + 64)), ("256^3", (256, 256, at(h256, 256)), (512, 512, at(h256, 256) + 256)),
         ("1024 x 1024 x 64 slab", (0, 0, at(hslab, 64)), (1024, 1024, at(hslab, 64) + 64)), ("256^3 random, density 0.5", (0, 0, 0), (256, 256, 256))]


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def host_slabs(volume, lo):
    """the old route's meshing: 16 z-slabs of the host volume, each meshed with the slices beside it as context, one thread each"""
    nz = volume.shape[0]
    edges = [nz * k // 16 for k in range(17)]

    def one(k):
        z0, z1 = edges[k], edges[k + 1]
        a, b = max(z0 - 1, 0), min(z1 + 1, nz)
        padded = np.zeros((z1 - z0 + 2,) + tuple(s + 2 for s in volume.shape[1:]), np.uint8)   # a shell of empty voxels: the box's sides are closed
        padded[a - z0 + 1:b - z0 + 1, 1:-1, 1:-1] = volume[a:b]
        return bm.host_mesh_quads(padded, (lo[0] - 1, lo[1] - 1, lo[2] + z0 - 1), halo=True)
    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(one, range(16)))


for name, lo, hi in BOXES:
    shape = tuple(h - l for l, h in zip(lo, hi))[::-1]
    random = "random" in name
    vox = torch.empty(shape, dtype=torch.uint8, device="cuda")
    if random:
        vox.copy_(torch.from_numpy((np.random.default_rng(1).random(shape) < 0.5).astype(np.uint8)))
    else:
        scene.read_region(lo, hi, out=vox, device=True)
    n = scene.mesh_quads(vox, lo).count
    stages, tris, read = [], [], []
    for i in range(reps + 2):
        q, ms = scene.mesh_quads_times(vox, lo, capacity=n)
        t = events(lambda: q.triangles())
        r = 0.0 if random else events(lambda: scene.read_region(lo, hi, out=vox, device=True))
        if i >= 2:
            stages.append(ms); tris.append(t); read.append(r)
    count, scan, emit = (float(np.median([s[k] for s in stages])) for k in range(3))
    total, tri, read = count + scan + emit, float(np.median(tris)), float(np.median(read))
    lines.append(f"{name} at {lo}: {int(torch.count_nonzero(vox))} solid voxels of {vox.numel()}; {q.count} quads for {q.faces} faces, {q.faces / max(q.count, 1):.2f} faces per quad")
    lines.append(f"    bm_mesh_quads              {total:9.4f} ms   count {count:.4f}  scan {scan:.4f}  emit {emit:.4f}   ({vox.numel() / total / 1e6:.1f} G voxels / s)")
    lines.append(f"    bm_mesh_triangles          {tri:9.4f} ms   ({2 * q.count} triangles, {72 * q.count / 1e6:.1f} MB)")
    if not random:
        lines.append(f"    read_region(device=True)   {read:9.4f} ms   the floor; mesh_quads / read = {total / read:.2f}")
    t0 = time.perf_counter()
    host = vox.cpu().numpy() if random else scene.read_region(lo, hi).view(np.uint8)
    t1 = time.perf_counter()
    slabs = host_slabs(host, lo)
    t2 = time.perf_counter()
    old = (t2 - t0) * 1e3
    assert sum(int(r["faces"]) for _, r in slabs) == q.faces, "the host counts other faces"
    if shape[0] % 128 == 0 and lo[2] % 8 == 0 and q.count < 5_000_000:   # slabs of whole cells: the same quads as a set
        assert np.array_equal(np.sort(np.concatenate([s for s, _ in slabs]), order=["z", "y", "x", "shape"]), np.sort(q.records, order=["z", "y", "x", "shape"]))
    lines.append(f"    {'copy' if random else 'read_region'} to the host + bm_host_mesh_quads on 16 threads   {old:9.1f} ms wall ({(t1 - t0) * 1e3:.1f} + {(t2 - t1) * 1e3:.1f}); old route / mesh_quads = {old / total:.0f}")
lines.append("not measured: the counting call on its own (it is count + scan of the emitting call), Scene.extract_mesh end to end with torch's allocations, volumes of other densities")
scene.close()
text = "\n".join(lines) + "\n"
print(text, end="")
out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mesh_time.txt")
if os.environ.get("BM_MESH_TIME_OUT"):
    out = os.environ["BM_MESH_TIME_OUT"]
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write(text)
