"""Cost of the distance field (bm_distance_field through bm_debug_distance_times, and bm_distance_mask) on the config-2 world (1024^3
voxels, preloaded): the boxes of mesh_time.txt -- 64^3, 256^3 and a 1024 x 1024 x 64 slab, each with the median terrain surface of its
columns in its middle -- a 256^3 random volume of density 0.5, and a 256^3 volume with a single source, the longest envelopes.  Medians of 7
calls after warm-up.  Per pass, from hipEvents: x, y, z + finish; and the mask at radius_sq 9.  Held against
  - read_region(device=True) of the same box: it writes the bytes the field reads -- the floor;
  - what a caller had before: read_region to the host + bm_host_distance_field (wall clock, once, ONE thread: the host routine has no door
    for a single pass, so the slabs of a 16-thread run cannot be formed from outside it).
Then Scene.grow and Scene.shrink of the 64^3 box at radius_sq 9, end to end (wall clock around a synchronise; the box is restored).
Device fields are checked against the host's.  No bar is fixed; the file records the ratios.
usage: python tools/distance_time.py [repeats]  (-> profiles/distance_time.txt)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
G = 1024
scene = bm.Scene(G, G, device=0).generate().preload_all()
stream = torch.cuda.current_stream()
lines = [f"config-2 world {G}^3, preloaded; medians of {reps} calls after 2 warm-up calls; device times from hipEvents; host: one thread, wall clock, once"]
heights = np.block([[scene.column_heights(sx, sy) for sx in range(G // 128)] for sy in range(G // 128)])  # [y, x]
h64, h256, hslab = (int(np.median(heights[y0:y1, x0:x1])) for x0, x1, y0, y1 in ((480, 544, 480, 544), (256, 512, 256, 512), (0, G, 0, G)))
at = lambda h, n: max(0, min(G - n, h - n // 2))  # the box's first slice: the median surface height of its columns in its middle
BOXES = [("64^3", (480, 480, at(h64, 64)), (544, 544, at(h64, 64) + 64)), ("256^3", (256, 256, at(h256, 256)), (512, 512, at(h256, 256) + 256)),
         ("1024 x 1024 x 64 slab", (0, 0, at(hslab, 64)), (1024, 1024, at(hslab, 64) + 64)), ("256^3 random, density 0.5", (0, 0, 0), (256, 256, 256)),
         ("256^3 single source", (0, 0, 0), (256, 256, 256))]


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


for name, lo, hi in BOXES:
    shape = tuple(h - l for l, h in zip(lo, hi))[::-1]
    world = "random" not in name and "single" not in name
    vox = torch.empty(shape, dtype=torch.uint8, device="cuda")
    if "random" in name:
        vox.copy_(torch.from_numpy((np.random.default_rng(1).random(shape) < 0.5).astype(np.uint8)))
    elif "single" in name:
        vox.zero_()
        vox[0, 0, 0] = 1
    else:
        scene.read_region(lo, hi, out=vox, device=True)
    out = torch.empty(shape, dtype=torch.int32, device="cuda")
    mask = torch.empty(shape, dtype=torch.uint8, device="cuda")
    stages, masks, read = [], [], []
    for i in range(reps + 2):
        d, ms = scene.distance_field_times(vox, out=out)
        m = events(lambda: d.mask(9, out=mask))
        r = events(lambda: scene.read_region(lo, hi, out=vox, device=True)) if world else 0.0
        if i >= 2:
            stages.append(ms); masks.append(m); read.append(r)
    x, y, z = (float(np.median([s[k] for s in stages])) for k in range(3))
    total, m, read = x + y + z, float(np.median(masks)), float(np.median(read))
    rec = d.record
    lines.append(f"{name} at {lo}: {int(rec['sources'])} solid voxels of {vox.numel()}; largest empty ball: radius_sq {int(rec['max_sq'])} at index {int(rec['max_at'])}")
    lines.append(f"    bm_distance_field          {total:9.4f} ms   x {x:.4f}  y {y:.4f}  z + finish {z:.4f}   ({vox.numel() / total / 1e6:.1f} G voxels / s)")
    lines.append(f"    bm_distance_mask           {m:9.4f} ms")
    if world:
        lines.append(f"    read_region(device=True)   {read:9.4f} ms   the floor; distance_field / read = {total / read:.2f}")
    t0 = time.perf_counter()
    host = scene.read_region(lo, hi).view(np.uint8) if world else vox.cpu().numpy()
    t1 = time.perf_counter()
    want, want_rec = bm.host_distance_field(host)
    t2 = time.perf_counter()
    old = (t2 - t0) * 1e3
    assert want_rec == rec and torch.equal(out.cpu(), torch.from_numpy(want)), "the device's field is not the host's"
    lines.append(f"    {'read_region' if world else 'copy'} to the host + bm_host_distance_field on one thread   {old:9.1f} ms wall ({(t1 - t0) * 1e3:.1f} + {(t2 - t1) * 1e3:.1f}); old route / distance_field = {old / total:.0f}")

name, lo, hi = BOXES[0]
before = scene.read_region(lo, hi, device=True)
for op in ("grow", "shrink"):
    times = []
    for i in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        changed = getattr(scene, op)(lo, hi, 9)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        scene.write_region(lo, before)
    lines.append(f"Scene.{op} of the {name} box at radius_sq 9, end to end: {float(np.median(times[2:])):.3f} ms wall ({changed} voxels changed; read of a 70^3 box, field, mask, write, a count with torch)")
lines.append("not measured: the host routine on 16 threads over slabs (it has no door for a single pass), to='empty' and outside=True (the same kernels; the flag "
             "changes one comparison and one minimum), volumes beyond 2^26 voxels, rows of 32 voxels and fewer, stacks staged in LDS (not built)")
scene.close()
text = "\n".join(lines) + "\n"
print(text, end="")
out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "distance_time.txt")
if os.environ.get("BM_DISTANCE_TIME_OUT"):
    out = os.environ["BM_DISTANCE_TIME_OUT"]
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write(text)
