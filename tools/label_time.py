"""Cost of connected-component labelling (bm_scene_label_region, bm_scene_label_components) on the config-2 world (1024^3 voxels,
preloaded): boxes of 64^3, 256^3 and a 1024 x 1024 x 64 slab, each with the median terrain
surface of its columns in its middle, medians of 7 calls after warm-up.  Per stage, from hipEvents: local, merge,
flatten (bm_scene_last_label_ms) and components (events around the call).  Held against
  - read_region(device=True) of the same box: the floor -- it reads the same bricks and writes a quarter of the bytes;
  - what a caller had to do before, where scipy is present: read_region to the host + scipy.ndimage.label (wall clock).
No bar is fixed; the file records the ratios.  usage: python tools/label_time.py [repeats]  (-> profiles/label_time.txt)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
try:
    from scipy import ndimage
except ImportError:
    ndimage = None
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
G = 1024
scene = bm.Scene(G, G, device=0).generate().preload_all()
stream = torch.cuda.current_stream()
lines = [f"config-2 world {G}^3, preloaded; medians of {reps} calls after 2 warm-up calls; device times from hipEvents; scipy {'present' if ndimage else 'absent'}"]
heights = np.block([[scene.column_heights(sx, sy) for sx in range(G // 128)] for sy in range(G // 128)])  # [y, x]
h64, h256, hslab = (int(np.median(heights[y0:y1, x0:x1])) for x0, x1, y0, y1 in ((480, 544, 480, 544), (256, 512, 256, 512), (0, G, 0, G)))
at = lambda h, n: max(0, min(G - n, h - n // 2))  # the box's first slice: the median surface height of its columns in its middle
BOXES = [("64^3", (480, 480, at(h64, 64)), (544, 544, at(h64, 64) + 64)), ("256^3", (256, 256, at(h256, 256)), (512, 512, at(h256, 256) + 256)),
         ("1024 x 1024 x 64 slab", (0, 0, at(hslab, 64)), (1024, 1024, at(hslab, 64) + 64))]


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


for name, lo, hi in BOXES:
    shape = tuple(h - l for l, h in zip(lo, hi))[::-1]
    labels = torch.empty(shape, dtype=torch.int32, device="cuda")
    vox = torch.empty(shape, dtype=torch.uint8, device="cuda")
    stages, total, comp, read = [], [], [], []
    for i in range(reps + 2):
        t = events(lambda: scene.label_region(lo, hi, out=labels))
        _, count = scene.label_region(lo, hi, out=labels)
        torch.cuda.synchronize()
        n = int(count.item())
        table = torch.empty((max(n, 1), 5), dtype=torch.int64, device="cuda")
        c = events(lambda: scene.label_components_raw(lo, hi, labels.data_ptr(), table.data_ptr(), n, stream.cuda_stream))
        r = events(lambda: scene.read_region(lo, hi, out=vox, device=True))
        if i >= 2:
            stages.append(scene.last_label_ms()); total.append(t); comp.append(c); read.append(r)
    local, merge, flatten = (float(np.median([s[k] for s in stages])) for k in range(3))
    total, comp, read = float(np.median(total)), float(np.median(comp)), float(np.median(read))
    solid = int(torch.count_nonzero(labels))
    lines.append(f"{name} at {lo}: {solid} solid voxels of {labels.numel()}, {n} components")
    lines.append(f"    label_region               {total:9.4f} ms   local {local:.4f}  merge {merge:.4f}  flatten {flatten:.4f}")
    lines.append(f"    label_components           {comp:9.4f} ms   ({n} records)")
    lines.append(f"    read_region(device=True)   {read:9.4f} ms   the floor; label_region / read = {total / read:.2f}, with components {(total + comp) / read:.2f}")
    if ndimage:
        t0 = time.perf_counter()
        host = scene.read_region(lo, hi)
        t1 = time.perf_counter()
        _, m = ndimage.label(host)
        t2 = time.perf_counter()
        assert m == n, "scipy counts other components"
        old = (t2 - t0) * 1e3
        lines.append(f"    read_region to the host + scipy.ndimage.label   {old:9.1f} ms wall ({(t1 - t0) * 1e3:.1f} + {(t2 - t1) * 1e3:.1f}); old route / (label_region + components) = {old / (total + comp):.0f}")
    else:
        lines.append("    read_region to the host + scipy.ndimage.label: not measured (scipy absent)")
scene.close()
text = "\n".join(lines) + "\n"
print(text, end="")
out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "label_time.txt")
if os.environ.get("BM_LABEL_TIME_OUT"):
    out = os.environ["BM_LABEL_TIME_OUT"]
with open(out, "w") as f:
    f.write(text)
