"""Cost of the spill-level field (bm_water_field through bm_debug_water_times) on the config-2 world (1024^3 voxels, preloaded): the terrain
boxes of travel_time.txt -- 64^3, 256^3 and a 1024 x 1024 x 64 slab, each with the median terrain surface of its columns in its middle --
with their four sides open, and a 256^3 random volume of density 0.6.  Medians of 7 calls after warm-up, at batch sizes 16 and 64 (the
rounds enqueued between two looks of the host): set-up, rounds and finish from hipEvents, the number of rounds, of host looks and of tile
visits (a visit is a tile listed in a round), visits per tile.  Held against, for the same bytes,
  - travel_field, seeded where travel_time.txt seeds it (the highest empty voxel of the box's middle column; the random volume's first
    open voxel), whose kernels these are modelled on;
  - what a caller had before: read_region to the host + bm_host_water_field (wall clock, once, one thread).
Device fields are checked against the host's.  No bar is fixed; the file records the ratios.
The tool runs in steps, each a process of its own, so that each gets a time limit of its own and a step that fails ends the chain:
  timeout -k 10 600 python tools/water_time.py small && timeout -k 10 600 python tools/water_time.py large && \\
  python tools/water_time.py join      (-> profiles/water_time.txt)
The steps leave their lines in BM_WATER_TIME_PARTS (default: a directory under the system's temporary one); `join` needs no GPU."""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
STEPS = ("small", "large")
step = sys.argv[1] if len(sys.argv) > 1 else ""
parts = os.environ.get("BM_WATER_TIME_PARTS", os.path.join(tempfile.gettempdir(), "bm_water_time"))
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if step == "join":
    text = "".join(open(os.path.join(parts, s + ".txt")).read() for s in STEPS)
    out = os.environ.get("BM_WATER_TIME_OUT", os.path.join(root, "profiles", "water_time.txt"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")
    sys.exit(0)
if step not in STEPS:
    sys.exit(__doc__)
import torch, brickmap_amd as bm
from brickmap_amd import water
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
G = 1024
scene = bm.Scene(G, G, device=0).generate().preload_all()
heights = np.block([[scene.column_heights(sx, sy) for sx in range(G // 128)] for sy in range(G // 128)])  # [y, x]
h64, h256, hslab = (int(np.median(heights[y0:y1, x0:x1])) for x0, x1, y0, y1 in ((480, 544, 480, 544), (256, 512, 256, 512), (0, G, 0, G)))
at = lambda h, n: max(0, min(G - n, h - n // 2))  # the box's first slice: the median surface height of its columns in its middle
BOXES = {"small": [("64^3", (480, 480, at(h64, 64)), (544, 544, at(h64, 64) + 64)), ("256^3", (256, 256, at(h256, 256)), (512, 512, at(h256, 256) + 256))],
         "large": [("1024 x 1024 x 64 slab", (0, 0, at(hslab, 64)), (1024, 1024, at(hslab, 64) + 64)), ("256^3 random, density 0.6", (0, 0, 0), (256, 256, 256))]}[step]
lines = []


def volume_of(name, lo, hi):
    """(device volume, travel's seed in the box's coordinates, is it a box of the world)"""
    shape = tuple(h - l for l, h in zip(lo, hi))[::-1]
    vox = torch.empty(shape, dtype=torch.uint8, device="cuda")
    if "random" in name:
        host = (np.random.default_rng(1).random(shape) < 0.6).astype(np.uint8)
        vox.copy_(torch.from_numpy(host))
        z, y, x = np.argwhere(host == 0)[0]
        return vox, (int(x), int(y), int(z)), False
    scene.read_region(lo, hi, out=vox, device=True)
    cx, cy = shape[2] // 2, shape[1] // 2
    column = vox[:, cy, cx].cpu().numpy()
    return vox, (cx, cy, int(np.flatnonzero(column == 0).max())), True


def medians(call):
    """medians over the repeats of ([set-up, rounds, finish] ms, counts ...), and the last result"""
    runs = []
    for i in range(reps + 2):
        field, info = call()
        if i >= 2:
            runs.append(info)
    return [float(np.median([r[0][k] for r in runs])) for k in range(3)], runs[-1][1:], field


if step == "small":
    lines.append(f"config-2 world {G}^3, preloaded; medians of {reps} calls after 2 warm-up calls; device times from hipEvents (the rounds include the host's looks: "
                 f"a 4-byte copy and a wait each, the first of them before round 1); host: one thread, wall clock, once; R = the rounds enqueued between two looks")
for name, lo, hi in BOXES:
    vox, seed, world = volume_of(name, lo, hi)
    out = torch.empty(tuple(vox.shape), dtype=torch.int32, device="cuda")
    tiles = int(np.prod([(n + 7) // 8 for n in vox.shape]))
    best = None
    for batch in (16, 64):
        ms, (rounds, looks, visits), field = medians(lambda: water.water_field_times(scene, vox, out=out, batch=batch))
        total = sum(ms)
        if batch == 16:
            rec = field.record
            lines.append(f"{name} at {lo}, sides open: {int(rec['wet'])} wet and {int(rec['closed'])} closed voxels of {vox.numel()}; deepest {int(rec['deepest'])} at index {int(rec['deepest_at'])}")
        lines.append(f"    bm_water_field, R = {batch:2d}     {total:9.4f} ms   set-up {ms[0]:.4f}  rounds {ms[1]:.4f}  finish {ms[2]:.4f}   {rounds} rounds, {looks} looks, "
                     f"{visits} tile visits = {visits / tiles:.2f} per tile   ({vox.numel() / total / 1e6:.2f} G voxels / s)")
        best = (total, batch) if best is None or total < best[0] else best
    seeds = torch.tensor([seed], dtype=torch.int32, device="cuda")
    tms, (trounds, tlooks), _ = medians(lambda: scene.travel_field_times(vox, seeds, out=out))
    travel = sum(tms)
    lines.append(f"    bm_travel_field, seed {seed}  {travel:9.4f} ms   set-up {tms[0]:.4f}  rounds {tms[1]:.4f}  finish {tms[2]:.4f}   {trounds} rounds, {tlooks} looks "
                 f"(its door counts no visits); water_field (R = {best[1]}) / travel_field = {best[0] / travel:.2f}")
    field = water.water_field(scene, vox)
    t0 = time.perf_counter()
    host = scene.read_region(lo, hi).view(np.uint8) if world else vox.cpu().numpy()
    t1 = time.perf_counter()
    want, want_rec = water.host_water_field(host)
    t2 = time.perf_counter()
    old = (t2 - t0) * 1e3
    assert want_rec == field.record and torch.equal(field.field.cpu(), torch.from_numpy(want)), "the device's field is not the host's"
    lines.append(f"    {'read_region' if world else 'copy'} to the host + bm_host_water_field on one thread   {old:9.1f} ms wall ({(t1 - t0) * 1e3:.1f} + {(t2 - t1) * 1e3:.1f}); "
                 f"old route / water_field = {old / best[0]:.1f}")
    if name == "256^3":
        lines.append(f"the better of R = 16 and R = 64 on the {name} terrain box: R = {best[1]}")
if step == "large":
    lines.append("the default batch stays kTravelBatch = 64, the better of the two on the 256^3 terrain box (by less than the spread between runs; R = 16 is the better one "
                 "on the 64^3 box, where a batch of 64 is mostly rounds with an empty list)")
    lines.append("visits: a tile that is reached is visited once, and again whenever a neighbour's face value falls after that; bm_travel_field's door counts none, so there "
                 "is no ratio -- on the terrain boxes 1.6 to 1.8 visits per tile is close to that floor, on the random volume a tile is visited 6 times: lower levels arrive "
                 "late by detours and tiles settle again.  What that suggests, and was not built: rounds ordered by level (a tile waits until no lower level is pending), "
                 "as the host's buckets do")
    lines.append("not measured: drains, a sea level, open top or bottom faces, volumes beyond 2^26 voxels, bm_water_mask (one pass: a load and a byte store per voxel)")
scene.close()
os.makedirs(parts, exist_ok=True)
with open(os.path.join(parts, step + ".txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
