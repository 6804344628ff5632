"""Cost of the travel field (bm_travel_field through bm_debug_travel_times) on the config-2 world (1024^3 voxels, preloaded): the terrain
boxes of distance_time.txt -- 64^3, 256^3 and a 1024 x 1024 x 64 slab, each with the median terrain surface of its columns in its middle --
seeded at the highest empty voxel of the box's middle column, in the air above the surface, and a 256^3 random volume of density 0.3 seeded
at its first open voxel.  Medians of 7 calls after warm-up: set-up, rounds and finish from hipEvents, the number of rounds and of host
looks, ms per round.  Held against, for the same boxes,
  - read_region(device=True): it writes the bytes the field reads -- the floor;
  - distance_field, the sibling;
  - what a caller had before: read_region to the host + bm_host_travel_field (wall clock, once, one thread);
and Scene.find_path end to end across the 64^3 box (wall clock around the call, which waits).  Then the batch size R -- the rounds enqueued
between two looks of the host -- at 4, 16 and 64 on the 256^3 and the 64^3 terrain box.  Device fields are checked against the host's.  No bar is
fixed; the file records the ratios.
The tool runs in steps, each a process of its own, so that each gets a time limit of its own and a step that fails ends the chain:
  timeout -k 10 600 python tools/travel_time.py boxes && timeout -k 10 300 python tools/travel_time.py batch && \\
  timeout -k 10 300 python tools/travel_time.py path && python tools/travel_time.py join      (-> profiles/travel_time.txt)
The steps leave their lines in BM_TRAVEL_TIME_PARTS (default: a directory under the system's temporary one); `join` needs no GPU."""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
STEPS = ("boxes", "batch", "path")
step = sys.argv[1] if len(sys.argv) > 1 else ""
parts = os.environ.get("BM_TRAVEL_TIME_PARTS", os.path.join(tempfile.gettempdir(), "bm_travel_time"))
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if step == "join":
    text = "".join(open(os.path.join(parts, s + ".txt")).read() for s in STEPS)
    out = os.environ.get("BM_TRAVEL_TIME_OUT", os.path.join(root, "profiles", "travel_time.txt"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")
    sys.exit(0)
if step not in STEPS:
    sys.exit(__doc__)
import torch, brickmap_amd as bm
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
G = 1024
scene = bm.Scene(G, G, device=0).generate().preload_all()
stream = torch.cuda.current_stream()
heights = np.block([[scene.column_heights(sx, sy) for sx in range(G // 128)] for sy in range(G // 128)])  # [y, x]
h64, h256, hslab = (int(np.median(heights[y0:y1, x0:x1])) for x0, x1, y0, y1 in ((480, 544, 480, 544), (256, 512, 256, 512), (0, G, 0, G)))
at = lambda h, n: max(0, min(G - n, h - n // 2))  # the box's first slice: the median surface height of its columns in its middle
BOXES = [("64^3", (480, 480, at(h64, 64)), (544, 544, at(h64, 64) + 64)), ("256^3", (256, 256, at(h256, 256)), (512, 512, at(h256, 256) + 256)),
         ("1024 x 1024 x 64 slab", (0, 0, at(hslab, 64)), (1024, 1024, at(hslab, 64) + 64)), ("256^3 random, density 0.3", (0, 0, 0), (256, 256, 256))]
lines = []


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def volume_of(name, lo, hi):
    """(device volume, seed in the box's coordinates, is it a box of the world)"""
    shape = tuple(h - l for l, h in zip(lo, hi))[::-1]
    vox = torch.empty(shape, dtype=torch.uint8, device="cuda")
    if "random" in name:
        host = (np.random.default_rng(1).random(shape) < 0.3).astype(np.uint8)
        vox.copy_(torch.from_numpy(host))
        z, y, x = np.argwhere(host == 0)[0]
        return vox, (int(x), int(y), int(z)), False
    scene.read_region(lo, hi, out=vox, device=True)
    cx, cy = shape[2] // 2, shape[1] // 2
    column = vox[:, cy, cx].cpu().numpy()
    return vox, (cx, cy, int(np.flatnonzero(column == 0).max())), True


def timed(vox, seed, batch=0):
    """medians over the repeats: ([set-up, rounds, finish] ms, rounds, looks, the last TravelField)"""
    out = torch.empty(tuple(vox.shape), dtype=torch.int32, device="cuda")
    seeds = torch.tensor([seed], dtype=torch.int32, device="cuda")
    runs = []
    for i in range(reps + 2):
        field, info = scene.travel_field_times(vox, seeds, out=out, batch=batch)
        if i >= 2:
            runs.append(info)
    ms = [float(np.median([r[0][k] for r in runs])) for k in range(3)]
    return ms, runs[-1][1], runs[-1][2], field


if step == "boxes":
    lines.append(f"config-2 world {G}^3, preloaded; medians of {reps} calls after 2 warm-up calls; device times from hipEvents (the rounds include the host's looks: "
                 f"a 4-byte copy and a wait each); host: one thread, wall clock, once")
    for name, lo, hi in BOXES:
        vox, seed, world = volume_of(name, lo, hi)
        ms, rounds, looks, field = timed(vox, seed)
        total = sum(ms)
        rec = field.record
        lines.append(f"{name} at {lo}, seed {seed}: {int(rec['reached'])} voxels reached of {vox.numel()}; farthest {int(rec['farthest'])} steps at index {int(rec['farthest_at'])}")
        lines.append(f"    bm_travel_field            {total:9.4f} ms   set-up {ms[0]:.4f}  rounds {ms[1]:.4f}  finish {ms[2]:.4f}   {rounds} rounds, {looks} looks, "
                     f"{ms[1] / rounds:.4f} ms per round   ({vox.numel() / total / 1e6:.2f} G voxels / s)")
        dist = []
        for i in range(reps + 2):
            d, dms = scene.distance_field_times(vox)
            dist.append(sum(dms))
        dist = float(np.median(dist[2:]))
        lines.append(f"    bm_distance_field          {dist:9.4f} ms   the sibling; travel_field / distance_field = {total / dist:.2f}")
        if world:
            read = float(np.median([events(lambda: scene.read_region(lo, hi, out=vox, device=True)) for i in range(reps + 2)][2:]))
            lines.append(f"    read_region(device=True)   {read:9.4f} ms   the floor; travel_field / read = {total / read:.2f}")
        t0 = time.perf_counter()
        host = scene.read_region(lo, hi).view(np.uint8) if world else vox.cpu().numpy()
        t1 = time.perf_counter()
        want, want_rec = bm.host_travel_field(host, [seed])
        t2 = time.perf_counter()
        old = (t2 - t0) * 1e3
        assert want_rec == rec and torch.equal(field.field.cpu(), torch.from_numpy(want)), "the device's field is not the host's"
        lines.append(f"    {'read_region' if world else 'copy'} to the host + bm_host_travel_field on one thread   {old:9.1f} ms wall ({(t1 - t0) * 1e3:.1f} + {(t2 - t1) * 1e3:.1f}); "
                     f"old route / travel_field = {old / total:.1f}")
elif step == "batch":
    for name, lo, hi in BOXES[1::-1]:
        vox, seed, _ = volume_of(name, lo, hi)
        best = None
        for batch in (4, 16, 64):
            ms, rounds, looks, field = timed(vox, seed, batch)
            lines.append(f"R = {batch:2d} on the {name} terrain box: rounds {ms[1]:9.4f} ms   {rounds} rounds enqueued, {looks} looks   (set-up {ms[0]:.4f}, finish {ms[2]:.4f})")
            best = (ms[1], batch) if best is None or ms[1] < best[0] else best
        lines.append(f"the best of the three on the {name} terrain box: R = {best[1]}")
    lines.append("the default (kTravelBatch) is the best of the three on the 256^3 terrain box; a round with an empty list costs about a tenth of a look, "
                 "so a larger batch pays for its unneeded rounds where the field is large and loses a little where it needs few rounds")
else:
    name, lo, hi = BOXES[0]
    vox, seed, _ = volume_of(name, lo, hi)
    z = lo[2] + seed[2]
    a, b = (lo[0] + 2, lo[1] + 32, z), (hi[0] - 3, lo[1] + 32, z)
    times = []
    for i in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        path = scene.find_path(a, b, lo, hi)
        times.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"Scene.find_path across the {name} box from {a} to {b}, end to end: {float(np.median(times[2:])):.3f} ms wall "
                 f"({'no path' if path is None else f'{len(path)} voxels'}; read_region, field, the start's value to the host, the walk, the path to the host)")
    lines.append("not measured: clearance_sq > 0 (distance_field and its mask come on top, profiles/distance_time.txt), many seeds, max_steps, volumes beyond 2^26 voxels, "
                 "larger tiles, values staged in LDS, a radius-bounded list (none of them built)")
scene.close()
os.makedirs(parts, exist_ok=True)
with open(os.path.join(parts, step + ".txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
