"""Cost of rigid settling (bm_settle through bm_debug_settle_times) on the config-2 world (1024^3 voxels, preloaded): the 64^3 and 256^3
terrain boxes of distance_time.txt -- each with the median terrain surface of its columns in its middle -- after a carve that detaches
pieces (a moat around the box's inner block down to a cut under the surface, and a second cut that splits the block in two: a stack),
and a 256^3 random volume of density 0.15 written into the world, with every piece that touches no side face chosen.  Medians of 7
calls after warm-up, for the batch size R -- the rounds enqueued between two looks of the host -- at 2, 4 and 8: set-up, rounds and move
from hipEvents, the rounds enqueued and the looks of the host.  Held against, for the same boxes,
  - Scene.components (label_region + label_components), which produces the input: the kernels' hipEvent times and the call's wall clock;
  - write_region(replace) of the output, which applies it;
  - what a caller had before: read_region to the host + bm_host_label_volume + bm_host_settle (wall clock, once, one thread).
Device results are checked against the host's.  No bar is fixed; the file records the ratios.
The tool runs in steps, each a process of its own, so that each gets a time limit of its own and a step that fails ends the chain:
  timeout -k 10 600 python tools/settle_time.py terrain && timeout -k 10 600 python tools/settle_time.py random && \\
  python tools/settle_time.py join      (-> profiles/settle_time.txt)
The steps leave their lines in BM_SETTLE_TIME_PARTS (default: a directory under the system's temporary one); `join` needs no GPU."""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
STEPS = ("terrain", "random")
step = sys.argv[1] if len(sys.argv) > 1 else ""
parts = os.environ.get("BM_SETTLE_TIME_PARTS", os.path.join(tempfile.gettempdir(), "bm_settle_time"))
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if step == "join":
    text = "".join(open(os.path.join(parts, s + ".txt")).read() for s in STEPS)
    out = os.environ.get("BM_SETTLE_TIME_OUT", os.path.join(root, "profiles", "settle_time.txt"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")
    sys.exit(0)
if step not in STEPS:
    sys.exit(__doc__)
import torch, brickmap_amd as bm
from brickmap_amd import settle as st
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
G = 1024
scene = bm.Scene(G, G, device=0).generate().preload_all()
stream = torch.cuda.current_stream()
lines = []


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def carve(lo, hi):
    """detach the inner block of the box above a cut 8 voxels under its middle, and split it by a second cut 6 voxels higher"""
    n = hi[0] - lo[0]
    m, cut = n // 8, lo[2] + n // 2 - 8
    scene.clear_box((lo[0] + m, lo[1] + m, cut), (hi[0] - m, hi[1] - m, cut + 3))
    scene.clear_box((lo[0] + m, lo[1] + m, cut + 9), (hi[0] - m, hi[1] - m, cut + 11))
    for a in (0, 1):
        for side in (0, 1):
            wlo, whi = [lo[0] + m, lo[1] + m, cut], [hi[0] - m, hi[1] - m, hi[2]]
            if side:
                wlo[a] = whi[a] - 2
            else:
                whi[a] = wlo[a] + 2
            scene.clear_box(tuple(wlo), tuple(whi))


def measure(name, lo, hi, anchor):
    walls, kernels = [], []
    for i in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        comps = scene.components(lo, hi)
        walls.append((time.perf_counter() - t0) * 1e3)
        kernels.append(sum(scene.last_label_ms()))
    chosen = comps.loose(anchor)
    lines.append(f"{name} at {lo}: {len(comps)} pieces, {int(chosen.sum())} chosen (no voxel on {', '.join(anchor)}), {int(comps.records['voxels'][chosen].sum())} voxels in them "
                 f"of {int(comps.records['voxels'].sum())} solid, {comps.labels.numel()} in the box")
    best = None
    for batch in (2, 4, 8):
        runs = []
        for i in range(reps + 2):
            done, info = st.settle_times(scene, comps.labels, comps.records, chosen, batch=batch)
            if i >= 2:
                runs.append(info)
        ms = [float(np.median([r[0][k] for r in runs])) for k in range(3)]
        total = sum(ms)
        lines.append(f"    bm_settle, R = {batch}           {total:9.4f} ms   set-up {ms[0]:.4f}  rounds {ms[1]:.4f}  move {ms[2]:.4f}   {runs[-1][1]} rounds enqueued, {runs[-1][2]} looks   "
                     f"({comps.labels.numel() / total / 1e6:.2f} G voxels / s)")
        best = (total, batch) if best is None or total < best[0] else best
    rec = done.record
    lines.append(f"    the best of the three: R = {best[1]}; moved {int(rec['moved_pieces'])} pieces, {int(rec['moved_voxels'])} voxels, largest drop {int(rec['largest_drop'])}, "
                 f"{int(rec['contacts'])} contacts")
    lines.append(f"    Scene.components           {float(np.median(walls[2:])):9.4f} ms wall, of which the label kernels {float(np.median(kernels[2:])):.4f} ms (label_region; the count to the host; "
                 f"label_components; the table to the host): it produces the input")
    t0 = time.perf_counter()
    host = scene.read_region(lo, hi).view(np.uint8)
    t1 = time.perf_counter()
    labels, _ = bm.host_label_volume(host)
    t2 = time.perf_counter()
    want, drops, want_rec = st.host_settle(labels, comps.records, chosen)
    t3 = time.perf_counter()
    assert want_rec.tobytes() == rec.tobytes() and np.array_equal(done.drops, drops) and torch.equal(done.out.cpu(), torch.from_numpy(want)), "the device's result is not the host's"
    old = (t3 - t0) * 1e3
    lines.append(f"    read_region to the host + bm_host_label_volume + bm_host_settle on one thread   {old:9.1f} ms wall ({(t1 - t0) * 1e3:.1f} + {(t2 - t1) * 1e3:.1f} + "
                 f"{(t3 - t2) * 1e3:.1f}); old route / (components + settle) = {old / (float(np.median(walls[2:])) + best[0]):.1f}")
    write = float(np.median([events(lambda: scene.write_region(lo, done.out)) for i in range(reps + 2)][2:]))
    lines.append(f"    write_region(replace)      {write:9.4f} ms   it applies the output")


if step == "terrain":
    lines.append(f"config-2 world {G}^3, preloaded; medians of {reps} calls after 2 warm-up calls; device times from hipEvents (the rounds include the host's looks: "
                 f"a 16-byte copy and a wait each); host: one thread, wall clock, once")
    heights = np.block([[scene.column_heights(sx, sy) for sx in range(G // 128)] for sy in range(G // 128)])  # [y, x]
    h64, h256 = (int(np.median(heights[y0:y1, x0:x1])) for x0, x1, y0, y1 in ((480, 544, 480, 544), (256, 512, 256, 512)))
    at = lambda h, n: max(0, min(G - n, h - n // 2))  # the box's first slice: the median surface height of its columns in its middle
    for name, lo, hi in (("64^3 terrain, carved", (480, 480, at(h64, 64)), (544, 544, at(h64, 64) + 64)),
                         ("256^3 terrain, carved", (256, 256, at(h256, 256)), (512, 512, at(h256, 256) + 256))):
        carve(lo, hi)
        measure(name, lo, hi, ("-x", "+x", "-y", "+y", "-z"))
else:
    volume = torch.from_numpy((np.random.default_rng(1).random((256, 256, 256)) < 0.15).astype(np.uint8)).cuda()
    scene.write_region((0, 0, 0), volume)
    measure("256^3 random, density 0.15", (0, 0, 0), (256, 256, 256), ("-x", "+x", "-y", "+y"))
    lines.append("not measured: slices in flight other than 8 and 16 (DESIGN.md 4.19 has the two), boxes beyond 2^24 voxels, tables kept sorted by first contact, a slot per voxel cached between rounds "
                 "(none of them built)")
scene.close()
os.makedirs(parts, exist_ok=True)
with open(os.path.join(parts, step + ".txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
