"""Cost of ground navigation (bm_foot_room, and bm_foot_field through bm_debug_foot_times) on the config-2 world (1024^3 voxels,
preloaded): the terrain boxes of distance_time.txt -- 64^3, 256^3 and a 1024 x 1024 x 64 slab, each with the median terrain surface of its
columns in its middle -- seeded at the ground of the box's middle column, for an agent of height 2, climb 1, drop 3.  Medians of 7 calls
after warm-up: the room bytes, then set-up, rounds and finish from hipEvents, the rounds enqueued and the looks of the host.  Held against,
for the same boxes,
  - read_region(device=True): it writes the bytes the room kernel reads;
  - bm_travel_field from the same seed, the sibling that flies;
  - what a caller had before: read_region to the host + bm_host_foot_room + bm_host_foot_field (wall clock, once, one thread).
Then the batch size R -- the rounds enqueued between two looks of the host -- at 4, 16 and 64 on the 64^3 and the 256^3 box.  Device results
are checked against the host's.  No bar is fixed; the file records the ratios.
The tool runs in steps, each a process of its own, so that each gets a time limit of its own and a step that fails ends the chain:
  timeout -k 10 600 python tools/foot_time.py boxes && timeout -k 10 300 python tools/foot_time.py batch && \\
  python tools/foot_time.py join      (-> profiles/foot_time.txt)
The steps leave their lines in BM_FOOT_TIME_PARTS (default: a directory under the system's temporary one); `join` needs no GPU."""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
STEPS = ("boxes", "batch")
step = sys.argv[1] if len(sys.argv) > 1 else ""
parts = os.environ.get("BM_FOOT_TIME_PARTS", os.path.join(tempfile.gettempdir(), "bm_foot_time"))
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if step == "join":
    text = "".join(open(os.path.join(parts, s + ".txt")).read() for s in STEPS)
    out = os.environ.get("BM_FOOT_TIME_OUT", os.path.join(root, "profiles", "foot_time.txt"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")
    sys.exit(0)
if step not in STEPS:
    sys.exit(__doc__)
import torch, brickmap_amd as bm
from brickmap_amd import foot
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
G = 1024
AGENT = dict(height=2, climb=1, drop=3)
scene = bm.Scene(G, G, device=0).generate().preload_all()
stream = torch.cuda.current_stream()
heights = np.block([[scene.column_heights(sx, sy) for sx in range(G // 128)] for sy in range(G // 128)])  # [y, x]
h64, h256, hslab = (int(np.median(heights[y0:y1, x0:x1])) for x0, x1, y0, y1 in ((480, 544, 480, 544), (256, 512, 256, 512), (0, G, 0, G)))
at = lambda h, n: max(0, min(G - n, h - n // 2))  # the box's first slice: the median surface height of its columns in its middle
BOXES = [("64^3", (480, 480, at(h64, 64)), (544, 544, at(h64, 64) + 64)), ("256^3", (256, 256, at(h256, 256)), (512, 512, at(h256, 256) + 256)),
         ("1024 x 1024 x 64 slab", (0, 0, at(hslab, 64)), (1024, 1024, at(hslab, 64) + 64))]
lines = []


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn):
    return float(np.median([events(fn) for i in range(reps + 2)][2:]))


def box_of(lo, hi):
    """(device volume, its room bytes, the seed: the ground of the middle column)"""
    vox = scene.read_region(lo, hi, device=True)
    room = foot.foot_room(scene, vox, floor=lo[2] == 0)
    nz, ny, nx = vox.shape
    (seed,) = foot.ground(room, [(nx // 2, ny // 2, nz - 1)], AGENT["height"])
    return vox, room, seed


def timed(room, seed, batch=0):
    """medians over the repeats: ([set-up, rounds, finish] ms, rounds, looks, the last FootField)"""
    out = torch.empty(tuple(room.shape), dtype=torch.int32, device="cuda")
    seeds = torch.tensor([seed], dtype=torch.int32, device="cuda")
    runs = []
    for i in range(reps + 2):
        field, info = foot.foot_field_times(scene, room, seeds, out=out, batch=batch, **AGENT)
        if i >= 2:
            runs.append(info)
    return [float(np.median([r[0][k] for r in runs])) for k in range(3)], runs[-1][1], runs[-1][2], field


if step == "boxes":
    lines.append(f"config-2 world {G}^3, preloaded; agent {AGENT}; medians of {reps} calls after 2 warm-up calls; device times from hipEvents (the rounds include the host's "
                 f"looks: a 4-byte copy and a wait each); host: one thread, wall clock, once")
    for name, lo, hi in BOXES:
        vox, room, seed = box_of(lo, hi)
        read = median_ms(lambda: scene.read_region(lo, hi, out=vox, device=True))
        room_ms = median_ms(lambda: foot.foot_room(scene, vox, floor=lo[2] == 0))
        ms, rounds, looks, field = timed(room, seed)
        rec = field.record
        total = room_ms + sum(ms)
        lines.append(f"{name} at {lo}, seeded at {seed}: {int(rec['standable'])} stands, {int(rec['reached'])} reached, farthest {int(rec['farthest'])}, {vox.numel()} voxels")
        lines.append(f"    bm_foot_room               {room_ms:9.4f} ms   ({vox.numel() / room_ms / 1e6:.2f} G voxels / s)")
        lines.append(f"    bm_foot_field              {sum(ms):9.4f} ms   set-up {ms[0]:.4f}  rounds {ms[1]:.4f}  finish {ms[2]:.4f}   {rounds} rounds enqueued, {looks} looks, "
                     f"{ms[1] / rounds * 1e3:.2f} us per round")
        lines.append(f"    read_region(device=True)   {read:9.4f} ms   it writes the bytes the room kernel reads")
        flying = torch.tensor([seed], dtype=torch.int32, device="cuda")
        travel = [scene.travel_field_times(vox, flying)[1] for i in range(reps + 2)][2:]
        tms = [float(np.median([r[0][k] for r in travel])) for k in range(3)]
        lines.append(f"    bm_travel_field, same seed {sum(tms):9.4f} ms   set-up {tms[0]:.4f}  rounds {tms[1]:.4f}  finish {tms[2]:.4f}   {travel[-1][1]} rounds enqueued, {travel[-1][2]} looks; "
                     f"room + walk field / travel field = {total / sum(tms):.2f}")
        t0 = time.perf_counter()
        host = scene.read_region(lo, hi).view(np.uint8)
        t1 = time.perf_counter()
        h_room = foot.host_foot_room(host, floor=lo[2] == 0)
        t2 = time.perf_counter()
        h_field, h_rec = foot.host_foot_field(h_room, [seed], **AGENT)
        t3 = time.perf_counter()
        assert torch.equal(room.cpu(), torch.from_numpy(h_room)) and torch.equal(field.field.cpu(), torch.from_numpy(h_field)) and h_rec.tobytes() == rec.tobytes(), \
            "the device's result is not the host's"
        old = (t3 - t0) * 1e3
        lines.append(f"    read_region to the host + bm_host_foot_room + bm_host_foot_field on one thread   {old:9.1f} ms wall ({(t1 - t0) * 1e3:.1f} + {(t2 - t1) * 1e3:.1f} + "
                     f"{(t3 - t2) * 1e3:.1f}); host route / (read_region + room + field on the device) = {old / (read + total):.1f}")
else:
    for name, lo, hi in BOXES[:2]:
        vox, room, seed = box_of(lo, hi)
        for batch in (4, 16, 64):
            ms, rounds, looks, field = timed(room, seed, batch)
            lines.append(f"{name}, R = {batch:2d}: bm_foot_field {sum(ms):9.4f} ms   set-up {ms[0]:.4f}  rounds {ms[1]:.4f}  finish {ms[2]:.4f}   {rounds} rounds enqueued, {looks} looks "
                         f"(farthest {int(field.record['farthest'])})")
    lines.append("not built, so not measured: the variant of foot_level in which one workgroup advances several levels of a small front by itself (a front in LDS, workgroup "
                 "barriers in between); a grid of a round other than 1024 waves; heights in flight other than 4")
scene.close()
os.makedirs(parts, exist_ok=True)
with open(os.path.join(parts, step + ".txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
