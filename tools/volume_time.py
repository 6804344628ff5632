"""Cost of the volume queries (bm_scene_query_volumes) on the config-2 world (1024^3 voxels, preloaded), medians after warm-up:
(a) one 256^3 aligned box: the query against read_region(..., device=True) of the same box -- what a caller had to run before any
    reduction -- and against the whole old route, read + torch.count_nonzero; the calls alternated;
(b) one million character-sized boxes (6 x 6 x 14 voxels) at random positions near the terrain surface, plain and with BM_VOLUME_ANY;
(c) the whole world as one box and as one sphere: time and effective bytes per second (one cube-field byte per cell, one index word
    and 64 brick bytes per brick).
Device times: torch.cuda events around the calls.  usage: python tools/volume_time.py [repeats]  (-> profiles/volume_time.txt)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
G, N = 1024, 1_000_000
scene = bm.Scene(G, G, device=0).generate().preload_all()
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)
heights = np.block([[scene.column_heights(sx, sy) for sx in range(G // 128)] for sy in range(G // 128)])  # [y, x]


def device_records(recs):
    return torch.from_numpy(recs.view(np.uint8).reshape(-1, 48)).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    out = fn()
    b.record(stream)
    return a, b, out


def median_ms(fns, reps):
    """medians of the device times of the calls `fns`, alternated"""
    for _ in range(5):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        events = [timed(fn) for fn in fns]
        torch.cuda.synchronize()
        for t, (a, b, _) in zip(times, events):
            t.append(a.elapsed_time(b))
    return [float(np.median(t)) for t in times]


def query(recs, flags=0):
    n = recs.shape[0]
    res = torch.empty((n, 40), dtype=torch.uint8, device="cuda")
    return (lambda: scene.query_volumes_raw(n, recs.data_ptr(), res.data_ptr(), flags, stream.cuda_stream)), res


solid_of = lambda res: res[:, 0:8].view(torch.int64).reshape(-1)
print(f"config-2 world {G}^3, preloaded; medians of {reps} runs after 5 warm-up rounds; device times from events around the calls")
# ---- (a)
lo, hi = (256, 256, 0), (512, 512, 256)
box = device_records(bm.volume_box(lo, hi))
out = torch.empty((256, 256, 256), dtype=torch.uint8, device="cuda")
q, res = query(box)
read = lambda: scene.read_region(lo, hi, out=out, device=True)
count = [None]
def old_route():
    read()
    count[0] = torch.count_nonzero(out)
tq, tr, to = median_ms([q, read, old_route], reps)
torch.cuda.synchronize()
assert int(solid_of(res)[0]) == int(count[0]), "the query and the old route disagree"
print(f"(a) one 256^3 aligned box at {lo} ({int(count[0])} solid voxels):")
print(f"    bm_scene_query_volumes              {tq:8.4f} ms")
print(f"    read_region(device=True)            {tr:8.4f} ms   (bar: query <= read; ratio {tq / tr:.2f})")
print(f"    read_region + torch.count_nonzero   {to:8.4f} ms")
# ---- (b)
x, y = rng.integers(0, G - 6, N), rng.integers(0, G - 6, N)
z = np.clip(heights[y, x].astype(np.int64) + rng.integers(-6, 10, N), 0, G - 14)
p = np.stack([x, y, z], -1)
chars = device_records(bm.volume_box(p, p + (6, 6, 14)))
qp, resp = query(chars)
qa, resa = query(chars, bm.BM_VOLUME_ANY)
tp, ta = median_ms([qp, qa], reps)
torch.cuda.synchronize()
blocked = solid_of(resp) > 0
assert torch.equal(blocked, solid_of(resa) > 0), "BM_VOLUME_ANY disagrees with the count"
print(f"(b) {N} boxes of 6 x 6 x 14 voxels within -6 ... +9 voxels of the terrain surface ({float(blocked.float().mean()) * 100:.1f} % touch something):")
print(f"    plain                               {tp:8.4f} ms   {N / tp / 1e6:7.3f} G queries/s")
print(f"    BM_VOLUME_ANY                       {ta:8.4f} ms   {N / ta / 1e6:7.3f} G queries/s   speed-up {tp / ta:.2f}")
print("    (for orientation only: bm_scene_cast_rays answers about 3 Grays/s on this world, profiles/query_time.txt)")
# ---- (c)
info = scene.info()
bytes_read = (G // 8) ** 3 + info["total_bricks"] * (4 + 64)
world = device_records(bm.volume_box((0, 0, 0), (G, G, G)))
ball = device_records(bm.volume_sphere((G // 2, G // 2, G // 2), G))
qw, resw = query(world)
qs, ress = query(ball)
tw, ts = median_ms([qw, qs], reps)
torch.cuda.synchronize()
assert int(solid_of(resw)[0]) == int(solid_of(ress)[0]), "the sphere that holds the world counts what the box counts"
print(f"(c) the whole world ({info['total_bricks']} bricks, {int(solid_of(resw)[0])} solid voxels; {bytes_read / 1e6:.1f} MB of field bytes, index words and bricks):")
print(f"    as one box                          {tw:8.4f} ms   {bytes_read / tw / 1e6:7.1f} GB/s")
print(f"    as one sphere of radius {G}        {ts:8.4f} ms   {bytes_read / ts / 1e6:7.1f} GB/s")
scene.close()
