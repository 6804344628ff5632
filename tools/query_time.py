"""Cost of the ray queries (bm_scene_cast_rays) on the config-2 world (1024^3 voxels, preloaded), one run after warm-up:
(a) the 1920x1080 pixel-centre rays of bench.py's config-2 camera against a BM_FLAG_PRIMARY_ONLY 1080p / 1 spp frame of the same camera
    (bm_render_frame: the same number of first-hit rays), the calls alternated -- the rays in row order, and the same rays stored in
    tile order (16x16 tiles of 8x8 blocks: what a wave takes is a block of neighbouring pixels, as in the frame);
(b) 2,073,600 incoherent rays -- seeded random origins above the terrain, random directions -- in Grays/s;
(c) the host-visible latency of a one-ray Scene.pick;
plus the record traffic (32 B in, 32 B out per ray) over the kernel time.  Device times: torch.cuda events around the calls, medians.
usage: python tools/query_time.py [repeats]  (-> profiles/query_time.txt)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
G, W, H = 1024, 1920, 1080
N = W * H
scene = bm.Scene(G, G, device=0).generate().preload_all()
cam = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
frame = bm.FrameParams(W, H, spp=1, max_bounces=0, flags=bm.BM_FLAG_PRIMARY_ONLY)
px, py = np.meshgrid(np.arange(W, dtype=np.float32) + np.float32(0.5), np.arange(H, dtype=np.float32) + np.float32(0.5))
pixel_np = bm.camera_pixel_rays(cam, W, H, px.ravel(), py.ravel())
pixel = torch.from_numpy(pixel_np.view(np.float32).reshape(N, 8)).cuda()
# the same rays stored in tile order: 16x16-pixel tiles row by row (the frame's work items), inside a tile four 8x8 blocks, so that the
# 64 consecutive records a wave takes are one 8x8 block of neighbouring pixels instead of 64 pixels of one row
yy, xx = np.divmod(np.arange(N), W)
tile_order = np.lexsort((xx % 8, yy % 8, (xx % 16) // 8, (yy % 16) // 8, xx // 16, yy // 16))
tiled = torch.from_numpy(np.ascontiguousarray(pixel_np[tile_order]).view(np.float32).reshape(N, 8)).cuda()
rng = np.random.default_rng(1)
heights = np.block([[scene.column_heights(sx, sy) for sx in range(G // 128)] for sy in range(G // 128)])  # [y, x]
ox, oy = rng.uniform(0, G, N), rng.uniform(0, G, N)
oz = np.minimum(heights[oy.astype(int), ox.astype(int)] + rng.uniform(1, 64, N), G - 1)
dirs = rng.normal(size=(N, 3))
dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
incoherent = torch.from_numpy(bm.pack_rays(np.stack([ox, oy, oz], -1), dirs).view(np.float32).reshape(N, 8)).cuda()
hits = torch.empty((N, 8), dtype=torch.float32, device="cuda")
stream = torch.cuda.current_stream()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    return a, b


def query(rays):
    return lambda: scene.cast_rays_raw(N, rays.data_ptr(), hits.data_ptr(), 0, None, stream.cuda_stream)


render = lambda: scene.render(cam, frame, acc, stream=stream.cuda_stream)
for _ in range(5):  # warm-up
    query(pixel)(); render(); query(incoherent)()
torch.cuda.synchronize()
qa, fa, fk, qb, qt = [], [], [], [], []
for _ in range(reps):
    e1 = timed(query(pixel))
    e2 = timed(render)
    e3 = timed(query(tiled))
    torch.cuda.synchronize()
    qa.append(e1[0].elapsed_time(e1[1])); fa.append(e2[0].elapsed_time(e2[1])); fk.append(scene.last_render_ms())
    qt.append(e3[0].elapsed_time(e3[1]))
for _ in range(reps):
    e = timed(query(incoherent))
    torch.cuda.synchronize()
    qb.append(e[0].elapsed_time(e[1]))
res = scene.cast_rays(pixel)
torch.cuda.synchronize()
lv = res.level.cpu().numpy()
rest = scene.cast_rays(tiled)
torch.cuda.synchronize()
bits = lambda h: h.packed.cpu().view(torch.int32)  # (bit patterns: a miss's voxel of -1 is a NaN as a float)
assert torch.equal(bits(rest), bits(res)[torch.from_numpy(tile_order)]), "tile order changed the answers"
resb = scene.cast_rays(incoherent)
torch.cuda.synchronize()
lvb = resb.level.cpu().numpy()
picks = []
for _ in range(reps):
    t0 = time.perf_counter()
    hit = scene.pick(cam, W // 2, H // 2, W, H)
    picks.append((time.perf_counter() - t0) * 1e3)
m = lambda v: float(np.median(v))
print(f"config-2 world {G}^3, preloaded; medians of {reps} runs after 5 warm-up rounds; device times from events around the calls")
print(f"(a) 1080p pixel-centre rays of the config-2 camera ({N} rays, {np.mean(lv == 2) * 100:.1f} % hit a voxel):")
print(f"    bm_scene_cast_rays                 {m(qa):8.4f} ms   {N / m(qa) / 1e6:6.3f} Grays/s")
print(f"    primary-only 1080p / 1 spp frame   {m(fa):8.4f} ms   (its kernel alone, bm_last_render_ms: {m(fk):.4f} ms)")
print(f"    ratio query / frame                {m(qa) / m(fa):8.3f}     (target <= 1.2)")
print(f"    the same rays in tile order        {m(qt):8.4f} ms   {N / m(qt) / 1e6:6.3f} Grays/s   ratio to the frame {m(qt) / m(fa):.3f}")
print(f"(b) {N} incoherent rays (random origins 1-64 voxels above the terrain, random directions; {np.mean(lvb == 2) * 100:.1f} % hit):")
print(f"    bm_scene_cast_rays                 {m(qb):8.4f} ms   {N / m(qb) / 1e6:6.3f} Grays/s")
print(f"(c) Scene.pick, one ray, host-visible (Python, waits for the result): {m(picks):.3f} ms  (hit level {hit.level if hit else -1})")
print(f"record traffic, 64 B per ray: (a) {64 * N / m(qa) / 1e6:.1f} GB/s, (b) {64 * N / m(qb) / 1e6:.1f} GB/s -- far below HBM bandwidth: the walk, not the records, sets the time")
scene.close()
