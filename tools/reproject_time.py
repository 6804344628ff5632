"""Cost of the temporal reprojection (bm_reproject) at 1080p on the config-2 world (1024^3 voxels, preloaded), bench.py's config-2 camera
walking half a voxel sideways per frame.  Eight frames through TemporalAccumulator build a real history; then one round = a production
1-spp frame of the last view (its kernel: bm_last_render_ms), the guides (Scene.pixel_hits), the reprojection of that frame into the
history of the frame before, and a clone() of the float4 image -- the floor of one image pass: one read and one write per pixel -- each
between device events; medians over the rounds after warm-up.  And, because one call is short against the resolution of an event, a batch
of 100 reprojections between one pair of events.  The bar to report against is the denoise's: below the 1-spp frame's kernel.
usage: python tools/reproject_time.py [repeats]  (-> profiles/reproject_time.txt)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
G, W, H, FRAMES, BATCH = 1024, 1920, 1080, 8, 100
N = W * H
scene = bm.Scene(G, G, device=0).generate().preload_all()
start = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
side = np.cross(np.asarray(start.direction, np.float64), (0.0, 0.0, 1.0))
side /= np.linalg.norm(side)
view = lambda k: bm.Camera(position=tuple(float(p + 0.5 * k * s) for p, s in zip(start.position, side)), direction=start.direction, up=start.up)
acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
stream = torch.cuda.current_stream()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    r = fn()
    b.record(stream)
    return a, b, r


def render(k):
    acc.zero_()
    scene.render(view(k), bm.FrameParams(W, H, spp=1, sample_base=k, max_bounces=3), acc)


temporal = bm.TemporalAccumulator(scene, W, H)
for k in range(FRAMES - 1):
    render(k)
    temporal.add(view(k), acc)
prev, prev_cam, cam = temporal.history, view(FRAMES - 2), view(FRAMES - 1)
out = bm.History(torch.empty(5 * N, dtype=torch.float32, device="cuda"), W, H)
render(FRAMES - 1)
hits = scene.pixel_hits(cam, W, H)
run = lambda: scene.reproject(acc, hits, cam, prev_cam, prev, W, H, out=out)
for _ in range(5):  # warm-up of every call the rounds time
    render(FRAMES - 1); scene.pixel_hits(cam, W, H); run(); acc.clone()
torch.cuda.synchronize()
t = {k: [] for k in ("frame_kernel", "hits", "reproject", "clone", "batch")}
for _ in range(reps):
    render(FRAMES - 1)
    e_h = timed(lambda: scene.pixel_hits(cam, W, H))
    e_r = timed(run)
    e_c = timed(lambda: acc.clone())
    e_b = timed(lambda: [run() for _ in range(BATCH)])
    torch.cuda.synchronize()
    t["frame_kernel"].append(scene.last_render_ms())
    for name, e in (("hits", e_h), ("reproject", e_r), ("clone", e_c)):
        t[name].append(e[0].elapsed_time(e[1]))
    t["batch"].append(e_b[0].elapsed_time(e_b[1]) / BATCH)
m = lambda v: float(np.median(v))
img, a = out.image.cpu().numpy(), acc.cpu().numpy()
took = img[..., 3] > a[..., 3]
lv = hits.level.cpu().numpy()
print(f"config-2 world {G}^3, preloaded; {W}x{H}; history of {FRAMES - 1} frames, the camera half a voxel sideways per frame, max_history 32; "
      f"medians of {reps} rounds after 5 warm-up rounds; device events")
print(f"guides: {np.mean(lv >= 0) * 100:.1f} % of the pixels hit; {took.mean() * 100:.1f} % of the pixels took history, mean samples taken over {float((img[..., 3] - a[..., 3])[took].mean()):.2f}")
print(f"1-spp production frame, its kernel (bm_last_render_ms)   {m(t['frame_kernel']):8.4f} ms")
print(f"guides: Scene.pixel_hits (pixel rays + LoD ray query)     {m(t['hits']):8.4f} ms   (shared with the denoise)")
print(f"bm_reproject, events around one call                      {m(t['reproject']):8.4f} ms   ratio to the frame {m(t['reproject']) / m(t['frame_kernel']):.3f}  (bar: < 1)")
print(f"bm_reproject, {BATCH} calls between one pair of events, each  {m(t['batch']):8.4f} ms   {90 * N / m(t['batch']) / 1e6:7.1f} GB/s at 90 bytes per pixel   "
      f"{m(t['batch']) / m(t['clone']):5.2f} x clone   min {min(t['batch']):.4f} max {max(t['batch']):.4f}")
print(f"clone() of the float4 image (one read + one write)        {m(t['clone']):8.4f} ms   {32 * N / m(t['clone']) / 1e6:7.1f} GB/s")
scene.close()
