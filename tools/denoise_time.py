"""Cost of the a-trous filter (bm_denoise) at 1080p with 5 iterations on the config-2 world (1024^3 voxels, preloaded), bench.py's config-2
camera.  One round = a production 1-spp frame, the guides (Scene.pixel_hits: device pixel rays + a BM_QUERY_LOD ray query), the filter, the
filter once more through the measuring door (a hipEvent between its kernels) and a clone() of the float4 image -- the floor of one image
pass: one read and one write per pixel -- each between device events; medians over the rounds after warm-up.  The bar to report against: the
filter without its guides should cost less than the frame it cleans.  BM_DENOISE_TILED_MAX (the largest a-trous stride that stages its
taps in LDS; unset = the library's choice) is echoed, so that runs with different values can be laid side by side.
usage: python tools/denoise_time.py [repeats]  (-> profiles/denoise_time.txt)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
G, W, H, ITER, SIGMA = 1024, 1920, 1080, 5, 4.0
N = W * H
scene = bm.Scene(G, G, device=0).generate().preload_all()
cam = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
frame = bm.FrameParams(W, H, spp=1, max_bounces=3)
acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
out = torch.empty_like(acc)
stream = torch.cuda.current_stream()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    r = fn()
    b.record(stream)
    return a, b, r


def render():
    acc.zero_()
    scene.render(cam, frame, acc)


hits = scene.pixel_hits(cam, W, H)
for _ in range(5):  # warm-up of every call the rounds time
    render(); scene.pixel_hits(cam, W, H); scene.denoise(acc, hits, W, H, ITER, SIGMA, out=out); scene.denoise_times(acc, hits, W, H, ITER, SIGMA, out=out); acc.clone()
torch.cuda.synchronize()
t = {k: [] for k in ("frame", "frame_kernel", "hits", "denoise", "clone")}
kernels = []
for _ in range(reps):
    render()  # (its own time: bm_last_render_ms, the kernel between the library's events, without the zeroing)
    e_h = timed(lambda: scene.pixel_hits(cam, W, H))
    e_d = timed(lambda: scene.denoise(acc, e_h[2], W, H, ITER, SIGMA, out=out))
    e_c = timed(lambda: acc.clone())
    torch.cuda.synchronize()
    t["frame_kernel"].append(scene.last_render_ms())
    t["hits"].append(e_h[0].elapsed_time(e_h[1])); t["denoise"].append(e_d[0].elapsed_time(e_d[1])); t["clone"].append(e_c[0].elapsed_time(e_c[1]))
    kernels.append(scene.denoise_times(acc, e_h[2], W, H, ITER, SIGMA, out=out)[1])
m = lambda v: float(np.median(v))
k = np.median(np.array(kernels), axis=0)
lv = hits.level.cpu().numpy()
names = ["denoise_prepare", "denoise_moments"] + [f"a-trous pass, step {1 << i:<3d}" for i in range(ITER)]
knob = os.environ.get("BM_DENOISE_TILED_MAX", "")
print(f"config-2 world {G}^3, preloaded; {W}x{H}, {ITER} iterations, sigma_l {SIGMA}; medians of {reps} rounds after 5 warm-up rounds; device events")
print(f"BM_DENOISE_TILED_MAX={knob if knob else '(unset: the library default)'}; guides: {np.mean(lv >= 0) * 100:.1f} % of the pixels hit, levels 0/1/2: "
      f"{np.mean(lv == 0) * 100:.1f} / {np.mean(lv == 1) * 100:.1f} / {np.mean(lv == 2) * 100:.1f} %")
print(f"1-spp production frame, its kernel (bm_last_render_ms)   {m(t['frame_kernel']):8.4f} ms")
print(f"guides: Scene.pixel_hits (pixel rays + LoD ray query)     {m(t['hits']):8.4f} ms")
print(f"bm_denoise, events around the call                        {m(t['denoise']):8.4f} ms   ratio to the frame {m(t['denoise']) / m(t['frame_kernel']):.3f}  (bar: < 1)")
print(f"clone() of the float4 image (one read + one write)        {m(t['clone']):8.4f} ms   {32 * N / m(t['clone']) / 1e6:7.1f} GB/s")
print("per kernel (a hipEvent between the kernels: bm_debug_denoise_times), and the bytes a pass needs at least over its time:")
need = [48 + 20, 20 + 16] + [20 + 16] * ITER  # prepare: accum + hit in, image + key out; the others: image + key in, image out
for n_, ms, b in zip(names, k, need):
    print(f"    {n_:<24s} {ms:8.4f} ms   {b * N / ms / 1e6:7.1f} GB/s   {ms / m(t['clone']):5.2f} x clone")
print(f"    sum of the kernels       {k.sum():8.4f} ms   dominant: {names[int(np.argmax(k))].strip()}")
print(f"filter + guides: {m(t['denoise']) + m(t['hits']):.4f} ms = {(m(t['denoise']) + m(t['hits'])) / m(t['frame_kernel']):.3f} x the frame")
scene.close()
