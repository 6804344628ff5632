# wall ms per frame of a ring of 20 frames (config 2) whose camera MOVES every frame: no view plane is ever built; best of 5 launches.
# usage via tools/ab_run.py <lib> tools/ring20_moving.py
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
G, W, H = 1024, 1920, 1080
scene = bm.Scene(G, G, device=0).generate().preload_all()
K = 20
accs = [torch.zeros((H, W, 4), dtype=torch.float32, device='cuda') for _ in range(K)]
best = 1e9
for rep in range(8):
    cams = [bm.Camera(position=(G / 2 + 1.25 * (rep * K + i), G / 8 + 0.5 * i, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update() for i in range(K)]
    ps = [bm.FrameParams(W, H, spp=1, sample_base=rep * K + i, max_bounces=3) for i in range(K)]
    scene.render_frames(cams, ps, accs)
    torch.cuda.synchronize()
    if rep >= 3: best = min(best, scene.last_render_ms() / K)
builds = scene.view_plane_stats()[0] if hasattr(scene._L, "bm_scene_view_plane_stats") else "n/a"
print(f"ring of 20 distinct cameras: {best:.4f} ms per frame (kernel); view plane builds: {builds}")
