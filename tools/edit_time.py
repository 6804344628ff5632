"""Cost of one voxel-edit batch on the config-2 world (1024^3 voxels = 8x8x8 supercells, preloaded): carve a sphere of radius 8, 32
and 128 into the terrain the camera looks at and time, with hipEvents on the load stream, the scatter (pool moves, bricks, index
words) and the cube-field update (bm_scene_last_edit_ms), plus the host time of the call and the kernel time of the 1080p frame after
the edit.  usage: python tools/edit_time.py [repeats]  (-> profiles/edit_time.txt)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
G, W, H = 1024, 1920, 1080
scene = bm.Scene(G, G, device=0).generate().preload_all()
cam = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
p = bm.FrameParams(W, H, spp=1, max_bounces=3)
for i in range(8):
    scene.render(cam, p, acc)
torch.cuda.synchronize()
base = float(np.median(scene.render_times(6)))
print(f"config-2 world {G}^3, preloaded; frame before any edit: {base:.4f} ms (median of 6)")
print(f"{'radius':>6} {'cells':>7} {'host ms':>8} {'scatter ms':>10} {'field ms':>9} {'edit ms':>8} {'next frame ms':>13}")
rng = np.random.default_rng(1)
for r in (8, 32, 128):
    rows = []
    for k in range(reps):
        x, y = int(rng.integers(300, 700)), int(rng.integers(300, 700))
        c = (x, y, int(scene.column_heights(x // 128, y // 128)[y % 128, x % 128]))  # on the terrain surface
        scene.render(cam, p, acc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scene.carve_sphere(c, r)
        t1 = time.perf_counter()
        scatter, field = scene.last_edit_ms()
        scene.render(cam, p, acc)
        torch.cuda.synchronize()
        rows.append(((t1 - t0) * 1e3, scatter, field, scene.last_render_ms()))
        scene.fill_sphere(c, r)  # a full brick set back: the world stays terrain-like for the next sample
        torch.cuda.synchronize()
    a = np.median(np.array(rows), 0)
    cells = (2 * r + 8) ** 3 // 512
    print(f"{r:>6} {cells:>7} {a[0]:>8.3f} {a[1]:>10.4f} {a[2]:>9.4f} {a[1] + a[2]:>8.4f} {a[3]:>13.4f}")
print(f"(medians of {reps} carves per radius; 'cells' = brick cells of the sphere's bounding box; 'edit ms' = scatter + field on the device)")
scene.close()
