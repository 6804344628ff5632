"""What temporal reprojection (Scene.reproject) buys for a moving camera: the sequence of tests/test_gpu_reproject.py -- eight 1-spp
frames, the camera half a voxel sideways per frame, every frame with samples of its own, through TemporalAccumulator -- on the test's
view (256^3 world, 128x72) and on bench.py's config-2 view (1024^3 world, 1080p).  RMSE of the radiance of the last frame against 256 spp
of the last view (other samples) for the 1-spp frame, the reprojected history, the denoised 1-spp frame and the denoised history, over
the pixels that took history and over all filtered (non-special) pixels.
usage: python tools/reproject_quality.py  (-> profiles/reproject_quality.txt)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm

FRAMES = 8
for G, W, H in ((256, 128, 72), (1024, 1920, 1080)):
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    start = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
    side = np.cross(np.asarray(start.direction, np.float64), (0.0, 0.0, 1.0))
    side /= np.linalg.norm(side)
    temporal = bm.TemporalAccumulator(scene, W, H)
    means = []
    for k in range(FRAMES):
        cam = bm.Camera(position=tuple(float(p + 0.5 * k * s) for p, s in zip(start.position, side)), direction=start.direction, up=start.up)
        one = torch.zeros((H, W, 4), device="cuda")
        scene.render(cam, bm.FrameParams(W, H, spp=1, sample_base=k), one)
        hits = scene.pixel_hits(cam, W, H)
        image = temporal.add(cam, one, hits)
        means.append(float(image[..., 3][image[..., 3] > 0].mean()))
    ref = torch.zeros((H, W, 4), device="cuda")
    scene.render(cam, bm.FrameParams(W, H, spp=256, sample_base=1000), ref)
    rad = lambda a: torch.where(a[..., 3:] > 0, a[..., :3] / a[..., 3:], torch.zeros_like(a[..., :3])).double()
    c256 = rad(ref)
    took = image[..., 3] > one[..., 3]
    filtered = temporal.history.keys != -1  # (the special key, as int32 bits)
    shown = {"1 spp": rad(one), "reprojected": rad(image), "denoised 1 spp": scene.denoise(one, hits, W, H)[..., :3].double(),
             "reprojected + denoised": scene.denoise(image, hits, W, H)[..., :3].double()}
    print(f"{G}^3 world, {W}x{H}, camera ({G / 2:g}, {G / 8:g}, {0.8 * G:g}) angles 0.8 / -0.5, {FRAMES} frames, 0.5 voxel sideways per frame, max_history 32; reference: 256 spp")
    print(f"    mean samples per pixel with samples, frame by frame: {' '.join(f'{v:.2f}' for v in means)}")
    for label, keep in ((f"the pixels that took history ({float(took.float().mean()) * 100:.1f} % of the image)", took),
                        (f"all filtered pixels ({float(filtered.float().mean()) * 100:.1f} %)", filtered)):
        rmse = lambda img: float(torch.sqrt(((img - c256)[keep] ** 2).mean()))
        base = rmse(shown["1 spp"])
        print(f"    over {label}:")
        for name, img in shown.items():
            print(f"        {name:<24s} RMSE {rmse(img):.4f}   ratio {rmse(img) / base:.3f}")
    scene.close()
