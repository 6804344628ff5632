"""What the a-trous filter (Scene.denoise) buys: RMSE of a 1-spp frame and of its denoised version against a 256-spp frame of the same view
(other samples), over the filtered pixels, for the view of tests/test_gpu_denoise.py (256^3 world, 128x72) and for bench.py's config-2 view
(1024^3 world, 1080p), by number of iterations.
usage: python tools/denoise_quality.py  (-> profiles/denoise_quality.txt)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm

for G, W, H in ((256, 128, 72), (1024, 1920, 1080)):
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    cam = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
    one, ref = torch.zeros((H, W, 4), device="cuda"), torch.zeros((H, W, 4), device="cuda")
    scene.render(cam, bm.FrameParams(W, H, spp=1), one)
    scene.render(cam, bm.FrameParams(W, H, spp=256, sample_base=1), ref)
    hits = scene.pixel_hits(cam, W, H)
    rad = lambda a: torch.where(a[..., 3:] > 0, a[..., :3] / a[..., 3:], torch.zeros_like(a[..., :3])).double()
    c256 = rad(ref)
    raw = scene.denoise(one, hits, W, H, iterations=0)
    # filtered pixels: those an iteration may change (the key rule of include/brickmap.h, from the guide records)
    normal, level = hits.normal.reshape(H, W, 3), hits.level.reshape(H, W)
    keep = (one[..., 3] > 0) & (level >= 0) & (level <= 2) & (normal != 0).any(-1)
    rmse = lambda img: float(torch.sqrt(((img[..., :3].double() - c256)[keep] ** 2).mean()))
    base = rmse(raw)
    print(f"{G}^3 world, {W}x{H}, camera ({G / 2:g}, {G / 8:g}, {0.8 * G:g}) angles 0.8 / -0.5; {float(keep.float().mean()) * 100:.1f} % of the pixels are filtered; reference: 256 spp")
    print(f"    1 spp                      RMSE {base:.4f}")
    for it in (1, 2, 3, 4, 5, 6):
        e = rmse(scene.denoise(one, hits, W, H, iterations=it, sigma_l=4.0))
        print(f"    denoised, {it} iterations     RMSE {e:.4f}   ratio {e / base:.3f}")
    for sigma in (1.0, 16.0):
        e = rmse(scene.denoise(one, hits, W, H, iterations=5, sigma_l=sigma))
        print(f"    5 iterations, sigma_l {sigma:<4g} RMSE {e:.4f}   ratio {e / base:.3f}")
    scene.close()
