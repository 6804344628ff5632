"""Cost of building the sun plane (csrc/sunfield.hip), hipEvents on the load stream (bm_scene_sun_plane_stats): the terrain world of the
given sizes (cubes of that many voxels), one 64 x 64 production frame per sun -- every new sun is one build of the whole plane -- for an
x-dominant, a y-dominant and a z-dominant sun, twice.  usage: python tools/sunfield_time.py [size ...]  (default 1024 4096)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096]
SUNS = {"x dominant": (0.05, 0.1), "y dominant": (0.2, 0.1), "z dominant": (0.3, 0.4)}
for G in sizes:
    t0 = time.perf_counter()
    scene = bm.Scene(G, G, device=0).generate()
    print(f"{G}^3 voxels ({G // 8}^3 cells), generated in {time.perf_counter() - t0:.1f} s")
    cam = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
    acc = torch.zeros((64, 64, 4), dtype=torch.float32, device="cuda")
    for rep in range(2):
        for name, sun in SUNS.items():
            scene.render(cam, bm.FrameParams(64, 64, spp=1, max_bounces=3, sun_position=sun), acc)
            torch.cuda.synchronize()
            builds, ms = scene.sun_plane_stats()
            plane, plan = scene.sun_plane()
            share = "" if plane is None else f", bytes 255: {np.count_nonzero(plane[1:-1, 1:-1, 1:-1] == 255) / plane[1:-1, 1:-1, 1:-1].size:.3f}, bytes >= 4: {np.count_nonzero((plane >= 4) & (plane < 255)) / plane[1:-1, 1:-1, 1:-1].size:.3f}"
            print(f"  {name:>10}: build {builds} took {ms:.3f} ms (bins per slab {plan['lo1']}..{plan['hi1']}, {plan['lo2']}..{plan['hi2']}){share if rep == 0 else ''}")
    scene.close()
