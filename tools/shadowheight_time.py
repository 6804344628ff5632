"""Cost of the shadow heights (csrc/shadowheight.h, built by sunfield.hip with the sun plane), hipEvents on the load stream
(bm_scene_sun_plane_stats, which brackets the whole build): the resident terrain world of the given sizes (cubes of that many voxels), one
64 x 64 production frame per event --
  a new sun: the plane and the slice together (x-, y- and z-dominant; the last has no shadow heights: the slice is zeroed);
  an edit of one voxel inside a full brick: no cell's occupancy changes, the plane stands, the slice alone is rebuilt;
  a loop of such an edit before every frame: wall ms per (edit + frame) against the loop without the edit.
Run it against another build with tools/ab_run.py: a library without shadow heights reports the plane's build alone.
usage: python tools/shadowheight_time.py [size ...]  (default 1024)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
from brickmap_amd import _lib
sizes = [int(a) for a in sys.argv[1:]] or [1024]
SUNS = {"x dominant": (0.05, 0.1), "y dominant": (0.2, 0.1), "z dominant": (0.3, 0.4)}
have = "bm_scene_shadow_heights" in _lib.SIGNATURES
for G in sizes:
    t0 = time.perf_counter()
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    print(f"{G}^3 voxels ({G // 8}^3 cells), generated and preloaded in {time.perf_counter() - t0:.1f} s; shadow heights in this library: {have}")
    cam = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
    acc = torch.zeros((64, 64, 4), dtype=torch.float32, device="cuda")

    def frame(sun):
        scene.render(cam, bm.FrameParams(64, 64, spp=1, max_bounces=3, sun_position=sun), acc)
        torch.cuda.synchronize()
    for rep in range(2):
        for name, sun in SUNS.items():
            frame(sun)
            builds, ms = scene.sun_plane_stats()
            extra = ""
            if have and rep == 0:
                entries, splan, nbytes = scene.shadow_heights()
                extra = f"; shadow heights valid {splan['valid']}, rise {splan['rise']}..{splan['rise_hi']}, {np.count_nonzero(entries)} of {entries.size} columns have dark cells, {nbytes} bytes"
            print(f"  {name:>10}: build {builds} took {ms:.3f} ms{extra}")
    sun = SUNS["x dominant"]
    frame(sun)
    v = (G // 2 + 3, G // 2 + 3, 3)  # a voxel of a bottom brick: full in the terrain
    for rep in range(3):
        scene.clear_box(v, tuple(c + 1 for c in v)) if rep % 2 == 0 else scene.fill_box(v, tuple(c + 1 for c in v))
        frame(sun)
        builds, ms = scene.sun_plane_stats()
        print(f"  one-voxel edit, no occupancy change: builds {builds}, last build (the slice alone where there is one) {ms:.3f} ms")
    for edit in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(40):
            if edit:
                scene.clear_box(v, tuple(c + 1 for c in v)) if i % 2 == 0 else scene.fill_box(v, tuple(c + 1 for c in v))
            scene.render(cam, bm.FrameParams(64, 64, spp=1, max_bounces=3, sun_position=sun), acc)
        torch.cuda.synchronize()
        print(f"  loop of 40 x ({'one-voxel edit + ' if edit else ''}64 x 64 frame): {(time.perf_counter() - t0) / 40 * 1e3:.3f} ms each")
    scene.close()
