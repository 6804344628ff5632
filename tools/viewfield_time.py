"""Cost of building the view plane (csrc/viewfield.hip), hipEvents on the load stream (bm_scene_view_plane_stats): the terrain world of the
given sizes (cubes of that many voxels), 64 x 64 production frames from bench config 2's camera position and from two others -- every
new resting position is one build of the whole plane.  With a saving per frame in ms as the last argument after `--`, the break-even
number of resting frames (build ms / saving) is printed as well.
usage: python tools/viewfield_time.py [size ...] [-- saving_ms]  (default 1024 4096)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
args = sys.argv[1:]
saving = float(args[args.index("--") + 1]) if "--" in args else None
sizes = [int(a) for a in (args[:args.index("--")] if "--" in args else args)] or [1024, 4096]
for G in sizes:
    t0 = time.perf_counter()
    scene = bm.Scene(G, G, device=0).generate()
    print(f"{G}^3 voxels ({G // 8}^3 cells), generated in {time.perf_counter() - t0:.1f} s")
    acc = torch.zeros((64, 64, 4), dtype=torch.float32, device="cuda")
    for name, pos in {"config 2's camera": (G / 2, G / 8, 0.8 * G), "high in a corner": (G / 16, G / 16, 0.95 * G), "low, at the middle": (G / 2 + 3.5, G / 2 + 1.5, 0.55 * G)}.items():
        cam = bm.Camera(position=pos, horizontal_angle=0.8, vertical_angle=-0.5).update()
        for rep in range(2):  # the second launch from a position finds the camera at rest
            scene.render(cam, bm.FrameParams(64, 64, spp=1, max_bounces=3), acc)
        torch.cuda.synchronize()
        builds, ms = scene.view_plane_stats()
        plane, origin = scene.view_plane()
        inner = plane[1:-1, 1:-1, 1:-1]
        field = scene.device_cube_field()[:, 1:-1, 1:-1, 1:-1].max(axis=0) if G <= 1024 else None
        more = "" if field is None else f", above every octant's byte: {np.count_nonzero((inner != 255) & (inner > field)) / inner.size:.3f}"
        even = "" if saving is None else f"; break-even after {ms / saving:.0f} resting frames at {saving} ms saved per frame"
        print(f"  {name:>18}: build {builds} took {ms:.3f} ms (bytes 255: {np.count_nonzero(inner == 255) / inner.size:.3f}, bytes >= 4: {np.count_nonzero((inner >= 4) & (inner < 255)) / inner.size:.3f}{more}){even}")
    scene.close()
