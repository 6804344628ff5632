"""Host time per call of the calls that only read the world (csrc/world_reads.cpp), at sizes where the host dominates, on a 128^3 world: a
device read_region of one cell in a preloaded and in a streaming scene (after a residency reset: the cell goes through the patch list),
label_region of a 64^3 box, cast_rays of 256 rays, query_volumes of 300 boxes.  Wall clock around the C call with every stream idle
beforehand (host) and around the call and the wait for it (total): median, p10 and p90 in microseconds of `calls` calls after 30; then the
device times of the last label_region.  One process is one sample: medians of different processes differ by more than the p10 ... p90 of one.
usage: python tools/read_time.py [calls]  (-> profiles/world_reads_time.txt)"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brickmap_amd as bm
from brickmap_amd.world import region_of

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 400
G = 128
vox = np.zeros((G, G, G), np.uint8)
vox[:16] = 1
vox[16:40, 72:88, 24:40] = 1
vox[16:56, 80:96, 88:104] = 1
vox[64:72, 60:68, 60:68] = 1
pre = bm.Scene.from_voxels(vox)
streaming = bm.Scene.from_voxels(vox).reset_residency()
L = pre._L
dev = "cuda:0"
stream = torch.cuda.current_stream().cuda_stream

cell = torch.empty((8, 8, 8), dtype=torch.uint8, device=dev)
r_cell, p_cell, _ = region_of((0, 0, 0), cell, "out")
labels = torch.empty((64, 64, 64), dtype=torch.int32, device=dev)
count = torch.zeros(1, dtype=torch.int64, device=dev)
rng = np.random.default_rng(3)
rays = np.zeros((256, 8), np.float32)
rays[:, 0:3] = rng.uniform(1.0, G - 1.0, (256, 3))
d = rng.normal(size=(256, 3))
rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
rays[:, 6] = np.inf
rays = torch.from_numpy(rays).to(dev)
hits = torch.empty((256, 32), dtype=torch.uint8, device=dev)  # (bm_ray_hit is at most 32 bytes)
lo = rng.integers(-8, G - 8, (300, 3))
boxes = torch.from_numpy(bm.volume_box(lo, lo + rng.integers(1, 40, (300, 3))).view(np.uint8).reshape(300, 48)).to(dev)
results = torch.empty((300, 40), dtype=torch.uint8, device=dev)


def read_call(scene):
    def call():
        e = L.bm_scene_read_region(scene.gpuScene, C.byref(r_cell), C.c_void_p(p_cell), 1, C.c_void_p(stream))
        assert e == 0, e
    return call


cases = [
    ("read_region 1 cell, preloaded", read_call(pre)),
    ("read_region 1 cell, streaming", read_call(streaming)),
    ("label_region 64^3", lambda: pre.label_region_raw((32, 32, 0), (96, 96, 64), labels.data_ptr(), count.data_ptr(), 0, stream)),
    ("cast_rays 256", lambda: pre.cast_rays_raw(256, rays.data_ptr(), hits.data_ptr(), 0, None, stream)),
    ("query_volumes 300", lambda: pre.query_volumes_raw(300, boxes.data_ptr(), results.data_ptr(), 0, stream)),
]
print(f"library {bm._lib.LIB_PATH}, {REPS} calls per case after 30; microseconds: host = the call alone, total = call + wait")
for name, call in cases:
    host, total = [], []
    for i in range(REPS + 30):
        torch.cuda.synchronize()
        t0 = time.perf_counter_ns()
        call()
        t1 = time.perf_counter_ns()
        torch.cuda.synchronize()
        t2 = time.perf_counter_ns()
        if i >= 30:
            host.append((t1 - t0) / 1e3)
            total.append((t2 - t0) / 1e3)
    h, t = np.array(host), np.array(total)
    print(f"{name:32s} host median {np.median(h):8.2f}  p10 {np.percentile(h, 10):8.2f}  p90 {np.percentile(h, 90):8.2f}   total median {np.median(t):8.2f}  p10 {np.percentile(t, 10):8.2f}")
assert int(cell.min()) == 1 and int(count.item()) >= 1 and int(results[:, 0:8].contiguous().view(torch.int64).sum()) > 0
lm = pre.last_label_ms()
print("label_region 64^3 device: local %.4f merge %.4f flatten %.4f ms" % lm)
