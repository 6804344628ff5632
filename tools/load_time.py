"""Cost of building a scene from dense voxels (bm_scene_load_voxels) on the config-2 world (1024^3 voxels; the volume is that world's own
voxels) and on a volume that is not terrain (blobs + 1 % noise): wall time of generate (16 threads) + preload_all -- the only way to
that scene before --, of the host route and of the device route (volume already on the GPU), the device route's split from
bm_scene_last_load_ms (pack = classify + number + pack kernels / cube field / copy back to the host world), and, in the same process, a
plain device-to-device hipMemcpyAsync of the same volume.  Wall times end in a finished scene (the calls synchronise).
usage: python tools/load_time.py [repeats]  (-> profiles/load_time.txt)"""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
G = 1024


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def d2d_copy_ms(src):
    """median device time of hipMemcpyAsync(dst, src, bytes, device to device) on the current stream"""
    dst = torch.empty_like(src)
    hip = None
    for name in ("libamdhip64.so.7", "libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            pass
    stream = torch.cuda.current_stream()
    times = []
    for k in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if hip is not None:
            assert hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(src.numel()), 3, C.c_void_p(stream.cuda_stream)) == 0
        else:
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    assert torch.equal(dst, src)
    return float(np.median(times[2:])), "hipMemcpyAsync" if hip is not None else "tensor.copy_"


def measure(name, volume, generate):
    dev = torch.from_numpy(volume).to("cuda:0")
    torch.cuda.synchronize()
    print(f"--- {name}: {G}^3 voxels, {volume.size / 2**30:.2f} GiB, {int(np.count_nonzero(volume)) / volume.size:.1%} solid")
    if generate:
        ms = [wall(lambda: bm.Scene(G, G, device=0).generate(16).preload_all())[0] for _ in range(max(2, reps // 2))]
        print(f"generate(16 threads) + preload_all, wall: {np.median(ms):9.1f} ms   (min {min(ms):.1f}, {len(ms)} runs)")
    ms = [wall(lambda: bm.Scene.from_voxels(volume))[0] for _ in range(max(2, reps // 2))]
    print(f"host route   (numpy volume), wall:       {np.median(ms):9.1f} ms   (min {min(ms):.1f}, {len(ms)} runs)")
    scene = bm.Scene(G, G, device=0)
    scene.load_voxels(dev)  # warm-up: code objects, the first mapping of the arena
    rows = []
    for _ in range(reps):
        w, _ = wall(lambda: scene.load_voxels(dev))
        rows.append((w,) + scene.last_load_ms())
    r = np.median(np.array(rows), 0)
    print(f"device route (device tensor), wall:      {r[0]:9.1f} ms   (min {min(x[0] for x in rows):.1f}, {reps} runs; a scene that already holds a world)")
    print(f"  device time: pack {r[1]:.3f} ms (classify + number + pack kernels), field {r[2]:.3f} ms, mirror {r[3]:.3f} ms (words + bricks back to the host)")
    copy, how = d2d_copy_ms(dev)
    gib = volume.size / 2**30
    print(f"  device-to-device {how} of the volume: {copy:.3f} ms ({2 * gib / copy * 1e3:.0f} GiB/s read + written)")
    print(f"  pack / copy = {r[1] / copy:.2f}  (expected <= 1.5)   bricks: {scene.info()['total_bricks']}")
    scene.close()
    return r


print(f"{torch.cuda.get_device_name(0)}; medians; volume: uint8 [z, y, x]")
terrain = bm.Scene(G, G, device=0).generate(16).preload_all()
vol = terrain.voxels().view(np.uint8)
terrain.close()
measure("config-2 terrain", vol, True)
rng = np.random.default_rng(2)
other = (rng.random((G, G, G), dtype=np.float32) < 0.01).astype(np.uint8)
z, y, x = np.ogrid[:256, :256, :256]
for k in range(24):
    c = rng.integers(0, G - 256, 3)
    r = int(rng.integers(30, 120))
    other[c[2]:c[2] + 256, c[1]:c[1] + 256, c[0]:c[0] + 256] |= ((x - 128) ** 2 + (y - 128) ** 2 + (z - 128) ** 2 <= r * r).astype(np.uint8)
measure("blobs + 1% noise", other, False)
