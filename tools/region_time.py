"""Cost of writing and reading dense voxel regions of a live scene (bm_scene_write_region / bm_scene_read_region) on the config-2 world
(1024^3 voxels, preloaded): boxes of 64^3, 256^3 and 1024 x 1024 x 64 voxels, each aligned and offset by (3, 5, 1).  Per box, medians of
repeated calls after a warm-up: a device write that changes every brick of the box and one that changes none -- wall time of the call
and its split from bm_scene_last_region_ms (pack / copy / scatter / field; host = wall minus those: merge and staging) --, the device
read (unpack time by events on the stream, wall time), and in the same process a device-to-device hipMemcpyAsync of as many bytes as the
box holds, the bar for the aligned pack and unpack of the two large boxes (<= 1.5 x).  For the aligned 64^3 box also set_voxels with the
same content, and for the 256^3 box a full load_voxels of the world with the box applied: the two things a caller had to do before.
usage: python tools/region_time.py [repeats]  (-> profiles/region_time.txt)"""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, brickmap_amd as bm
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
G = 1024
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "region_time.txt")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def d2d_copy_ms(nbytes):
    """median device time of a contiguous hipMemcpyAsync(device to device) of nbytes on the current stream"""
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0"), torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    hip = C.CDLL("libamdhip64.so.7")
    stream = torch.cuda.current_stream()
    times = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(nbytes), 3, C.c_void_p(stream.cuda_stream)) == 0
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times[2:]))


def med(rows):
    return np.median(np.array(rows), axis=0)


def measure(scene, name, lo, shape, bar):
    nbytes = int(np.prod(shape))
    g = torch.Generator(device="cuda:0").manual_seed(1)
    # two contents that differ in every brick of the box (a voxel of every 8-row flips), both about half solid
    a = (torch.rand(shape, device="cuda:0", generator=g) < 0.5).to(torch.uint8)
    b = a.clone()
    b[:, :, ::8] ^= 1
    copy = d2d_copy_ms(nbytes)
    say(f"--- {name}: lo {lo}, {shape[2]} x {shape[1]} x {shape[0]} voxels, {nbytes / 2**20:.1f} MiB; device-to-device copy of as many bytes {copy:.3f} ms")
    scene.write_region(lo, a)
    scene.write_region(lo, b)  # warm-up: staging buffers grown, pools grown
    for label, volumes in (("every brick changes", (a, b)), ("no brick changes  ", (b, b))):
        rows = []
        for k in range(reps):
            v = volumes[k % 2]
            w = wall(lambda: scene.write_region(lo, v))
            p, c, s, f = scene.last_region_ms()
            rows.append((w, p, c, s, f, w - p - c - s - f))
        w, p, c, s, f, h = med(rows)
        say(f"write, {label}: wall {w:8.3f} ms = pack {p:.3f} + copy {c:.3f} + scatter {s:.3f} + field {f:.3f} + host (merge, staging) {h:.3f};  pack / d2d copy = {p / copy:.2f}"
            + (f"  [bar 1.5: {'holds' if p / copy <= 1.5 else 'MISSED'}]" if bar else ""))
    out = torch.empty(shape, dtype=torch.uint8, device="cuda:0")
    hi = (lo[0] + shape[2], lo[1] + shape[1], lo[2] + shape[0])
    scene.read_region(lo, hi, out=out)
    rows = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        scene.read_region(lo, hi, out=out)
        e1.record()
        torch.cuda.synchronize()
        rows.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
    w, u = med(rows)
    nx, ny = min(shape[2], G - lo[0]), min(shape[1], G - lo[1])  # the part of the box inside the world holds what the last write left; the rest reads 0
    assert torch.equal(out[:, :ny, :nx], b[:, :ny, :nx]) and not out[:, ny:, :].any() and not out[:, :, nx:].any()
    say(f"read to device memory: wall {w:8.3f} ms, unpack {u:.3f} ms;  unpack / d2d copy = {u / copy:.2f}" + (f"  [bar 1.5: {'holds' if u / copy <= 1.5 else 'MISSED'}]" if bar else ""))
    return a, b


def main():
    say(f"region_time: {G}^3 world (config 2), preloaded; medians of {reps} calls after a warm-up; {torch.cuda.get_device_name(0)}")
    scene = bm.Scene(G, G, device=0).generate(16).preload_all()
    base = (256, 256, 448)
    for name, shape in (("64^3", (64, 64, 64)), ("256^3", (256, 256, 256)), ("1024 x 1024 x 64 slab", (64, 1024, 1024))):
        for off, kind in (((0, 0, 0), "aligned"), ((3, 5, 1), "offset by (3, 5, 1)")):
            lo = tuple((0 if n == G else v) + o for v, n, o in zip(base, shape[::-1], off))
            a, b = measure(scene, f"{name}, {kind}", lo, shape, bar=kind == "aligned" and name != "64^3")
            if kind != "aligned":
                continue
            if name == "64^3":  # what a caller had to do before: one edit per voxel
                z, y, x = np.nonzero(np.ones(shape, bool))
                coords = np.stack([x + lo[0], y + lo[1], z + lo[2]], 1).astype(np.int32)
                va, vb = a.cpu().numpy().ravel(), b.cpu().numpy().ravel()
                ms = [wall(lambda: scene.set_voxels(coords, va if k % 2 else vb)) for k in range(max(3, reps // 2))]
                w = float(np.median([wall(lambda: scene.write_region(lo, a if k % 2 else b)) for k in range(reps)]))
                say(f"set_voxels with the same 64^3 content (host coordinates and values): wall {np.median(ms):.1f} ms = {np.median(ms) / w:.0f} x the region write ({w:.3f} ms)")
            if name == "256^3":  # or: reload the whole world with the box applied
                world = scene.read_region((0, 0, 0), (G, G, G), device=True)
                other = bm.Scene(G, G, device=0)
                other.load_voxels(world)
                ms = [wall(lambda: other.load_voxels(world)) for _ in range(max(3, reps // 2))]
                w = float(np.median([wall(lambda: scene.write_region(lo, a if k % 2 else b)) for k in range(reps)]))
                say(f"full load_voxels of the {G}^3 world from a device tensor: wall {np.median(ms):.1f} ms = {np.median(ms) / w:.1f} x the 256^3 region write ({w:.3f} ms)")
                other.close()
                del world
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
