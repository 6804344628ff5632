"""Ray queries against a live scene on the MI355X (bm_scene_cast_rays): hits equal the oracle's intersect_voxel bit for bit (exact and
LoD mode), non-resident bricks are reported and requested like the frames request them, edits issued on another stream are seen,
tmax filters exactly, degenerate rays miss, bad arguments launch nothing, and headless_main --dig-at digs where it picked."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = 10001, 10002
INT_MAX = 2**31 - 1
CAMS = [((128, 32, 204.8), 0.8, -0.5), ((20, 20, 200), 0.7, -0.7), ((230, 200, 120), -2.4, -0.35)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def make_rays(bm, G, H, n, seed, cams=CAMS, scale=1.0):
    """origins inside, outside and on the faces of the box; random, axis-aligned and one-zero-component directions; pixel rays"""
    rng = np.random.default_rng(seed)
    box = np.array([G, G, H], np.float32)
    k = n // 6
    inside = rng.uniform(0.01, 0.99, (k, 3)).astype(np.float32) * box
    outside = (rng.uniform(-0.5, 1.5, (k, 3)) * box).astype(np.float32)
    face = (rng.uniform(0, 1, (k, 3)) * box).astype(np.float32)
    axis = rng.integers(0, 3, k)
    face[np.arange(k), axis] = np.where(rng.integers(0, 2, k) == 1, box[axis], 0).astype(np.float32)
    o = np.concatenate([inside, outside, face])
    d = rng.normal(size=(len(o), 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    m = len(o)
    sel = rng.permutation(m)
    a = sel[: m // 6]                       # axis-aligned
    d[a] = 0
    d[a, rng.integers(0, 3, len(a))] = rng.choice([-1, 1], len(a)).astype(np.float32)
    z = sel[m // 6: m // 3]                 # one zero component
    d[z, rng.integers(0, 3, len(z))] = 0
    d[z] /= np.linalg.norm(d[z], axis=1, keepdims=True).astype(np.float32)
    rays = [bm.pack_rays(o, d * np.float32(scale))]
    per_cam = max(1, (n - m) // len(cams))
    side = int(np.sqrt(per_cam))
    for pos, h, v in cams:
        cam = bm.Camera(position=(pos[0] * G / 256, pos[1] * G / 256, pos[2] * H / 256), horizontal_angle=h, vertical_angle=v).update()
        px, py = np.meshgrid(np.linspace(0.5, 319.5, side, dtype=np.float32), np.linspace(0.5, 179.5, side, dtype=np.float32))
        rays.append(bm.camera_pixel_rays(cam, 320, 180, px.ravel(), py.ravel()))
    return np.concatenate(rays)


def oracle_hits(world, rays, campos=(0, 0, 0)):
    """intersect_voxel per ray, as bm_ray_hit records"""
    out = np.zeros(len(rays), RAY_HIT)
    cells = world.grid_size // 8
    for i, r in enumerate(rays):
        h = world.intersect_voxel(r["origin"], r["direction"], campos)
        if not h["hit"]:
            out[i] = (np.inf, (0, 0, 0), (-1, -1, -1), -1)
            continue
        b, s, lv = h["brick_id"], h["sub_id"], h["level"]
        v = np.array([b % cells, (b // cells) % cells, b // (cells * cells)]) * 8
        if lv == 2:
            v += [s & 7, (s >> 3) & 7, s >> 6]
        elif lv == 1:
            v += [4 * (s & 1), 4 * ((s >> 1) & 1), 4 * (s >> 2)]
        out[i] = (h["distance"], h["normal"], v, lv)
    return out


RAY_HIT = np.dtype([("distance", "<f4"), ("normal", "<f4", 3), ("voxel", "<i4", 3), ("level", "<i4")])


def assert_same_hits(got, want, what=""):
    g, w = got.view(RAY_HIT), want.view(RAY_HIT)
    bad = np.nonzero(g.view(np.uint32).reshape(-1, 8) != w.view(np.uint32).reshape(-1, 8))[0]
    assert len(bad) == 0, f"{what}: {len(np.unique(bad))} of {len(g)} rays differ, first: got {g[bad[0]]} want {w[bad[0]]}"


@pytest.fixture(scope="module")
def scene256(bm, torch_cuda):
    return bm.Scene(256, 256, device=0).generate().preload_all()


@pytest.fixture(scope="module")
def oracle256(orc):
    w = orc.World(256, 256)
    w.reset_device(True)
    return w


@pytest.mark.parametrize("dims", [(256, 256), (1024, 256)])
def test_exact_mode_matches_the_oracle(bm, orc, torch_cuda, dims, scene256, oracle256):
    G, H = dims
    if dims == (256, 256):
        scene, world = scene256, oracle256
    else:
        scene = bm.Scene(G, H, device=0).generate().preload_all()
        world = orc.World(G, H)
        world.reset_device(True)
    world.set_lod(INT_MAX, INT_MAX)
    rays = make_rays(bm, G, H, 10000, seed=G)
    got = scene.cast_rays(rays).packed
    want = oracle_hits(world, rays)
    assert (want["level"] == 2).sum() > len(rays) // 4 and (want["level"] == -1).sum() > 100  # both kinds are exercised
    assert_same_hits(got, want, f"exact {dims}")
    # torch input, packed on the device: the same records
    d_rays = torch_cuda.from_numpy(rays.view(np.float32).reshape(-1, 8)).cuda()
    res = scene.cast_rays(d_rays)
    torch_cuda.cuda.synchronize()
    assert res.packed.data_ptr() != d_rays.data_ptr() and res.level.dtype == torch_cuda.int32
    assert np.array_equal(res.packed.cpu().numpy().view(np.uint32), got.view(np.uint32).reshape(-1, 8))
    # ... and from separate origin / direction tensors
    res2 = scene.cast_rays(torch_cuda.from_numpy(rays["origin"].copy()).cuda(), torch_cuda.from_numpy(rays["direction"].copy()).cuda())
    torch_cuda.cuda.synchronize()
    assert np.array_equal(res2.distance.cpu().numpy(), got["distance"]) and np.array_equal(res2.voxel.cpu().numpy(), got["voxel"])


def test_direction_length_scales_the_distance_only(bm, scene256):
    """direction need not be unit length: the hit is the same cell and the distance scales by exactly 1 / s for a power of two s
    (walks with the largest component outside [0.5, 2) are rescaled by powers of two); other lengths give the same cells"""
    rays = make_rays(bm, 256, 256, 3000, seed=5)
    base = scene256.cast_rays(rays).packed
    for s in (2.0 ** -20, 2.0 ** -3, 4.0, 2.0 ** 30):
        r = rays.copy()
        r["direction"] *= np.float32(s)
        got = scene256.cast_rays(r).packed
        assert np.array_equal(got["level"], base["level"]) and np.array_equal(got["voxel"], base["voxel"])
        assert np.array_equal(got["normal"], base["normal"])
        assert np.array_equal(got["distance"], (base["distance"] / np.float32(s)).astype(np.float32)), f"scale {s}"
    r = rays.copy()
    r["direction"] *= np.float32(0.37)  # not a power of two: the walk rounds differently, the answers agree up to that rounding
    got = scene256.cast_rays(r).packed
    assert (got["level"] == base["level"]).mean() > 0.99
    hit = (got["level"] == 2) & (base["level"] == 2)
    assert np.allclose(got["distance"][hit] * np.float32(0.37), base["distance"][hit], rtol=1e-4, atol=1e-3)


def test_lod_mode_matches_the_oracle(bm, orc, torch_cuda):
    G, H = 1024, 256
    lod8, lod2 = 40 ** 2, 16 ** 2  # (cells^2: the worlds that fit a test are too small for the reference's 600000 / 100000)
    scene = bm.Scene(G, H, device=0).generate().preload_all()
    scene.set_lod(lod8, lod2)
    world = orc.World(G, H)
    world.reset_device(True)
    world.set_lod(lod8, lod2)
    rays = make_rays(bm, G, H, 8000, seed=11)
    origin = np.array([0.5 * G, 0.125 * G, 0.8 * H], np.float32)
    campos = [int(np.float32(v) / np.float32(8)) for v in origin]
    got = scene.cast_rays(rays, lod_origin=origin).packed
    want = oracle_hits(world, rays, campos)
    for lv in (0, 1, 2):
        assert (want["level"] == lv).sum() > 50, f"level {lv} does not occur"
    assert_same_hits(got, want, "LoD")


def requested_bits(scene, world=None):
    info = scene.info()
    got, want = [], []
    for sc in range(info["supercells"]):
        got.append(scene.device_indices(sc) & np.uint32(0x20000000))
        if world is not None:
            want.append(world.sc_dev_indices(sc) & np.uint32(0x20000000))
    return np.concatenate(got), (np.concatenate(want) if world is not None else None)


def all_device_indices(scene):
    return np.concatenate([scene.device_indices(sc) for sc in range(scene.info()["supercells"])])


@pytest.mark.parametrize("overlapped", [0, 1])
def test_streaming_reports_and_requests_like_the_oracle(bm, orc, torch_cuda, overlapped, oracle256):
    G = 256
    scene = bm.Scene(G, G, device=0)
    scene.set_queue_capacity(1 << 16)
    scene.set_streaming_mode(overlapped)
    scene.generate()
    world = orc.World(G, G)
    world.set_queue_cap(1 << 16)
    world.reset_device(False)
    world.set_lod(INT_MAX, INT_MAX)
    rays = make_rays(bm, G, G, 6000, seed=3)
    # BM_QUERY_NO_REQUESTS writes no index word
    before = all_device_indices(scene)
    quiet = scene.cast_rays(rays, request=False).packed
    assert np.array_equal(all_device_indices(scene), before)
    got = scene.cast_rays(rays).packed
    assert np.array_equal(quiet.view(np.uint32), got.view(np.uint32))
    want = oracle_hits(world, rays)
    assert (want["level"] == 3).sum() > 100
    assert_same_hits(got, want, "streaming")
    g, w = requested_bits(scene, world)
    assert np.array_equal(g, w), f"{int((g != w).sum())} index words differ in the REQUESTED bit"
    # serviced (twice per round in the overlapped mode: a request becomes resident one servicing later), the rays walk on; once no
    # brick along them is missing they give the preloaded answers
    oracle256.set_lod(INT_MAX, INT_MAX)
    full = oracle_hits(oracle256, rays)
    for _ in range(32):
        for _ in range(1 + overlapped):
            scene.process_load_queue()
        got = scene.cast_rays(rays).packed
        if not (got["level"] == 3).any():
            break
    assert_same_hits(got, full, "after servicing")


def column_tops(vol, x0, x1, y0, y1):
    """[y, x] -> z of the top solid voxel of each column of the host volume [z, y, x], -1 = empty column"""
    sub = vol[:, y0:y1, x0:x1]
    has = sub.any(axis=0)
    top = sub.shape[0] - 1 - np.argmax(sub[::-1], axis=0)
    return np.where(has, top, -1)


def world_voxels(scene):
    info = scene.info()
    sg, sgz = info["supergrid_xy"], info["supergrid_z"]
    v = np.zeros((sgz * 128, sg * 128, sg * 128), bool)
    for sc in range(info["supercells"]):
        idx, bricks = scene.host_supercell(sc)
        sx, sy, sz = sc % sg, (sc // sg) % sg, sc // (sg * sg)
        for cell in np.nonzero(idx)[0]:
            bits = np.unpackbits(bricks[idx[cell] & 0xFFF].view(np.uint8), bitorder="little").reshape(8, 8, 8).astype(bool)
            x, y, z = sx * 128 + (cell & 15) * 8, sy * 128 + ((cell >> 4) & 15) * 8, sz * 128 + (cell >> 8) * 8
            v[z:z + 8, y:y + 8, x:x + 8] = bits
    return v


def test_queries_see_edits_issued_on_another_stream(bm, torch_cuda):
    torch = torch_cuda
    G = 256
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    x0, x1, y0, y1 = 90, 170, 60, 140
    ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
    o = np.stack([xs + 0.5, ys + 0.5, np.full(xs.shape, G + 10.0)], -1).reshape(-1, 3).astype(np.float32)
    d = np.tile(np.array([0, 0, -1], np.float32), (len(o), 1))
    o0, d0 = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    s_edit, s_query = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    edits = [lambda s: scene.fill_box((100, 70, 120), (140, 110, 160), stream=s),
             lambda s: scene.carve_sphere((130, 100, 60), 25, stream=s),
             lambda s: scene.set_voxels(np.stack([rng.integers(x0, x1, 300), rng.integers(y0, y1, 300), rng.integers(100, 250, 300)], -1).astype(np.int32),
                                        rng.integers(0, 2, 300), stream=s)]
    for edit in edits:
        edit(s_edit.cuda_stream)
        # the inputs are computed on the current stream and dropped right after the call, the query runs on a third stream: cast_rays
        # orders it behind the current stream's work and keeps the inputs alive for it (no host synchronisation anywhere in between)
        d_o, d_d = o0 * 1.0, d0 + 0.0
        res = scene.cast_rays(d_o, d_d, stream=s_query.cuda_stream)
        del d_o, d_d
        clobber = torch.full((len(o), 8), float("nan"), device="cuda")  # may reuse the inputs' memory if they were released too early
        torch.cuda.synchronize()
        del clobber
        tops = column_tops(world_voxels(scene), x0, x1, y0, y1).reshape(-1)
        lv, vox = res.level.cpu().numpy(), res.voxel.cpu().numpy()
        assert np.array_equal(lv, np.where(tops >= 0, 2, -1))
        hit = tops >= 0
        assert np.array_equal(vox[hit, 2], tops[hit]) and np.array_equal(vox[hit, 0], (o[hit, 0]).astype(int))
        assert np.array_equal(vox[hit, 1], (o[hit, 1]).astype(int))
        assert np.array_equal(res.normal.cpu().numpy()[hit], np.tile([0, 0, 1], (int(hit.sum()), 1)).astype(np.float32))
    # pick, carve there, pick again through the same pixel: the new hit lies farther along the ray and outside the sphere
    cam = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
    first = scene.pick(cam, 40, 30, 96, 64)
    assert first is not None and first.level == 2
    scene.carve_sphere(first.voxel, 6)
    second = scene.pick(cam, 40, 30, 96, 64)
    assert second is not None and second.distance > first.distance
    assert sum((a - b) ** 2 for a, b in zip(second.voxel, first.voxel)) > 36


def test_tmax_filters_the_unbounded_result(bm, scene256):
    rays = make_rays(bm, 256, 256, 6000, seed=9)
    full = scene256.cast_rays(rays).packed
    d = full["distance"]
    rng = np.random.default_rng(2)
    fin = np.where(np.isfinite(d), d, np.float32(100))
    choices = {"zero": np.zeros(len(rays), np.float32), "equal": fin, "below": np.nextafter(fin, np.float32(0)),
               "random": rng.uniform(0, 300, len(rays)).astype(np.float32), "mixed": np.where(rng.integers(0, 2, len(rays)) == 1, fin, np.nextafter(fin, np.float32(-1)))}
    miss = np.zeros(1, RAY_HIT)
    miss[0] = (np.inf, (0, 0, 0), (-1, -1, -1), -1)
    for name, t in choices.items():
        r = rays.copy()
        r["tmax"] = t
        got = scene256.cast_rays(r).packed
        want = np.where(full["distance"] <= t, full, miss[0])
        assert_same_hits(got, want, f"tmax {name}")


def test_degenerate_rays_and_refusals(bm, torch_cuda, scene256):
    torch = torch_cuda
    o = np.array([[100, 100, 250]] * 8, np.float32)
    d = np.array([[np.nan, 0, -1], [0, 0, 0], [np.inf, 0, 0], [0, -np.inf, 1], [0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, -1]], np.float32)
    o[5, 0] = np.nan
    o[6, 2] = np.inf
    rays = bm.pack_rays(o, d)
    rays["reserved"][7] = 1
    got = scene256.cast_rays(rays).packed
    assert list(got["level"]) == [-1, -1, -1, -1, 2, -1, -1, -1]
    assert np.all(np.isinf(got["distance"][[0, 1, 2, 3, 5, 6, 7]])) and np.all(got["voxel"][[0, 1, 2, 3, 5, 6, 7]] == -1)
    assert np.all(got["normal"][[0, 1, 2, 3, 5, 6, 7]] == 0)

    L = bm.load()
    cam = bm.Camera(position=(128, 32, 204.8), horizontal_angle=0.8, vertical_angle=-0.5).update()
    params = bm.FrameParams(64, 48, spp=1, max_bounces=2, flags=bm.BM_FLAG_ORDERED)

    def frame():
        acc = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
        scene256.render(cam, params, acc)
        torch.cuda.synchronize()
        return acc.cpu().numpy()

    img = frame()
    info = scene256.info()
    d_rays = torch.from_numpy(bm.pack_rays(np.array([[128, 128, 250]], np.float32), np.array([[0, 0, -1]], np.float32)).view(np.float32).reshape(1, 8)).cuda()
    hits = torch.full((4, 8), 7.0, dtype=torch.float32, device="cuda:0")
    origin = (C.c_float * 3)(1, 2, 3)
    h, rp, hp, st = scene256.gpuScene, C.c_void_p(d_rays.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(0)
    assert L.bm_scene_cast_rays(h, -1, rp, hp, 0, None, st) == EINVAL
    assert L.bm_scene_cast_rays(h, (1 << 28) + 1, rp, hp, 0, None, st) == EINVAL
    assert L.bm_scene_cast_rays(h, 1, None, hp, 0, None, st) == EINVAL
    assert L.bm_scene_cast_rays(h, 1, rp, None, 0, None, st) == EINVAL
    assert L.bm_scene_cast_rays(h, 1, rp, hp, 4, None, st) == EINVAL                  # unknown flag
    assert L.bm_scene_cast_rays(h, 1, rp, hp, bm.BM_QUERY_LOD, None, st) == EINVAL    # LoD without an origin
    bad = (C.c_float * 3)(1, float("nan"), 3)
    assert L.bm_scene_cast_rays(h, 1, rp, hp, bm.BM_QUERY_LOD, bad, st) == EINVAL
    assert L.bm_scene_cast_rays(h, 0, None, None, 0, None, st) == 0                    # n == 0: a no-op
    torch.cuda.synchronize()
    assert torch.all(hits == 7.0), "a refused call wrote results"
    assert scene256.info() == info
    assert np.array_equal(frame(), img)
    assert L.bm_scene_cast_rays(h, 1, rp, hp, bm.BM_QUERY_LOD, origin, st) == 0
    torch.cuda.synchronize()
    assert torch.all(hits[1:] == 7.0) and int(hits[0, 7].view(torch.int32)) == 2     # one record written, at the ray's index
    # a scene that is not on the device
    fresh = bm.Scene(256, 256, device=0)
    assert L.bm_scene_cast_rays(fresh.gpuScene, 1, rp, hp, 0, None, st) == ESTATE


def test_headless_main_dig_at(bm, torch_cuda):
    exe = os.path.join(ROOT, "examples", "headless_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    r = subprocess.run([exe, "--dig-at", "80,40,5", "256", "256", "160", "96", "2", os.devnull], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"picked voxel (-?\d+),(-?\d+),(-?\d+) level (-?\d+)", r.stdout)
    assert m, r.stdout
    voxel, level = tuple(int(m.group(k)) for k in (1, 2, 3)), int(m.group(4))
    assert level == 2
    # the example carved: the same pixel now sees a voxel outside the sphere (or nothing)
    m2 = re.search(r"carved radius 5 at (-?\d+),(-?\d+),(-?\d+); the pixel now sees voxel (-?\d+),(-?\d+),(-?\d+) level (-?\d+)", r.stdout)
    assert m2, r.stdout
    assert tuple(int(m2.group(k)) for k in (1, 2, 3)) == voxel
    after, after_level = tuple(int(m2.group(k)) for k in (4, 5, 6)), int(m2.group(7))
    assert after_level == -1 or (after_level == 2 and sum((a - b) ** 2 for a, b in zip(after, voxel)) > 25)
    # the same pick through Python on a fresh (streaming) scene, then the same carve: that voxel is empty in the host world
    scene = bm.Scene(256, 256, device=0).generate()
    cam = bm.Camera(position=(128, 32, 0.8 * 256), horizontal_angle=0.8, vertical_angle=-0.5).update()
    hit = scene.pick(cam, 80, 40, 160, 96)
    for _ in range(8):
        if hit is None or hit.level != 3:
            break
        scene.process_load_queue()
        hit = scene.pick(cam, 80, 40, 160, 96)
    assert hit is not None and hit.voxel == voxel and hit.level == 2
    assert world_voxels(scene)[voxel[2], voxel[1], voxel[0]]
    scene.carve_sphere(hit.voxel, 5)
    assert not world_voxels(scene)[voxel[2], voxel[1], voxel[0]]
    again = scene.pick(cam, 80, 40, 160, 96)
    for _ in range(8):
        if again is None or again.level != 3:
            break
        scene.process_load_queue()
        again = scene.pick(cam, 80, 40, 160, 96)
    assert (again is None and after_level == -1) or (again.voxel == after and again.level == after_level)
