"""Scene.query_volumes on the MI355X (the kernels of csrc/volume.hip): for batches of boxes and spheres, the number of solid voxels, their
tight bounds and the unresolved brick cells, against numpy on Scene.voxels().  For a box the model is vox[z0:z1, y0:y1, x0:x1] -- its
sum and the min / max of np.nonzero; for a sphere the integer inequality in int64.  Every number is an integer and every comparison
exact."""
import ctypes as C
import time

import numpy as np
import pytest

from _edit_model import LOADED, all_device_words, model_sphere, occupancy
from test_gpu_edit import CAM, G, render

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = 10001, 10002
BOX, SPHERE = 1, 2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def preloaded(bm, torch_cuda):
    """the generated 256^3 world, every brick resident, and its voxels"""
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    vox = scene.voxels().view(np.uint8).copy()
    yield scene, vox
    scene.close()


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_volume.py took {time.time() - t0:.1f} s")


# ---------------------------------------------------------------- the model
def malformed(rec):
    if rec["reserved"] != 0 or rec["shape"] not in (BOX, SPHERE):
        return True
    if rec["shape"] == BOX:
        return bool((rec["hi"] < rec["lo"]).any())
    return bool(rec["radius"] < 0)


def cover_of(rec, dims):
    """(x0, y0, z0), mask [z, y, x] of the record's voxels inside the world (mask None = the whole clipped box), or None when nothing is left"""
    if rec["shape"] == BOX:
        a, b = rec["lo"].astype(np.int64), rec["hi"].astype(np.int64)
    else:
        c, r = rec["center"].astype(np.int64), int(rec["radius"])
        a, b = c - r, c + r + 1
    a, b = np.clip(a, 0, dims), np.clip(b, 0, dims)
    if (a >= b).any():
        return None
    if rec["shape"] == BOX:
        return a, b, None
    d = [(np.arange(a[k], b[k], dtype=np.int64) - c[k]) ** 2 for k in range(3)]
    mask = d[2][:, None, None] + d[1][None, :, None] + d[0][None, None, :] <= np.int64(r) * np.int64(r)
    return a, b, mask


def model_results(bm, vox, recs, resident=None):
    """bm_volume_result records of the model: vox = the world [z, y, x]; resident = None (every brick) or bool [cz, cy, cx]"""
    Z, Y, X = vox.shape
    dims = np.array([X, Y, Z], np.int64)
    seen = vox if resident is None else vox * np.repeat(np.repeat(np.repeat(resident, 8, 0), 8, 1), 8, 2)
    missing = None if resident is None else occupancy(vox) & ~resident
    out = np.zeros(len(recs), bm.VOLUME_RESULT_DTYPE)
    out["lo"] = out["hi"] = -1
    for i, rec in enumerate(recs):
        if malformed(rec):
            out["status"][i] = 1
            continue
        cover = cover_of(rec, dims)
        if cover is None:
            continue
        a, b, mask = cover
        sub = seen[a[2]:b[2], a[1]:b[1], a[0]:b[0]]
        if mask is not None:
            sub = sub * mask
        solid = int(sub.sum(dtype=np.int64))
        out["solid"][i] = solid
        if solid:
            nz = np.nonzero(sub)
            out["lo"][i] = [a[0] + nz[2].min(), a[1] + nz[1].min(), a[2] + nz[0].min()]
            out["hi"][i] = [a[0] + nz[2].max() + 1, a[1] + nz[1].max() + 1, a[2] + nz[0].max() + 1]
        if missing is not None:
            c0, c1 = a >> 3, ((b - 1) >> 3) + 1
            cells = missing[c0[2]:c1[2], c0[1]:c1[1], c0[0]:c1[0]]
            if mask is not None:  # the cells that hold a voxel of the sphere
                full = np.zeros(tuple(8 * (c1[k] - c0[k]) for k in (2, 1, 0)), bool)
                o = a - 8 * c0
                full[o[2]:o[2] + mask.shape[0], o[1]:o[1] + mask.shape[1], o[0]:o[0] + mask.shape[2]] = mask
                cells = cells & occupancy(full)
            out["unresolved"][i] = int(cells.sum())
    return out


def assert_results(got, want, any_mode=False, what=""):
    if any_mode:
        want = want.copy()
        solid = want["solid"] > 0
        want["unresolved"] = (~solid & (want["unresolved"] > 0)).astype(np.uint32)
        want["solid"] = solid
        want["lo"] = want["hi"] = -1
    for name in ("status", "solid", "unresolved", "lo", "hi"):
        bad = np.nonzero((got[name] != want[name]).reshape(len(want), -1).any(1))[0]
        assert len(bad) == 0, f"{what}{name}: {len(bad)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def resident_cells(scene):
    """bool [cz, cy, cx]: the device index word of the cell has the loaded bit"""
    info = scene.info()
    sg, sgz = info["supergrid_xy"], info["supergrid_z"]
    loaded = (all_device_words(scene) & np.uint32(LOADED)) != 0
    return loaded.reshape(sgz, sg, sg, 16, 16, 16).transpose(0, 3, 1, 4, 2, 5).reshape(sgz * 16, sg * 16, sg * 16)


def mixed_records(bm, rng, size, n_small=16000, big_spheres=True):
    """single voxels, boxes inside one cell, boxes across the supercell corner, boxes clipped by every face, boxes outside, empty boxes,
    the whole world, spheres of radius 0, 1, 7, 40 and 200 (some centred outside), and malformed records of each kind in between"""
    parts = []
    p = rng.integers(0, size, (n_small // 4, 3))
    parts.append(bm.volume_box(p, p + 1))                                                   # single voxels
    c = rng.integers(0, size // 8, (n_small // 4, 3)) * 8
    a = rng.integers(0, 8, (n_small // 4, 3))
    parts.append(bm.volume_box(c + a, c + a + rng.integers(0, 9, a.shape).clip(0, 8 - a)))  # inside one cell (some empty)
    p = rng.integers(-20, size + 10, (n_small // 2, 3))
    parts.append(bm.volume_box(p, p + rng.integers(0, 24, p.shape)))                        # small boxes anywhere, across the faces too
    p = 128 - rng.integers(1, 40, (300, 3))
    parts.append(bm.volume_box(p, 128 + rng.integers(1, 40, p.shape)))                      # across the supercell corner on x, y and z
    for k in range(3):                                                                      # clipped by every face
        for side in (0, 1):
            lo = rng.integers(20, size - 60, (40, 3))
            hi = lo + rng.integers(1, 60, lo.shape)
            if side:
                hi[:, k] = size + rng.integers(0, 50, 40)
            else:
                lo[:, k] = -rng.integers(0, 50, 40)
            parts.append(bm.volume_box(lo, hi))
    far = rng.integers(size + 1, size + 1000, (100, 3)) * rng.choice([-1, 1], (100, 3))
    parts.append(bm.volume_box(far, far + 9))                                               # wholly outside
    parts.append(bm.volume_box([(2 ** 31 - 10, 0, 0), (-2 ** 31, -2 ** 31, -2 ** 31)], [(2 ** 31 - 1, 9, 9), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]))
    parts.append(bm.volume_box((0, 0, 0), (size, size, size)))                              # the whole world
    for radius, count in ((0, 1200), (1, 1200), (7, 1200), (40, 120), (200, 6 if big_spheres else 0)):
        if count:
            parts.append(bm.volume_sphere(rng.integers(-radius - 5, size + radius + 5, (count, 3)), radius))
    parts.append(bm.volume_sphere([(size // 2, size // 2, 2 ** 31 - 1), (-2 ** 31, 5, 5), (2 ** 24 + 3, 100, 100)], [2 ** 31 - 1, 2 ** 31 - 1, 2 ** 24]))
    recs = np.concatenate(parts)
    recs = recs[rng.permutation(len(recs))]
    bad = rng.choice(len(recs), 400, replace=False)                                         # malformed records of each kind, interleaved
    for j, i in enumerate(bad):
        kind = j % 5
        if kind == 0:
            recs["shape"][i] = rng.choice([0, 3, -1, 77])
        elif kind == 1:
            recs[i] = bm.volume_box((10, 10, 10), (20, 9, 20))[0]
        elif kind == 2:
            recs[i] = bm.volume_sphere((50, 50, 50), -1)[0]
        elif kind == 3:
            recs["reserved"][i] = 1 + j
        else:
            recs[i] = bm.volume_box((10, 10, 10), (9, 20, 20))[0]
    return recs


# ---------------------------------------------------------------- tests
def test_mixed_batch_in_a_preloaded_scene(bm, torch_cuda, preloaded):
    scene, vox = preloaded
    recs = np.concatenate([mixed_records(bm, np.random.default_rng(71), G), bm.volume_box((0, 0, 0), (G, G, G))])
    assert len(recs) >= 20000
    want = model_results(bm, vox, recs)
    assert (want["status"] == 1).sum() >= 400 and (want["solid"] > 0).sum() > 2000
    got = scene.query_volumes(recs)
    assert_results(got.packed, want)
    whole = np.nonzero((recs["shape"] == BOX) & (recs["lo"] == 0).all(1) & (recs["hi"] == G).all(1) & (recs["reserved"] == 0))[0]
    assert len(whole) >= 1 and int(got.solid[whole[0]]) == int(vox.sum(dtype=np.int64)) and int(got.unresolved[whole[0]]) == 0
    assert (got.unresolved == 0).all()
    # the same records as a yes / no probe
    assert_results(scene.query_volumes(recs, any=True).packed, want, any_mode=True, what="BM_VOLUME_ANY ")
    # tensors in, tensors out: the results stay on the device
    torch = torch_cuda
    t = torch.from_numpy(recs.view(np.uint8).reshape(-1, 48)).to("cuda:0")
    res = scene.query_volumes(t)
    assert res.packed.is_cuda and res.solid.dtype == torch.int64
    assert_results(res.packed.cpu().numpy().view(bm.VOLUME_RESULT_DTYPE).reshape(-1), want, what="tensor ")
    assert np.array_equal(res.solid.cpu().numpy(), want["solid"].astype(np.int64)) and np.array_equal(res.lo.cpu().numpy(), want["lo"])
    assert np.array_equal(res.hi.cpu().numpy(), want["hi"]) and np.array_equal(res.status.cpu().numpy(), want["status"].astype(np.int32))


def test_one_box_from_python(bm, torch_cuda, preloaded):
    scene, vox = preloaded
    assert scene.count_box((30, 40, 50), (100, 90, 200)) == int(vox[50:200, 40:90, 30:100].sum())
    ball = np.zeros_like(vox)
    model_sphere(ball, "set", (120, 130, 60), 33)
    assert scene.count_sphere((120, 130, 60), 33) == int((vox & ball).sum())
    assert scene.is_free((0, 0, G - 8), (G, G, G)) == (not vox[G - 8:].any())
    assert not scene.is_free((0, 0, 0), (G, G, 8)) and vox[:8].any()
    assert scene.query_volumes(np.zeros(0, bm.VOLUME_DTYPE)).packed.shape == (0,)


def test_queries_are_ordered_with_edits_and_writes(bm, torch_cuda):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    v0 = scene.voxels().view(np.uint8).copy()
    rng = np.random.default_rng(5)
    p = rng.integers(0, G - 30, (3000, 3))
    ball_c, ball_r = (250, 128, 230), 30  # in the sky, clipped by the world's +x and +z faces
    recs = np.concatenate([bm.volume_sphere(ball_c, ball_r), bm.volume_box((0, 0, 0), (G, G, G)), bm.volume_box(p, p + rng.integers(1, 30, p.shape))])
    t = torch.from_numpy(recs.view(np.uint8).reshape(-1, 48)).to("cuda:0")
    V = (rng.random((40, 50, 60)) < 0.4).astype(np.uint8)
    tv = torch.from_numpy(V).to("cuda:0")
    side = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    results = [scene.query_volumes(t, stream=side.cuda_stream)]  # no host synchronisation from here on
    scene.fill_sphere(ball_c, ball_r)
    results.append(scene.query_volumes(t, stream=side.cuda_stream))
    scene.carve_sphere((100, 100, 60), 45)
    results.append(scene.query_volumes(t, stream=side.cuda_stream))
    scene.write_region((90, 80, 70), tv, "replace")
    results.append(scene.query_volumes(t, stream=side.cuda_stream))
    torch.cuda.synchronize()
    models = [v0.copy()]
    models.append(models[-1].copy())
    model_sphere(models[-1], "set", ball_c, ball_r)
    models.append(models[-1].copy())
    model_sphere(models[-1], "clear", (100, 100, 60), 45)
    models.append(models[-1].copy())
    models[-1][70:110, 80:130, 90:150] = V
    assert np.array_equal(scene.voxels().view(np.uint8), models[-1])
    for k, (res, model) in enumerate(zip(results, models)):
        assert_results(res.packed.cpu().numpy().view(bm.VOLUME_RESULT_DTYPE).reshape(-1), model_results(bm, model, recs), what=f"query {k}: ")
    ball = np.zeros_like(v0)
    model_sphere(ball, "set", ball_c, ball_r)
    assert not (v0 & ball).any() and int(results[1].solid[0]) == int(ball.sum()), "the sphere just filled holds the clipped sphere's voxels"
    assert int(results[0].solid[0]) == 0
    scene.close()


def test_streaming_scene_counts_what_is_resident(bm, torch_cuda):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0)
    scene.set_queue_capacity(1 << 16)
    scene.generate().reset_residency()
    cam = bm.Camera(**CAM).update()
    for _ in range(3):
        render(bm, torch, scene, cam)
        scene.process_load_queue()
    info = scene.info()
    assert 0 < info["resident_bricks"] < info["total_bricks"]
    vox = scene.voxels().view(np.uint8).copy()
    words = all_device_words(scene)
    resident = resident_cells(scene)
    recs = mixed_records(bm, np.random.default_rng(72), G, n_small=6000, big_spheres=False)
    recs = np.concatenate([recs, bm.volume_sphere([(128, 128, 100), (40, 300, 90)], 200), bm.volume_box((-3, 5, 17), (141, 259, 203))])
    want = model_results(bm, vox, recs, resident)
    assert (want["unresolved"] > 0).sum() > 100 and (want["solid"] > 0).sum() > 100
    loads = scene.info()["stream_batches"]
    assert_results(scene.query_volumes(recs).packed, want, what="streaming ")
    assert_results(scene.query_volumes(recs, any=True).packed, want, any_mode=True, what="streaming BM_VOLUME_ANY ")
    assert np.array_equal(all_device_words(scene), words), "a volume query wrote an index word"
    assert scene.process_load_queue() == 0 and scene.info()["stream_batches"] == loads, "a volume query filed a brick request"
    scene.preload_all()
    got = scene.query_volumes(recs)
    assert_results(got.packed, model_results(bm, vox, recs), what="after preload_all ")
    assert (got.unresolved == 0).all()
    scene.close()


def test_random_world_of_partially_filled_bricks(bm, torch_cuda):
    rng = np.random.default_rng(73)
    size = 128
    vox = (rng.random((size, size, size)) < 0.3).astype(np.uint8)
    vox[40:80, 30:70, 50:120] = 0  # and a hole of empty cells
    scene = bm.Scene.from_voxels(vox)
    recs = mixed_records(bm, rng, size, n_small=4000, big_spheres=False)
    recs = np.concatenate([recs, bm.volume_sphere([(64, 64, 64), (0, 130, 20)], [200, 90])])
    want = model_results(bm, vox, recs)
    assert_results(scene.query_volumes(recs).packed, want, what="random world ")
    assert_results(scene.query_volumes(recs, any=True).packed, want, any_mode=True, what="random world BM_VOLUME_ANY ")
    scene.close()


def test_sweep_box_against_translate_and_test(bm, torch_cuda, preloaded):
    scene, vox = preloaded
    rng = np.random.default_rng(74)
    n = 2000
    lo = rng.integers(-10, G - 4, (n, 3))
    lo[:, 2] = rng.integers(40, G + 6, n)  # mostly above the ground, so that sweeps have room
    hi = lo + rng.integers(1, 15, (n, 3))
    axis, sign = np.arange(n) % 3, np.where((np.arange(n) // 3) % 2 == 0, 1, -1)
    dist = rng.integers(0, 60, n)
    d, unresolved = scene.sweep_box(lo, hi, axis, sign, dist)
    assert (unresolved == 0).all()
    pad = np.zeros((G + 200, G + 200, G + 200), np.uint8)  # the world with 100 empty voxels all round
    pad[100:100 + G, 100:100 + G, 100:100 + G] = vox
    for i in range(n):
        want = 0
        for k in range(1, int(dist[i]) + 1):
            a, b = lo[i].copy(), hi[i].copy()
            a[axis[i]] += sign[i] * k
            b[axis[i]] += sign[i] * k
            a, b = np.clip(a + 100, 0, G + 200), np.clip(b + 100, 0, G + 200)
            if pad[a[2]:b[2], a[1]:b[1], a[0]:b[0]].any():
                break
            want = k
        assert int(d[i]) == want, (i, lo[i], hi[i], axis[i], sign[i], dist[i], int(d[i]), want)
    assert len(set(zip(axis.tolist(), sign.tolist()))) == 6 and (d < dist).sum() > 50 and (d == dist).sum() > 50
    left = (lo[np.arange(n), axis] - dist < 0) | (hi[np.arange(n), axis] + dist > G)
    assert left.sum() > 50, "some sweeps leave the world"
    # one box, scalars: down onto the ground
    x, y = 100, 60
    top = int(np.nonzero(vox[:, y:y + 6, x:x + 6].any(axis=(1, 2)))[0].max())
    assert scene.sweep_box((x, y, top + 21), (x + 6, y + 6, top + 35), 2, -1, 100) == (20, 0)


def test_refusals(bm, torch_cuda, preloaded):
    torch = torch_cuda
    scene, vox = preloaded
    L = bm._lib.load()
    recs = bm.volume_box((0, 0, 0), (G, G, G))
    t = torch.from_numpy(recs.view(np.uint8).reshape(-1, 48)).to("cuda:0")
    out = torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    vp, rp = C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())
    fresh = bm.Scene(G, G, device=0)
    cases = {
        "n < 0": (scene, -1, vp, rp, 0, EINVAL),
        "n > 2^24": (scene, (1 << 24) + 1, vp, rp, 0, EINVAL),
        "null volumes": (scene, 1, None, rp, 0, EINVAL),
        "null results": (scene, 1, vp, None, 0, EINVAL),
        "unknown flags": (scene, 1, vp, rp, 2, EINVAL),
        "unknown flags beside a known one": (scene, 1, vp, rp, 1 | 1 << 31, EINVAL),
        "a scene not on the device": (fresh, 1, vp, rp, 0, ESTATE),
    }
    for name, (s, n, v, r, flags, code) in cases.items():
        assert L.bm_scene_query_volumes(s.gpuScene, n, v, r, flags, stream) == code, name
        torch.cuda.synchronize()
        assert (out == 0xAB).all(), f"{name}: something was written"
        assert L.bm_scene_query_volumes(scene.gpuScene, 1, vp, rp, 0, stream) == 0  # and a valid query still answers
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(bm.VOLUME_RESULT_DTYPE)[0]
        assert int(got["solid"]) == int(vox.sum(dtype=np.int64)) and int(got["status"]) == 0
        out.fill_(0xAB)
    assert L.bm_scene_query_volumes(scene.gpuScene, 0, None, None, 0, stream) == 0, "n == 0 is a no-op"
    fresh.close()
