"""Scene.write_region / Scene.read_region on the MI355X: a dense box of voxels written into and read out of a live scene, from and to
torch tensors on the GPU (the pack / unpack kernels of csrc/region.hip) and numpy arrays.  The device world is compared cell by cell
with a numpy model that the tests edit alongside (assert_device_world), the cube field with the host build, frames and queries with a
scene built afresh from the model.  Every comparison of voxels, words, bricks, field bytes and hit records is exact."""
import ctypes as C
import time

import numpy as np
import pytest

from _edit_model import LOADED, REQUESTED, all_device_words, assert_device_world, cell_of, changed_bricks
from test_gpu_edit import CAM, G, assert_radiance, render
from test_region_host import model_write

pytestmark = pytest.mark.gpu
EINVAL = 10001


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def terrain(bm, torch_cuda):
    """voxels of the generated 256^3 world"""
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    vox = scene.voxels().view(np.uint8).copy()
    scene.close()
    return vox


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_region.py took {time.time() - t0:.1f} s")


def volume_for(rng, shape, fill=0.5):
    return (rng.random(shape) < fill).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)


def assert_fields_equal(scene):
    dev, host = scene.device_cube_field(), scene.host_cube_field()
    assert np.array_equal(dev, host), f"{np.count_nonzero(dev != host)} field bytes differ from the host build"


def whole_world(scene, device):
    size, height = scene.grid_size, scene.grid_height
    got = scene.read_region((0, 0, 0), (size, size, height), device=device)
    return got.cpu().numpy() if device else got.view(np.uint8)


# lo, (nz, ny, nx) of the written boxes in the 256^3 world
BOXES = {
    "aligned": ((32, 16, 40), (48, 64, 64)),              # lo.x a multiple of 16, a contiguous tensor: 16-byte loads
    "general": ((35, 21, 77), (37, 45, 51)),
    "across a supercell corner": ((100, 110, 120), (30, 40, 50)),  # crosses 128 on x, y and z
    "clipped by the world's edge": ((230, -7, 240), (40, 30, 50)),
}


@pytest.mark.parametrize("op", ["replace", "set", "clear"])
def test_device_write_into_a_preloaded_scene(op, bm, torch_cuda, terrain):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    model = terrain.copy()
    rng = np.random.default_rng(len(op))
    for name, (lo, shape) in BOXES.items():
        V = volume_for(rng, shape)
        t = torch.from_numpy(V).to("cuda:0")
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
        scene.write_region(lo, t, op)
        model = model_write(model, lo, V, op)
        ms = scene.last_region_ms()
        print(f"{op}, {name}: pack {ms[0]:.3f} copy {ms[1]:.3f} scatter {ms[2]:.3f} field {ms[3]:.3f} ms", flush=True)
    loaded = assert_device_world(scene, model)
    assert loaded == scene.info()["total_bricks"]
    assert_fields_equal(scene)
    assert np.array_equal(whole_world(scene, True), model)
    assert np.array_equal(whole_world(scene, False), model)
    assert np.array_equal(scene.voxels().view(np.uint8), model)
    scene.close()


def test_a_write_that_makes_a_pool_grow(bm, torch_cuda):
    """512 x 512 x 256 voxels: more bricks than the arena's smallest size, so the preloaded arena is an exact fit and a pool that grows
    makes the arena grow"""
    torch = torch_cuda
    scene = bm.Scene(512, 256, device=0).generate().preload_all()
    model = scene.voxels().view(np.uint8).copy()
    info = scene.info()
    assert info["total_bricks"] > 1 << 16, "the world is too small for the case"
    lo, shape = (130, 260, 200), (50, 100, 100)  # sky of one supercell of the upper layer
    assert not model[lo[2]:lo[2] + shape[0], lo[1]:lo[1] + shape[1], lo[0]:lo[0] + shape[2]].any()
    V = volume_for(np.random.default_rng(3), shape, 0.2)
    scene.write_region(lo, torch.from_numpy(V).to("cuda:0"), "set")
    model = model_write(model, lo, V, "set")
    after = scene.info()
    assert after["arena_growths"] > info["arena_growths"] and after["pool_bytes"] > info["pool_bytes"], (info, after)
    assert after["total_bricks"] > info["total_bricks"] and after["resident_bricks"] == after["total_bricks"]
    assert_device_world(scene, model)
    assert_fields_equal(scene)
    assert np.array_equal(whole_world(scene, True), model)
    scene.close()


def test_device_write_equals_host_write(bm, torch_cuda, terrain):
    torch = torch_cuda
    a, b = bm.Scene.from_voxels(terrain), bm.Scene.from_voxels(terrain)
    rng = np.random.default_rng(11)
    for op in ("clear", "replace", "set", "replace"):
        for lo, shape in BOXES.values():
            V = volume_for(rng, shape, 0.4)
            a.write_region(lo, torch.from_numpy(V).to("cuda:0"), op)
            b.write_region(lo, V, op)
    for sc in range(a.info()["supercells"]):
        (ia, ba), (ib, bb) = a.host_supercell(sc), b.host_supercell(sc)
        assert np.array_equal(ia, ib) and np.array_equal(ba, bb), f"supercell {sc}: host worlds differ"
        assert np.array_equal(a.device_indices(sc), b.device_indices(sc)), f"supercell {sc}: device words differ"
    a.close()
    b.close()


def test_frames_and_queries_equal_a_fresh_build(bm, torch_cuda, terrain):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    model = terrain.copy()
    rng = np.random.default_rng(12)
    # in what the camera sees: a carved block, a block of sky filled, random content around the surface
    for op, lo, shape, fill in (("clear", (100, 70, 60), (140, 90, 60), 0.7), ("set", (140, 44, 180), (14, 20, 22), 0.5), ("replace", (83, 61, 100), (70, 77, 91), 0.5)):
        V = volume_for(rng, shape, fill)
        scene.write_region(lo, torch.from_numpy(V).to("cuda:0"), op)
        model = model_write(model, lo, V, op)
    ref = bm.Scene.from_voxels(model)
    cam = bm.Camera(**CAM).update()
    got, want = render(bm, torch, scene, cam), render(bm, torch, ref, cam)
    assert np.array_equal(got[1], want[1]), f"{np.count_nonzero((got[1] != want[1]).any(-1))} pixels whose hit records differ"
    assert got[2] == want[2]
    assert_radiance(got[0], want[0])
    px, py = np.meshgrid(np.arange(0.5, 96, 1.5), np.arange(0.5, 64, 1.5))
    rays = bm.camera_pixel_rays(cam, 96, 64, px.ravel(), py.ravel())
    assert scene.cast_rays(rays).packed.tobytes() == ref.cast_rays(rays).packed.tobytes()
    ref.close()
    scene.close()


def mixed_residency(bm, torch, overlapped=0):
    scene = bm.Scene(G, G, device=0)
    scene.set_queue_capacity(1 << 16)
    scene.generate().set_streaming_mode(overlapped)
    cam = bm.Camera(**CAM).update()
    for _ in range(2):
        render(bm, torch, scene, cam)
        scene.process_load_queue()
    info = scene.info()
    assert 0 < info["resident_bricks"] < info["total_bricks"]
    return scene, cam


def test_write_and_read_of_a_streaming_scene(bm, torch_cuda, terrain):
    torch = torch_cuda
    scene, cam = mixed_residency(bm, torch)
    model = terrain.copy()
    info = scene.info()
    render(bm, torch, scene, cam)  # requests stand in the ring, not serviced yet
    words = all_device_words(scene)
    assert (words & np.uint32(REQUESTED)).any() and (words & np.uint32(LOADED)).any()
    # a box over resident, requested, unloaded and empty cells; inside it: requested bricks emptied, cells left as they are
    lo, hi = (60, 40, 30), (200, 170, 220)
    V = model[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].copy()
    cells = np.stack(np.meshgrid(np.arange(lo[0] // 8 + 1, hi[0] // 8 - 1), np.arange(lo[1] // 8 + 1, hi[1] // 8 - 1), np.arange(lo[2] // 8 + 1, hi[2] // 8 - 1), indexing="ij"), -1).reshape(-1, 3)
    sg = info["supergrid_xy"]
    word_of = lambda c: int(words[((c[0] >> 4) + (c[1] >> 4) * sg + (c[2] >> 4) * sg * sg) * 4096 + (c[0] & 15) + (c[1] & 15) * 16 + (c[2] & 15) * 256])
    requested = [c for c in cells if word_of(c) & REQUESTED]
    resident = [c for c in cells if word_of(c) & LOADED]
    assert len(requested) >= 8 and len(resident) >= 8
    emptied, kept_requested, rewritten = requested[::2], requested[1::2], resident[::2]
    for c in emptied:
        x, y, z = (int(v) * 8 for v in c)
        V[z - lo[2]:z - lo[2] + 8, y - lo[1]:y - lo[1] + 8, x - lo[0]:x - lo[0] + 8] = 0
    for c in rewritten:
        x, y, z = (int(v) * 8 for v in c)
        V[z - lo[2] + 1, y - lo[1] + 2, x - lo[0] + 3] ^= 1
    scene.write_region(lo, torch.from_numpy(V).to("cuda:0"), "replace")
    new_model = model_write(model, lo, V, "replace")
    changed = changed_bricks(model, new_model)
    assert len(changed) == len(emptied) + len(rewritten)
    assert_device_world(scene, new_model, changed)
    after = all_device_words(scene)
    changed_set = {tuple(int(v) for v in c) for c in changed}
    same = np.array([cell_of(info, i // 4096, i % 4096) not in changed_set for i in range(len(words))])
    assert np.array_equal(after[same], words[same]), "a cell whose bits did not change has another device word"
    words = after
    assert all(word_of(c) & REQUESTED for c in kept_requested), "an unchanged requested brick lost its requested bit"
    assert all(word_of(c) == 0 for c in emptied)
    # read back over resident, non-resident and empty cells, into device and host memory
    for rlo, rhi in ((lo, hi), ((-3, 5, 17), (141, 259, 203)), ((0, 0, 0), (G, G, G))):
        full = np.zeros((G + 16, G + 16, G + 16), np.uint8)
        full[8:8 + G, 8:8 + G, 8:8 + G] = scene.voxels()
        want = full[rlo[2] + 8:rhi[2] + 8, rlo[1] + 8:rhi[1] + 8, rlo[0] + 8:rhi[0] + 8]
        got = scene.read_region(rlo, rhi, device=True)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(scene.read_region(rlo, rhi).view(np.uint8), want)
    # the ring still names the emptied bricks: they are skipped
    scene.process_load_queue()
    assert not scene.info()["failed"]
    for _ in range(64):
        render(bm, torch, scene, cam)
        if scene.process_load_queue() == 0 and scene.process_load_queue() == 0:
            break
    else:
        pytest.fail("streaming did not reach a steady state")
    assert_device_world(scene, new_model)
    ref = bm.Scene.from_voxels(new_model)
    got, want = render(bm, torch, scene, cam), render(bm, torch, ref, cam)
    assert np.array_equal(got[1], want[1])
    ref.close()
    scene.close()


def test_write_is_ordered_between_frame_launches(bm, torch_cuda, terrain):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    cam = bm.Camera(**CAM).update()
    lo, shape = (100, 70, 60), (140, 90, 60)
    V = np.ones(shape, np.uint8)
    model = model_write(terrain, lo, V, "clear")
    old, new = bm.Scene.from_voxels(terrain), bm.Scene.from_voxels(model)
    want_old, want_new = render(bm, torch, old, cam), render(bm, torch, new, cam)
    assert not np.array_equal(want_old[1], want_new[1])
    W, H, n = 96, 64, 3
    p = [bm.FrameParams(W, H, spp=1, max_bounces=3, flags=bm.BM_FLAG_ORDERED) for _ in range(n)]
    accs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2 * n)]
    dbgs = [torch.zeros((H, W, 8), dtype=torch.int32, device="cuda:0") for _ in range(2 * n)]
    t = torch.from_numpy(V).to("cuda:0")
    torch.cuda.synchronize()
    scene.render_frames(cam, p, accs[:n], debugs=dbgs[:n])
    scene.write_region(lo, t, "clear")  # no synchronisation in between
    scene.render_frames(cam, p, accs[n:], debugs=dbgs[n:])
    torch.cuda.synchronize()
    for k in range(2 * n):
        want = want_old if k < n else want_new
        assert np.array_equal(dbgs[k].cpu().numpy().view(np.uint32), want[1]), f"frame {k}"
        assert_radiance(accs[k].cpu().numpy(), want[0])
    for s in (scene, old, new):
        s.close()


def test_the_volume_is_read_behind_its_stream(bm, torch_cuda, terrain):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    lo, shape = (16, 32, 64), (64, 96, 128)
    V = volume_for(np.random.default_rng(13), shape)
    final = torch.from_numpy(V).to("cuda:0")
    t = torch.zeros(shape, dtype=torch.uint8, device="cuda:0")
    busy = torch.zeros((4096, 4096), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    with torch.cuda.stream(side):
        for _ in range(40):  # queued work in front of the fill
            busy = busy @ busy
        t.copy_(final)
        filled = torch.cuda.Event()
        filled.record(side)
    pending = not filled.query()
    scene.write_region(lo, t, "replace", stream=side.cuda_stream)
    print("the fill was still pending when write_region was called:", pending)
    torch.cuda.synchronize()
    model = model_write(terrain, lo, V, "replace")
    assert np.array_equal(whole_world(scene, True), model)
    assert pending, "the queued work had finished before the call: the case shows nothing"
    scene.close()


def test_strided_tensors(bm, torch_cuda, terrain):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    rng = np.random.default_rng(14)
    big = volume_for(rng, (70, 90, 110))
    tb = torch.from_numpy(big).to("cuda:0")
    sub = tb[5:61, 7:80, 13:101]
    assert not sub.is_contiguous()
    lo = (21, 33, 90)
    scene.write_region(lo, sub, "replace")
    model = model_write(terrain, lo, big[5:61, 7:80, 13:101], "replace")
    assert_device_world(scene, model)
    # a read into a slice of a larger tensor: the bytes outside the box stay
    out = torch.full((80, 100, 144), 7, dtype=torch.uint8, device="cuda:0")
    for x0 in (16, 19):  # the aligned and the general instantiation
        out.fill_(7)
        view = out[3:73, 10:95, x0:x0 + 112]
        rlo = (16, 30, 80)  # lo.x a multiple of 16
        rhi = (rlo[0] + 112, rlo[1] + 85, rlo[2] + 70)
        assert scene.read_region(rlo, rhi, out=view) is view
        got = out.cpu().numpy()
        assert np.array_equal(got[3:73, 10:95, x0:x0 + 112], model[rlo[2]:rhi[2], rlo[1]:rhi[1], rlo[0]:rhi[0]])
        got[3:73, 10:95, x0:x0 + 112] = 7
        assert (got == 7).all(), "bytes outside the box were written"
    host = np.full((80, 100, 144), 7, np.uint8)
    scene.read_region(rlo, rhi, out=host[3:73, 10:95, 19:19 + 112])
    assert np.array_equal(host, out.cpu().numpy()), "the host read into a slice differs from the device read into the same slice"
    with pytest.raises(ValueError):
        scene.write_region(lo, tb[:, :, ::2])
    with pytest.raises(ValueError):
        scene.write_region(lo, tb.to(torch.float32))
    scene.close()


def test_writing_back_what_was_read_changes_nothing(bm, torch_cuda, terrain):
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    scene.clear_box((0, 0, 0), (60, 60, G))  # free slots
    lo, hi = (13, 22, 31), (203, 214, 225)
    words = all_device_words(scene)
    host = [scene.host_supercell(sc) for sc in range(scene.info()["supercells"])]
    for op, flip in (("replace", False), ("set", False), ("clear", True)):
        t = scene.read_region(lo, hi, device=True)
        scene.write_region(lo, 1 - t if flip else t, op)
        assert scene.last_region_ms()[2:] == (0.0, 0.0)
        assert scene.last_region_ms()[0] > 0
        assert np.array_equal(all_device_words(scene), words)
        for sc, (i, b) in enumerate(host):
            i2, b2 = scene.host_supercell(sc)
            assert np.array_equal(i, i2) and np.array_equal(b, b2)
    scene.close()


def test_refusals_leave_the_world_unchanged(bm, torch_cuda, terrain):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    L = bm._lib.load()
    words = all_device_words(scene)
    t = torch.ones((16, 16, 16), dtype=torch.uint8, device="cuda:0")
    hostv = np.ones((16, 16, 16), np.uint8)
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def region(lo, hi, row=0, sl=0):
        r = bm.bm_region()
        r.lo[:], r.hi[:] = lo, hi
        r.row_pitch, r.slice_pitch = row, sl
        return r

    ok = region((0, 0, 200), (16, 16, 216))
    dev, host = C.c_void_p(t.data_ptr()), C.c_void_p(hostv.ctypes.data)
    cases = {
        "a host pointer as BM_VOXELS_DEVICE": (ok, 0, host, bm.BM_VOXELS_DEVICE),
        "a span past its allocation": (region((0, 0, 200), (16, 16, 216), row=16, sl=1 << 24), 0, dev, bm.BM_VOXELS_DEVICE),
        "a box larger than the tensor": (region((0, 0, 0), (256, 256, 256)), 0, dev, bm.BM_VOXELS_DEVICE),
        "a bad op": (ok, 7, dev, bm.BM_VOXELS_DEVICE),
        "hi < lo": (region((0, 0, 200), (16, 15, 199)), 0, dev, bm.BM_VOXELS_DEVICE),
        "a bad where": (ok, 0, dev, 2),
        "a null volume": (ok, 0, None, bm.BM_VOXELS_DEVICE),
        "a pitch below the row": (region((0, 0, 200), (16, 16, 216), row=8), 0, dev, bm.BM_VOXELS_DEVICE),
    }
    if torch.cuda.device_count() > 1:
        other = torch.ones((16, 16, 16), dtype=torch.uint8, device="cuda:1")
        cases["a tensor on another device"] = (ok, 0, C.c_void_p(other.data_ptr()), bm.BM_VOXELS_DEVICE)
        with pytest.raises(ValueError):
            scene.write_region((0, 0, 200), other)
    for name, (r, op, ptr, where) in cases.items():
        assert L.bm_scene_write_region(scene.gpuScene, C.byref(r), op, ptr, where, stream) == EINVAL, name
        if name != "a bad op":
            assert L.bm_scene_read_region(scene.gpuScene, C.byref(r), ptr, where, stream) == EINVAL, name
    assert L.bm_scene_write_region(scene.gpuScene, None, 0, dev, bm.BM_VOXELS_DEVICE, stream) == EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(all_device_words(scene), words) and not scene.info()["failed"]
    assert np.array_equal(scene.voxels().view(np.uint8), terrain)
    assert (t == 1).all() and (hostv == 1).all()
    # a scene that is not on the device
    fresh = bm.Scene(G, G, device=0)
    assert L.bm_scene_write_region(fresh.gpuScene, C.byref(ok), 0, dev, bm.BM_VOXELS_DEVICE, stream) == 10002
    fresh.close()
    # and the valid call goes through
    assert L.bm_scene_write_region(scene.gpuScene, C.byref(ok), 0, dev, bm.BM_VOXELS_DEVICE, stream) == 0
    assert scene.read_region((0, 0, 200), (16, 16, 216)).all()
    scene.close()
