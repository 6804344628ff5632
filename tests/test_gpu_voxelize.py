"""Scene.voxelize and Scene.write_mesh on the MI355X (csrc/voxelize.hip): device bytes and the result record must equal bm_host_voxelize --
the host routine that tests/test_voxelize_host.py pins to the numpy model and to exact clipping -- byte for byte.  Shapes: row lengths on
both sides of a word edge (31, 32, 33) and a volume with no extent a multiple of 8; an unaligned base with pitches larger than the extents;
one triangle of 200 voxels, an icosphere, 70 000 sub-voxel triangles (the offset scan crosses workgroups), nothing but rejected triangles
and no triangle at all.  Every number is an integer, every comparison exact."""
import ctypes as C
import time

import numpy as np
import pytest

import _voxelize_model as model

pytestmark = pytest.mark.gpu
EINVAL = 10001
MODES = ("surface", "solid", "solid+surface")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def scene(bm, torch_cuda):
    """a small preloaded scene: a floor of 8 voxels, a random block in one corner, the rest empty"""
    vox = np.zeros((128, 128, 128), np.uint8)
    vox[:8] = 1
    vox[8:40, :40, :40] = np.random.default_rng(5).random((32, 40, 40)) < 0.2
    s = bm.Scene.from_voxels(vox)
    s.world = vox
    yield s
    s.close()


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_voxelize.py took {time.time() - t0:.1f} s")


def dev(torch, tri):
    return torch.from_numpy(np.ascontiguousarray(tri, np.float32).reshape(-1, 3, 3)).cuda()


def check(bm, torch, scene, tri, lo, shape, mode, what=""):
    want, rec = bm.host_voxelize(tri, lo, shape, mode=mode)
    got, res = scene.voxelize(dev(torch, tri), lo, shape, mode=mode)
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == tuple(shape)
    assert np.array_equal(got, want), f"{what} {mode} {shape}: {np.count_nonzero(got != want)} bytes differ"
    assert res.record == rec, f"{what} {mode}: {res.record} on the device, {rec} on the host"
    return want, rec


SPHERE = model.icosphere((16.3, 11.9, 8.2), 7.6, 3)   # 1 280 triangles


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(17, 24, 31), (17, 24, 32), (17, 24, 33), (17, 24, 40)])
def test_icosphere_at_word_edges(shape, mode, bm, torch_cuda, scene):
    """nx = 31, 32, 33 and 40 x 24 x 17: the sphere sticks out of the shorter rows, so crossings land on bit nx"""
    assert len(SPHERE) == 1280
    want, rec = check(bm, torch_cuda, scene, SPHERE, (0, 0, 0), shape, mode, "icosphere")
    assert want.any() and rec["open_columns"] == 0 and rec["rejected"] == 0


@pytest.mark.parametrize("mode", MODES)
def test_one_triangle_spanning_200_voxels(mode, bm, torch_cuda, scene):
    tri = np.array([[[-20.25, 3.5, 1.0], [180.5, 10.25, 30.75], [40.0, 44.5, 5.5]]], np.float32)
    want, rec = check(bm, torch_cuda, scene, tri, (-10, 0, 0), (33, 47, 170), mode, "large triangle")
    if mode != "solid":
        assert want.sum() > 1000
    if mode != "surface":
        assert rec["open_columns"] > 300


def test_sub_voxel_triangles_across_plan_workgroups(bm, torch_cuda, scene):
    """70 000 triangles of less than a voxel: 274 plan workgroups, so the scan of their sums runs more than one word per thread"""
    rng = np.random.default_rng(11)
    base = rng.uniform(-1, 41, size=(70_000, 1, 3))
    tri = (base + rng.uniform(-0.4, 0.4, size=(70_000, 3, 3))).astype(np.float32)
    want, rec = check(bm, torch_cuda, scene, tri, (0, 0, 0), (40, 40, 40), "solid+surface", "sub-voxel")
    assert want.sum() > 30_000 and rec["open_columns"] > 0


def test_rejected_degenerate_and_no_triangles(bm, torch_cuda, scene):
    bad = np.array([[[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [np.inf, 0, 0], [0, 1, 0]], [[5e6, 0, 0], [1, 0, 0], [0, 1, 0]],
                    [[0, 0, 0], [3000, 0, 0], [0, 1, 0]], [[20000, 0, 0], [20001, 0, 0], [20000, 1, 0]]], np.float32)
    want, rec = check(bm, torch_cuda, scene, bad, (0, 0, 0), (9, 10, 11), "solid+surface", "rejected")
    assert rec["rejected"] == 5 and not want.any()
    flat = np.array([[[1, 1, 1], [2, 2, 2], [3, 3, 3]], [[1, 1, 1], [1, 1, 1], [4, 5, 6]]], np.float32)
    want, rec = check(bm, torch_cuda, scene, np.concatenate((bad[:2], flat, model.box_mesh((2, 2, 2), (6, 7, 8)))), (0, 0, 0), (9, 10, 11), "solid+surface", "mixed")
    assert rec["rejected"] == 2 and rec["degenerate"] == 2 and want.sum() == 6 * 7 * 8
    want, rec = check(bm, torch_cuda, scene, np.zeros((0, 3, 3), np.float32), (0, 0, 0), (9, 10, 11), "solid", "empty")
    assert not want.any() and tuple(rec.tolist()) == (0, 0, 0)


@pytest.mark.parametrize("keep", [False, True])
def test_unaligned_base_pitches_and_keep(keep, bm, torch_cuda, scene):
    """the volume is a slice of a larger tensor that starts at an odd byte: the bytes around it stay, and KEEP leaves non-zero bytes as they are"""
    torch = torch_cuda
    rng = np.random.default_rng(3)
    big = np.where(rng.random((20, 30, 64)) < 0.1, rng.integers(1, 256, size=(20, 30, 64)), 0).astype(np.uint8)
    tri = model.torus((20.5, 12.0, 8.5), 8.0, 3.0)
    lo = (-2, 1, 0)
    for x0, nx in ((3, 37), (1, 16), (5, 47)):
        host = big.copy()
        bm.host_voxelize(tri, lo, out=host[2:19, 3:28, x0:x0 + nx], keep=keep)
        d_big = torch.from_numpy(big).cuda()
        out, res = scene.voxelize(dev(torch, tri), lo, out=d_big[2:19, 3:28, x0:x0 + nx], keep=keep)
        assert out.data_ptr() % 16 != 0 and np.array_equal(d_big.cpu().numpy(), host), (x0, nx, keep)
        assert res.open_columns == 0
        inner = host[2:19, 3:28, x0:x0 + nx]
        if keep:
            assert (inner[big[2:19, 3:28, x0:x0 + nx] > 1] > 1).any()
        else:
            assert inner.max() == 1


def test_triangles_made_on_the_stream_just_before(bm, torch_cuda, scene):
    torch = torch_cuda
    base = dev(torch, SPHERE)
    want, rec = bm.host_voxelize(SPHERE + np.float32(2.0), (0, 0, 0), (24, 28, 36))
    tri = base + 2.0   # a torch kernel on the current stream; the call is queued behind it
    got, res = scene.voxelize(tri, (0, 0, 0), (24, 28, 36))
    assert np.array_equal(got.cpu().numpy(), want) and res.record == rec
    verts = torch.from_numpy(SPHERE.reshape(-1, 3)).cuda()
    faces = torch.arange(len(verts), device="cuda").reshape(-1, 3)
    got, res = scene.voxelize((verts + 2.0, faces), (0, 0, 0), (24, 28, 36))
    assert np.array_equal(got.cpu().numpy(), want) and res.record == rec


def test_two_calls_on_two_streams(bm, torch_cuda, scene):
    torch = torch_cuda
    a, b = model.icosphere((20, 20, 20), 15.5, 3), model.torus((20, 20, 12), 12, 5, 40, 20)
    want_a, rec_a = bm.host_voxelize(a, (0, 0, 0), (40, 40, 40))
    want_b, rec_b = bm.host_voxelize(b, (0, 0, 0), (24, 40, 40))
    da, db = dev(torch, a), dev(torch, b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):
        outs.append((scene.voxelize(da, (0, 0, 0), (40, 40, 40), stream=s1.cuda_stream), scene.voxelize(db, (0, 0, 0), (24, 40, 40), stream=s2.cuda_stream)))
    torch.cuda.synchronize()
    for (ga, ra), (gb, rb) in outs:
        assert np.array_equal(ga.cpu().numpy(), want_a) and ra.record == rec_a
        assert np.array_equal(gb.cpu().numpy(), want_b) and rb.record == rec_b


def test_refusals_leave_the_volume_untouched(bm, torch_cuda, scene):
    torch = torch_cuda
    L = scene._L
    tri = dev(torch, model.box_mesh((1, 1, 1), (5, 5, 5)))
    n = int(tri.shape[0])
    vol = torch.full((8, 8, 8), 7, dtype=torch.uint8, device="cuda")
    need = bm.voxelize_workspace_bytes((8, 8, 8), n)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    res = torch.zeros(2, dtype=torch.int64, device="cuda")
    from brickmap_amd import _lib

    def call(extent=(8, 8, 8), row=0, sl=0, mode=3, flags=0, count=n, t=tri.data_ptr(), v=vol.data_ptr(), r=res.data_ptr(), w=ws.data_ptr(), wb=need):
        par = _lib.bm_voxelize_params()
        par.extent[:] = list(extent)
        par.row_pitch, par.slice_pitch, par.mode, par.flags = row, sl, mode, flags
        return L.bm_voxelize(scene.gpuScene, C.byref(par), count, C.c_void_p(t), C.c_void_p(v), C.c_void_p(r), C.c_void_p(w), wb, None)

    def refused(kw, fragment):
        """BM_EINVAL, and the refusal that fired: the message names the entry point and holds the fragment of its class"""
        assert call(**kw) == EINVAL, kw
        msg = L.bm_last_error_string()
        assert msg.startswith(b"bm_voxelize: ") and fragment in msg, (kw, msg)

    extent, null, aligned, overlaps = b"an extent below 1 or above 16384", b"null", b"aligned", b"overlaps"
    bad = [(dict(extent=(0, 8, 8)), extent), (dict(extent=(8, 8, 16385)), extent), (dict(row=7), b"row_pitch below the extent along x"),
           (dict(sl=63), b"slice_pitch below row_pitch * the extent along y"), (dict(mode=0), b"unknown mode"), (dict(mode=4), b"unknown mode"),
           (dict(flags=2), b"unknown flag"), (dict(count=-1), b"a triangle count below 0 or above 2^30"),
           (dict(t=0), null), (dict(v=0), null), (dict(w=0), null), (dict(t=tri.data_ptr() + 2), aligned), (dict(r=res.data_ptr() + 4), aligned),
           (dict(w=ws.data_ptr() + 8), aligned), (dict(wb=need - 1), b"smaller than"),
           (dict(w=vol.data_ptr(), wb=need), overlaps), (dict(v=ws.data_ptr() + 16), overlaps), (dict(t=ws.data_ptr()), overlaps)]
    for kw, fragment in bad:
        refused(kw, fragment)
    # a volume whose pitches carry it 56 MiB past an allocation of 512 bytes (one of its own: torch's tensors share theirs)
    own = C.c_void_p()
    assert L.bm_buffer_alloc(scene.device, 512, C.byref(own)) == 0
    refused(dict(row=1 << 20, sl=8 << 20, v=own.value), b"does not lie inside")
    torch.cuda.synchronize()
    assert (vol == 7).all().item() and not res.any().item() and not ws.any().item()
    assert call(v=own.value) == 0
    assert L.bm_synchronize(scene.gpuScene) == 0 and L.bm_buffer_free(scene.device, own) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(vol.cpu().numpy(), bm.host_voxelize(tri.cpu().numpy(), (0, 0, 0), (8, 8, 8))[0])


# ---------------------------------------------------------------- write_mesh into the live scene
def test_write_mesh_of_a_floating_sphere(bm, torch_cuda, scene):
    torch = torch_cuda
    tri = model.icosphere((80.3, 79.8, 70.4), 18.7, 3)
    lo, hi, res = scene.write_mesh(dev(torch, tri))
    assert res.open_columns == 0 and res.rejected == 0
    shape = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
    want, _ = model.model_voxelize(tri, lo, shape)
    before = scene.world[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    assert np.array_equal(scene.read_region(lo, hi), (want | before).astype(bool))
    # one piece, of the model's size, in an empty box around it
    comps = scene.components((50, 50, 40), (112, 112, 104))
    assert len(comps) == 1 and int(comps.records["voxels"][0]) == int(want.sum())
    # a ray from outside along +x through the centre row hits the model's first voxel
    y, z = 80, 70
    first = lo[0] + int(np.argmax(want[z - lo[2], y - lo[1]]))
    hits = scene.cast_rays(np.array([[45.5, y + 0.5, z + 0.5]], np.float32), np.array([[1.0, 0.0, 0.0]], np.float32))
    assert tuple(int(v) for v in np.asarray(hits.voxel)[0]) == (first, y, z)
    scene.write_region(lo, torch.from_numpy(want).cuda(), op="clear")
    assert np.array_equal(scene.read_region(lo, hi), before.astype(bool))


def test_write_mesh_half_outside_the_world(bm, torch_cuda, scene):
    torch = torch_cuda
    tri = model.icosphere((126.2, 64.1, 120.3), 14.2, 3)
    lo, hi, res = scene.write_mesh(dev(torch, tri))
    assert hi[0] == 128 and hi[2] == 128 and res.rejected == 0
    assert res.open_columns == 0, "crossings beyond the last voxel of a row count at nx: a closed mesh stays closed when the volume cuts it"
    shape = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
    want, rec = model.model_voxelize(tri, lo, shape)
    assert res.record == rec
    before = scene.world[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    assert np.array_equal(scene.read_region(lo, hi), (want | before).astype(bool))
    hits = scene.cast_rays(np.array([[100.5, 64.5, 120.5]], np.float32), np.array([[1.0, 0.0, 0.0]], np.float32))
    assert tuple(int(v) for v in np.asarray(hits.voxel)[0]) == (lo[0] + int(np.argmax(want[120 - lo[2], 64 - lo[1]])), 64, 120)
    scene.write_region(lo, torch.from_numpy(want).cuda(), op="clear")
    assert scene.write_mesh(dev(torch, tri + np.float32(500.0))) == (None, None, None)


# ---------------------------------------------------------------- the example
def test_headless_main_adds_a_mesh_file(bm, torch_cuda, tmp_path):
    """examples/headless_main --mesh FILE@x,y,z: a raw triangle file, moved, voxelized and written before the frame (C++ Scene::write_mesh)"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "headless_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    world = tmp_path / "empty.raw"
    np.zeros((128, 128, 128), np.uint8).tofile(world)
    mesh = tmp_path / "box.tri"
    model.box_mesh((0, 0, 0), (20, 10, 30)).tofile(mesh)
    out = tmp_path / "frame.ppm"
    r = subprocess.run([exe, "--voxels", str(world), "--mesh", f"{mesh}@40,50,60", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"mesh: 12 triangles \(0 rejected, 0 degenerate\) into a box of (\d+) voxels, open columns 0", r.stdout)
    assert m and int(m.group(1)) == 22 * 12 * 32, r.stdout
    (tmp_path / "short.tri").write_bytes(b"\x00" * 35)
    r = subprocess.run([exe, "--voxels", str(world), "--mesh", f"{tmp_path / 'short.tri'}@0,0,0", "128", "128", "64", "48", "1", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "does not hold" in r.stderr
