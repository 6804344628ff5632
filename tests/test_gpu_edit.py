"""Voxel edits of a live scene on the MI355X (bm_scene_edit): the GPU cube-field update is exact, edited worlds render like the oracle's
world edited the same way, edits are ordered between frames, and streaming survives requests that an edit made stale.

The oracle's world cannot gain bricks, so it is edited in place through its host arrays (orc_world_sc_indices / orc_world_sc_bricks):
voxels cleared, LoD masks recomputed, emptied cells' words set to 0.  The product takes the longer way -- clear a region R, then set
back a subset S of R's original voxels: new slots, the field shrinking and growing again -- and must end in the same world."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-4
G = 256
CAM = dict(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5)
# R: crosses the supercell borders at x = 128 and y = 128 and takes in what the camera sees of the terrain
R_LO, R_HI = np.array([100, 70, 60]), np.array([190, 160, 200])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def assert_radiance(got, want):
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-6)
    assert float(err.max()) <= RTOL, f"max relative radiance error {err.max():.3e}"


def render(bm, torch, scene, cam, W=96, H=64, mb=3, primary=False):
    """ordered frame with hit records and counters: (radiance, hit records, counters)"""
    flags = bm.BM_FLAG_ORDERED | bm.BM_FLAG_COUNTERS | (bm.BM_FLAG_PRIMARY_ONLY if primary else 0)
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    dbg = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda:0")
    scene.counters_reset()
    scene.render(cam, bm.FrameParams(W, H, spp=1, max_bounces=mb, flags=flags), acc, debug=dbg)
    torch.cuda.synchronize()
    return acc.cpu().numpy(), dbg.cpu().numpy().view(np.uint32), scene.counters()


def orender(orc, world, cam, W=96, H=64, mb=3, primary=False):
    oacc, odbg, ocnt, _ = world.render(orc.make_camera(cam.position, cam.direction), orc.make_frame(W, H, spp=1, max_bounces=mb, primary_only=1 if primary else 0))
    return oacc, odbg, ocnt


def assert_same(got, want, counters=True):
    acc, dbg, cnt = got
    oacc, odbg, ocnt = want
    assert np.array_equal(dbg, odbg), f"{np.count_nonzero((dbg != odbg).any(-1))} pixels whose hit records differ"
    assert_radiance(acc, oacc)
    if counters:
        assert cnt == ocnt


def world_voxels(bm, scene):
    """the scene's host world as a bool volume [z, y, x]"""
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


def oracle_clear(world, remove):
    """clear the voxels `remove` ([z, y, x] bool) in the oracle's host world, in place; then the caller resets its device view"""
    sg = world.grid_size // 128
    L = world.L
    for sc in range(world.nsc):
        sx, sy, sz = sc % sg, (sc // sg) % sg, sc // (sg * sg)
        sub = remove[sz * 128:sz * 128 + 128, sy * 128:sy * 128 + 128, sx * 128:sx * 128 + 128]
        if not sub.any():
            continue
        idx = np.ctypeslib.as_array(C.cast(L.orc_world_sc_indices(world.h, sc), C.POINTER(C.c_uint32)), shape=(4096,))
        n = world.sc_nbricks(sc)
        bricks = np.ctypeslib.as_array(C.cast(L.orc_world_sc_bricks(world.h, sc), C.POINTER(C.c_uint32)), shape=(n, 16))
        for cell in np.nonzero(idx)[0]:
            bx, by, bz = cell & 15, (cell >> 4) & 15, cell >> 8
            m = sub[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]
            if not m.any():
                continue
            slot = idx[cell] & 0xFFF
            bricks[slot] &= ~np.packbits(m.reshape(-1), bitorder="little").view(np.uint32)
            bits = np.unpackbits(bricks[slot].view(np.uint8), bitorder="little").reshape(2, 4, 2, 4, 2, 4).astype(bool)
            if not bits.any():
                idx[cell] = 0
                continue
            q = bits.any(axis=(1, 3, 5)).reshape(-1)  # [qz, qy, qx] -> bit 4 qz + 2 qy + qx (Scene.cpp:95)
            lod = int((q.astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum())
            idx[cell] = np.uint32(slot | 0x80000000 | (lod << 12))


def remove_then_restore(bm, scene, orig):
    """product: clear R, then set back S = the original voxels of R with (x + y + z) % 3 == 0; returns R \\ S as a volume"""
    scene.clear_box(R_LO, R_HI)
    z, y, x = np.nonzero(orig[R_LO[2]:R_HI[2], R_LO[1]:R_HI[1], R_LO[0]:R_HI[0]])
    x, y, z = x + R_LO[0], y + R_LO[1], z + R_LO[2]
    keep = (x + y + z) % 3 == 0
    scene.set_voxels(np.stack([x[keep], y[keep], z[keep]], 1).astype(np.int32), 1)
    removed = np.zeros_like(orig)
    removed[z[~keep], y[~keep], x[~keep]] = True
    return removed


@pytest.fixture(scope="module")
def pristine(bm, orc, torch_cuda):
    """original voxels of the 256^3 world and the oracle's renders of it"""
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    vox = world_voxels(bm, scene)
    cam = bm.Camera(**CAM).update()
    field = scene.device_cube_field()
    scene.close()
    w = orc.World(G, G)
    w.reset_device(True)
    return dict(vox=vox, field=field, cam=cam, full=orender(orc, w, cam), primary=orender(orc, w, cam, primary=True))


def test_device_field_is_exact_after_every_batch(bm, torch_cuda):
    torch = torch_cuda
    for dims in ((256, 256), (1024, 256)):
        scene = bm.Scene(*dims, device=0).generate().preload_all()
        if dims == (256, 256):  # an unedited world: the field equals bm_host_cube_field
            assert np.array_equal(scene.device_cube_field(), bm.host_cube_field(*dims))
        gs, gh = dims
        batches = [
            [bm.edit_box("set", (40, 40, gh - 60), (70, 52, gh - 20))],                       # a block in the sky
            [bm.edit_sphere("clear", (gs // 2, gs // 2, gh // 2), 30)],                         # a carve into the terrain
            [bm.edit_box("clear", (120, 120, 0), (140, 136, gh)), bm.edit_box("set", (0, 0, gh - 8), (9, gs, gh))],  # supercell borders, world border
            [bm.edit_sphere("set", (gs - 3, 5, gh - 4), 12)],                                  # clipped by the world
            [bm.edit_box("set", (200, 16, gh - 40), (208, 24, gh - 32))],                     # a cell fills ...
            [bm.edit_box("clear", (200, 16, gh - 40), (208, 24, gh - 32))],                   # ... and empties again
            [bm.edit_box("set", (3, 3, 3), (4, 4, 4)), bm.edit_box("clear", (3, 3, 3), (4, 4, 4))],  # set + clear in one batch
        ]
        for k, batch in enumerate(batches):
            scene.edit(batch)
            dev, host = scene.device_cube_field(), scene.host_cube_field()
            assert np.array_equal(dev, host), f"{dims} batch {k}: {np.count_nonzero(dev != host)} field bytes differ"
        info = scene.info()
        assert info["resident_bricks"] == info["total_bricks"] and not info["failed"]
        torch.cuda.synchronize()
        scene.close()


@pytest.mark.parametrize("primary", [True, False], ids=["primary", "paths4"])
def test_preloaded_edit_matches_the_oracle(primary, bm, orc, torch_cuda, pristine):
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    before = scene.info()["total_bricks"]
    removed = remove_then_restore(bm, scene, pristine["vox"])
    assert np.array_equal(scene.device_cube_field(), scene.host_cube_field())
    w = orc.World(G, G)
    oracle_clear(w, removed)
    w.reset_device(True)
    cam = pristine["cam"]
    got, want = render(bm, torch_cuda, scene, cam, primary=primary), orender(orc, w, cam, primary=primary)
    assert_same(got, want)
    assert not np.array_equal(want[1], pristine["primary" if primary else "full"][1]), "the edit is not visible"
    info = scene.info()
    assert info["total_bricks"] == w.total_bricks() or info["total_bricks"] <= before
    assert info["resident_bricks"] == info["total_bricks"]
    scene.close()


@pytest.mark.parametrize("overlapped", [0, 1])
def test_streaming_edit_matches_the_oracle(overlapped, bm, orc, torch_cuda, pristine):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0)
    scene.set_queue_capacity(1 << 16)
    scene.generate().preload_all()
    removed = remove_then_restore(bm, scene, pristine["vox"])  # made while preloaded, then back to the reference's initial residency
    scene.reset_residency().set_streaming_mode(overlapped)
    w = orc.World(G, G)
    w.set_queue_cap(1 << 16)
    oracle_clear(w, removed)
    w.reset_device(False)
    cam = pristine["cam"]
    # first frame: nothing resident, every brick requested the same way
    assert_same(render(bm, torch, scene, cam), orender(orc, w, cam))
    for _ in range(64):
        render(bm, torch, scene, cam)
        if scene.process_load_queue() == 0 and scene.process_load_queue() == 0:
            break
    else:
        pytest.fail("streaming did not reach a steady state")
    w.reset_device(True)
    assert_same(render(bm, torch, scene, cam), orender(orc, w, cam), counters=False)
    assert not scene.info()["failed"]
    scene.close()


@pytest.mark.parametrize("overlapped", [0, 1])
def test_edit_that_empties_requested_bricks_is_not_a_failure(overlapped, bm, orc, torch_cuda, pristine):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0)
    scene.set_queue_capacity(1 << 16)
    scene.generate().set_streaming_mode(overlapped)
    cam = pristine["cam"]
    render(bm, torch, scene, cam)  # requests every brick it sees
    if overlapped:
        scene.process_load_queue()  # the ring is copied out now; the edit lands between copy-out and servicing
    scene.clear_box(R_LO, R_HI)     # empties bricks that stand in the ring
    scene.process_load_queue()
    assert not scene.info()["failed"]
    for _ in range(64):
        render(bm, torch, scene, cam)
        if scene.process_load_queue() == 0 and scene.process_load_queue() == 0:
            break
    else:
        pytest.fail("streaming did not reach a steady state")
    info = scene.info()
    assert not info["failed"] and info["resident_bricks"] <= info["total_bricks"]
    w = orc.World(G, G)
    removed = np.zeros_like(pristine["vox"])
    removed[R_LO[2]:R_HI[2], R_LO[1]:R_HI[1], R_LO[0]:R_HI[0]] = True
    oracle_clear(w, removed)
    w.reset_device(True)
    assert_same(render(bm, torch, scene, cam), orender(orc, w, cam), counters=False)
    scene.close()


def test_round_trip_restores_the_pristine_scene(bm, orc, torch_cuda, pristine):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    cam = pristine["cam"]
    base = render(bm, torch, scene, cam)
    vox = pristine["vox"]
    c, r = np.array([180, 120, 120]), 28
    z, y, x = np.nonzero(vox[c[2] - r:c[2] + r + 1, c[1] - r:c[1] + r + 1, c[0] - r:c[0] + r + 1])
    inside = (x - r) ** 2 + (y - r) ** 2 + (z - r) ** 2 <= r * r
    solid = np.stack([x[inside], y[inside], z[inside]], 1).astype(np.int32) + (c - r).astype(np.int32)
    sky_lo, sky_hi = (60, 150, 230), (90, 170, 250)
    assert not vox[sky_lo[2]:sky_hi[2], sky_lo[1]:sky_hi[1], sky_lo[0]:sky_hi[0]].any()
    scene.edit([bm.edit_sphere("clear", c, r), bm.edit_box("set", sky_lo, sky_hi)])
    assert not np.array_equal(scene.device_cube_field(), pristine["field"])
    scene.clear_box(sky_lo, sky_hi)
    scene.set_voxels(solid, np.ones(len(solid), np.uint8))
    assert np.array_equal(scene.device_cube_field(), pristine["field"])
    acc, dbg, cnt = render(bm, torch, scene, cam)
    assert np.array_equal(dbg, base[1]) and cnt == base[2]
    assert_radiance(acc, base[0])
    scene.close()


def test_new_geometry_in_the_sky_is_hit(bm, torch_cuda):
    """a wall of voxels 4 voxels in front of a camera in the sky, looking along +y: every primary ray hits its face y = y0 at distance
    (y0 - y_cam) / dir_y, with the same normal.  With only words and bricks updated, the stale field would let the walk jump the wall."""
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    cam = bm.Camera(position=(128.5, 20.5, 230.5), horizontal_angle=0.0, vertical_angle=0.0).update()  # direction (0, 1, 0)
    W = H = 32
    _, before, _ = render(bm, torch, scene, cam, W, H, primary=True)
    y0 = 25
    scene.fill_box((0, y0, 200), (G, y0 + 8, G))
    _, dbg, _ = render(bm, torch, scene, cam, W, H, primary=True)
    hit = (dbg[..., 1] >> 8) & 1
    assert hit.all(), f"{np.count_nonzero(hit == 0)} rays missed the wall"
    assert len(np.unique(dbg[..., 1])) == 1, "the wall's face has one normal and one level"
    dist = dbg[..., 0].view(np.float32)
    d0 = y0 - cam.position[1]
    # the ray to pixel (i, j) leaves along dir + u right + v up; its hit distance is d0 / dir_y >= d0, at most d0 / cos(half the diagonal field)
    assert (dist >= d0 - 1e-3).all() and (dist <= d0 * 4).all(), f"hit distances {dist.min()} ... {dist.max()}, wall at {d0}"
    assert abs(float(dist[H // 2, W // 2]) - d0) < 0.25, f"centre ray: {dist[H // 2, W // 2]}"
    assert np.count_nonzero((before != dbg).any(-1)) > 0.9 * W * H
    scene.close()


def test_edit_is_ordered_between_frame_launches(bm, orc, torch_cuda, pristine):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    cam = pristine["cam"]
    W, H, n = 96, 64, 3
    p = [bm.FrameParams(W, H, spp=1, max_bounces=3, flags=bm.BM_FLAG_ORDERED) for _ in range(n)]
    accs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2 * n)]
    dbgs = [torch.zeros((H, W, 8), dtype=torch.int32, device="cuda:0") for _ in range(2 * n)]
    scene.render_frames(cam, p, accs[:n], debugs=dbgs[:n])
    scene.clear_box(R_LO, R_HI)  # no synchronisation in between
    scene.render_frames(cam, p, accs[n:], debugs=dbgs[n:])
    torch.cuda.synchronize()
    w = orc.World(G, G)
    removed = np.zeros_like(pristine["vox"])
    removed[R_LO[2]:R_HI[2], R_LO[1]:R_HI[1], R_LO[0]:R_HI[0]] = True
    oracle_clear(w, removed)
    w.reset_device(True)
    edited = orender(orc, w, cam)
    for k in range(2 * n):
        want = pristine["full"] if k < n else edited
        assert np.array_equal(dbgs[k].cpu().numpy().view(np.uint32), want[1]), f"frame {k}"
        assert_radiance(accs[k].cpu().numpy(), want[0])
    scene.close()


def test_wavefront_frames_see_edits(bm, orc, torch_cuda, pristine):
    torch = torch_cuda
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    wf = bm.Wavefront(scene, 1 << 16)
    scene.clear_box(R_LO, R_HI)
    w = orc.World(G, G)
    removed = np.zeros_like(pristine["vox"])
    removed[R_LO[2]:R_HI[2], R_LO[1]:R_HI[1], R_LO[0]:R_HI[0]] = True
    oracle_clear(w, removed)
    w.reset_device(True)
    owf = orc.Wavefront(queue_size=1 << 16, max_bounces=3)
    W, H = 96, 64
    cam = pristine["cam"]
    ocam = orc.make_camera(cam.position, cam.direction)
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    oacc = np.zeros((H, W, 4), np.float32)
    for _ in range(4):
        wf.frame(cam, bm.FrameParams(W, H, max_bounces=3), acc)
        ost = owf.frame(w, ocam, W, H, oacc)
        st = wf.stats()
        assert st == ost
        n = st["survivors"]
        assert n > 0
        got, want = wf.read_queue("work", 0, n).view(np.uint8), owf.read_queue(0, 0, n)
        assert np.array_equal(got, want), "extend results of the wavefront frame differ from the edited oracle's"
    assert_radiance(acc.cpu().numpy(), oacc)
    wf.close()
    scene.close()


def test_bad_edit_leaves_the_scene_unchanged(bm, torch_cuda):
    from brickmap_amd import _lib
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    field = scene.device_cube_field()
    idx = scene.host_supercell(5)
    bad = _lib.bm_edit()
    bad.op, bad.shape, bad.radius = 1, 2, -3
    with pytest.raises(bm.BrickmapError):
        scene.edit([bm.edit_box("clear", (0, 0, 0), (G, G, G)), bad])
    assert np.array_equal(scene.device_cube_field(), field) and np.array_equal(scene.host_supercell(5)[0], idx[0])
    scene.close()
