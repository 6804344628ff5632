"""Who waits for whom in a scene, on the MI355X (csrc/frame_order.h, csrc/launch_book.h, Turn and StageMarks of csrc/hip_owned.h): the stage
clocks of edits, region writes and loads -- what each reports, and when it reports nothing --, more frame streams than the stream table
holds with edits between the frames, a query ring that wraps, and a scratch or staging buffer that has to grow while the call before still uses it.
Every result is compared with the same calls made one by one, each waited for.  Nothing here depends on how the library decides the
ordering, only on what it computes: the file passes on a library built before the ordering had one owner as well.

The world is 128 x 128 x 128 voxels, the smallest a scene takes: a floor two cells thick, two towers on it and three pieces in the air."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 128
W = H = 64
AIR = ((40, 40, 96), (48, 48, 104))  # one empty cell, away from everything


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def volume():
    vox = np.zeros((G, G, G), np.uint8)  # [z, y, x]
    vox[:16] = 1
    vox[16:40, 72:88, 24:40] = 1
    vox[16:56, 80:96, 88:104] = 1
    vox[64:72, 60:68, 60:68] = 1
    vox[80:83, 30:41, 90:101] = 1
    vox[100:108, 100:108, 20:28] = 1
    return vox  # (shared: nobody changes it)


def state_error(bm, call):
    with pytest.raises(bm.BrickmapError, match="brickmap error 10002"):  # BM_ESTATE
        call()


def test_edit_clock(bm, volume):
    s = bm.Scene.from_voxels(volume)
    state_error(bm, s.last_edit_ms)
    s.clear_box(*AIR)                                # clears empty space: nothing is scattered
    s.clear_box((1000, 1000, 1000), (1008, 1008, 1008))  # outside the world
    state_error(bm, s.last_edit_ms)
    s.set_voxels([(5, 5, 5)], 0)                     # a voxel out of a full brick of the floor: bits only
    scatter, field = s.last_edit_ms()
    print(f"bits-only edit: scatter {scatter:.4f} ms, field {field:.4f} ms")
    assert scatter > 0 and field == 0.0
    s.fill_box(*AIR)                                 # a new brick: the cell's occupancy changes
    real = s.last_edit_ms()
    print(f"new brick: scatter {real[0]:.4f} ms, field {real[1]:.4f} ms")
    assert real[0] > 0 and real[1] > 0
    s.clear_box((8, 8, 112), (16, 16, 120))          # empty space again
    s.clear_box((1000, 1000, 1000), (1008, 1008, 1008))
    assert s.last_edit_ms() == real, "an edit that scatters nothing leaves the times of the last one that did"
    s.set_voxels([(6, 5, 5)], 0)
    scatter, field = s.last_edit_ms()
    assert scatter > 0 and field == 0.0 and (scatter, field) != real
    edited = volume.copy()
    edited[96:104, 40:48, 40:48] = 1
    edited[5, 5, 5:7] = 0
    assert np.array_equal(s.voxels(), edited.astype(bool))
    s.close()


def test_region_clock(bm, torch_cuda, volume):
    torch = torch_cuda
    s = bm.Scene.from_voxels(volume)
    state_error(bm, s.last_region_ms)
    brick = np.ones((8, 8, 8), np.uint8)
    s.write_region(AIR[0], brick)                    # host volume, a new brick
    pack, copy, scatter, field = s.last_region_ms()
    print(f"host write, new brick: {pack} {copy} {scatter:.4f} {field:.4f} ms")
    assert (pack, copy) == (0.0, 0.0) and scatter > 0 and field > 0
    brick[3, 3, 3] = 0
    s.write_region(AIR[0], brick)                    # host volume, bits only
    pack, copy, scatter, field = s.last_region_ms()
    assert (pack, copy) == (0.0, 0.0) and scatter > 0 and field == 0.0
    dev = torch.zeros((8, 8, 8), dtype=torch.uint8, device="cuda:0")
    s.write_region(AIR[0], dev)                      # device volume, the brick goes
    pack, copy, scatter, field = s.last_region_ms()
    print(f"device write, brick removed: {pack:.4f} {copy:.4f} {scatter:.4f} {field:.4f} ms")
    assert pack > 0 and copy > 0 and scatter > 0 and field > 0
    dev[2, 2, 2] = 1
    dev[5, 5, 5] = 1
    s.write_region(AIR[0], dev)                      # device volume, a new brick of two voxels
    assert min(s.last_region_ms()) > 0
    dev[2, 2, 2] = 0
    s.write_region(AIR[0], dev)                      # device volume, bits only
    pack, copy, scatter, field = s.last_region_ms()
    assert pack > 0 and copy > 0 and scatter > 0 and field == 0.0
    s.write_region(AIR[0], np.zeros((8, 8, 8), np.uint8))  # a host write after device writes: no pack, no copy
    pack, copy, scatter, field = s.last_region_ms()
    assert (pack, copy) == (0.0, 0.0) and scatter > 0 and field > 0
    assert np.array_equal(s.voxels(), volume.astype(bool))
    s.close()


def test_load_clock(bm, torch_cuda, volume):
    torch = torch_cuda
    s = bm.Scene(G, G)
    state_error(bm, s.last_load_ms)
    s.load_voxels(volume)
    state_error(bm, s.last_load_ms)                  # device time exists for loads from device memory only
    s.load_voxels(torch.from_numpy(volume).to("cuda:0"))
    times = s.last_load_ms()
    print("device load: pack %.4f, field %.4f, mirror %.4f ms" % times)
    assert min(times) > 0
    assert s.last_load_ms() == times
    s.load_voxels(volume)                            # a host load after a device load
    state_error(bm, s.last_load_ms)
    assert np.array_equal(s.voxels(), volume.astype(bool))
    s.close()


def _frames_and_edits(bm, torch, scene, streams, wait):
    """20 ordered 64 x 64 frames, frame i on streams[i % len(streams)], a small box put on the floor after every fourth; wait: the host
    waits after every call.  Returns the 20 images."""
    cam = bm.Camera(position=(64.0, 10.0, 70.0), horizontal_angle=0.0, vertical_angle=-0.6).update()
    images = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(20)]
    torch.cuda.synchronize()
    for i, image in enumerate(images):
        stream = streams[i % len(streams)].cuda_stream
        scene.render(cam, bm.FrameParams(W, H, spp=1, max_bounces=3, flags=bm.BM_FLAG_ORDERED), image, stream=stream)
        if wait:
            torch.cuda.synchronize()
        if i % 4 == 3:
            k = i // 4
            scene.fill_box((40 + 8 * k, 70, 16), (48 + 8 * k, 78, 24 + 4 * k), stream=stream)
            if wait:
                torch.cuda.synchronize()
    torch.cuda.synchronize()
    return [image.cpu().numpy().view(np.uint32) for image in images]


def test_more_streams_than_the_table_holds(bm, torch_cuda, volume):
    torch = torch_cuda
    one, many = bm.Scene.from_voxels(volume), bm.Scene.from_voxels(volume)
    want = _frames_and_edits(bm, torch, one, [torch.cuda.current_stream()], True)
    got = _frames_and_edits(bm, torch, many, [torch.cuda.Stream() for _ in range(20)], False)
    assert want[0].any() and np.array_equal(want[0], want[3]), "the same frame of the same world"
    assert all(not np.array_equal(want[4 * k + 3], want[4 * k + 4]) for k in range(4)), "every edit changes what the frames see"
    for i in range(20):
        assert np.array_equal(got[i], want[i]), f"frame {i}, on a stream of its own, differs from the frame issued alone"
    assert np.array_equal(one.voxels(), many.voxels())
    one.close()
    many.close()


def test_query_ring_wraps(bm, torch_cuda, volume):
    torch = torch_cuda
    s = bm.Scene.from_voxels(volume)
    rng = np.random.default_rng(15)
    sets = []
    for _ in range(70):
        rays = np.zeros((256, 8), np.float32)
        rays[:, 0:3] = rng.uniform(1.0, G - 1.0, (256, 3))
        d = rng.normal(size=(256, 3))
        rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
        rays[:, 6] = np.inf
        sets.append(torch.from_numpy(rays).to("cuda:0"))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got = [s.cast_rays(rays, stream=streams[k % 2].cuda_stream).packed for k, rays in enumerate(sets)]
    torch.cuda.synchronize()
    got = [g.cpu().numpy().view(np.uint32) for g in got]
    hits = 0
    for k, rays in enumerate(sets):
        want = s.cast_rays(rays).packed
        torch.cuda.synchronize()
        want = want.cpu().numpy()
        hits += int(np.isfinite(want[:, 0]).sum())
        assert np.array_equal(got[k], want.view(np.uint32)), f"query {k} of 70 in flight differs from the query made alone"
    assert hits > 70 * 64
    s.close()


def test_volume_scratch_grows_behind_a_query_in_flight(bm, torch_cuda, volume):
    torch = torch_cuda
    s = bm.Scene.from_voxels(volume)
    rng = np.random.default_rng(16)

    def boxes(n):
        lo = rng.integers(-8, G - 8, (n, 3))
        return torch.from_numpy(bm.volume_box(lo, lo + rng.integers(1, 40, (n, 3))).view(np.uint8).reshape(n, 48)).to("cuda:0")

    # the item offsets take (n + ceil(n / 256) + 1) * 8 bytes and start at 64 KiB: 300 records fit, 9000 (72 296 bytes) do not
    small, large = boxes(300), boxes(9000)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    got = [s.query_volumes(small, stream=a.cuda_stream).packed, s.query_volumes(large, stream=b.cuda_stream).packed]
    torch.cuda.synchronize()
    for g, records in zip(got, (small, large)):
        want = s.query_volumes(records).packed
        torch.cuda.synchronize()
        assert int(want[:, 0:8].view(torch.int64).sum()) > 0
        assert torch.equal(g, want), f"{records.shape[0]} volumes: the query in flight differs from the query made alone"
    s.close()


def test_label_scratch_grows_behind_a_call_in_flight(bm, torch_cuda, volume):
    torch = torch_cuda
    s = bm.Scene.from_voxels(volume)
    # the root counts take (ceil(voxels / 1024) + 1) * 8 bytes and start at 64 KiB: a box of 64^3 fits, one of 208^3 (70 320 bytes) does not
    boxes = (((32, 32, 16), (96, 96, 80)), ((-40, -40, -40), (168, 168, 168)))  # above the floor: parts of both towers and a piece in the air; everything
    capacity = 64
    from brickmap_amd.host import COMPONENT_DTYPE
    width = COMPONENT_DTYPE.itemsize // 8
    tables = [torch.zeros((capacity, width), dtype=torch.int64, device="cuda:0") for _ in boxes]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got = []
    for (lo, hi), table, stream in zip(boxes, tables, streams):
        labels, count = s.label_region(lo, hi, stream=stream.cuda_stream)
        s.label_components_raw(lo, hi, labels.data_ptr(), table.data_ptr(), capacity, stream.cuda_stream)
        got.append((labels, count))
    torch.cuda.synchronize()
    for (lo, hi), table, (labels, count) in zip(boxes, tables, got):
        want = s.components(lo, hi)
        n = len(want.records)
        assert 1 < n <= capacity and int(count.item()) == n
        assert torch.equal(labels, want.labels), f"box {lo} ... {hi}: labels differ from the call made alone"
        assert torch.equal(table[:n], want._table[:n]), f"box {lo} ... {hi}: the component table differs from the call made alone"
    s.close()


def _device_world(scene):
    """the index words of the world's one supercell, the brick the device holds for every cell that names one, and the device's cube field"""
    words = scene.device_indices(0)
    bricks = {int(j): scene.device_brick(0, int(words[j]) & 0xFFF) for j in np.flatnonzero(words & np.uint32(0x80000000))}
    return words, bricks, scene.device_cube_field()


def test_edit_staging_grows_behind_a_batch_in_flight(bm, torch_cuda, volume):
    torch = torch_cuda
    # a batch is staged in 76 bytes a cell (cell, word, arena slot, brick) and the staging starts at 64 KiB: one cell fits; the 2048 cells of eight
    # layers of the world (155 648 bytes, and a pool move: the exact-fit pool of a loaded world grows) do not, so the staging grows while the
    # batch before may still be running; the region write of the same box then packs 2048 bricks (128 KiB), more than its 64 KiB as well
    lo, hi = (0, 0, 56), (G, G, 120)
    z, y, x = np.indices((64, G, G))
    pattern = (((x // 4 + y // 4 + z // 4) & 1) == 0).astype(np.uint8)  # every brick of the box gets a checkerboard of 4-voxel blocks
    dev = torch.from_numpy(pattern).to("cuda:0")
    worlds = []
    for wait in (False, True):
        s = bm.Scene.from_voxels(volume)
        torch.cuda.synchronize()
        for call in (lambda: s.fill_box(*AIR), lambda: s.fill_box(lo, hi), lambda: s.write_region(lo, dev)):
            call()
            if wait:
                s.synchronize()
                torch.cuda.synchronize()
        s.synchronize()
        worlds.append(_device_world(s))
        want = volume.copy()
        want[56:120] = pattern
        assert np.array_equal(s.voxels(), want.astype(bool))
        s.close()
    (words, bricks, field), (words_1, bricks_1, field_1) = worlds
    assert len(bricks_1) >= 2048 + 512, "the floor and the eight layers"
    assert np.array_equal(words, words_1), "index words differ from the calls made one by one"
    assert bricks.keys() == bricks_1.keys() and all(np.array_equal(bricks[j], bricks_1[j]) for j in bricks), "bricks differ from the calls made one by one"
    assert np.array_equal(field, field_1), "the cube field differs from the calls made one by one"


def test_patch_list_grows_behind_a_read_in_flight(bm, torch_cuda):
    torch = torch_cuda
    # a device read of a streaming scene lists the bricks the device does not hold in 12 bytes a cell + 64 a brick (the bricks on a 64-byte
    # line), and the list starts at 64 KiB: 862 bricks fit.  Four layers of cells are 16 x 16 x 4 = 1024 bricks (77 824 bytes), so the list
    # grows while the read before may still use it -- and label_region of the same box then takes the same list
    vox = np.zeros((G, G, G), np.uint8)
    vox[:32] = 1
    s = bm.Scene.from_voxels(vox).reset_residency()  # streaming, nothing resident: every brick of a box is listed
    assert s.info()["resident_bricks"] == 0
    cell, whole = ((0, 0, 0), (8, 8, 8)), ((0, 0, 0), (G, G, G))
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    s.synchronize()
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        small = s.read_region(*cell, device=True)
    with torch.cuda.stream(b):
        large = s.read_region(*whole, device=True)
    with torch.cuda.stream(a):
        labels, count = s.label_region(*whole)
    torch.cuda.synchronize()
    assert s.info()["resident_bricks"] == 0, "a read asks for no bricks"
    for got, box in ((small, cell), (large, whole)):
        want = s.read_region(*box, device=True)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"box {box}: the read in flight differs from the read made alone"
        assert np.array_equal(got.cpu().numpy(), vox[tuple(slice(l, h) for l, h in zip(box[0][::-1], box[1][::-1]))])
    assert int(small.min()) == 1, "a cell of the solid layers"
    want_labels, want_count = s.label_region(*whole)
    torch.cuda.synchronize()
    assert int(count.item()) == int(want_count.item()) == 1, "the four layers are one piece"
    assert torch.equal(labels, want_labels), "labels differ from the call made alone"
    assert np.array_equal(labels.cpu().numpy() != 0, vox != 0)
    s.close()
