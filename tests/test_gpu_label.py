"""Scene.label_region, Scene.components, Components.mask / floating and Scene.remove_floating on the MI355X (csrc/label.hip): connected
components of a box of the live scene.  The model of every case is host_label_volume(read_region(lo, hi)) -- the host routine that
tests/test_label_host.py pins to numpy -- and the component table comes from tests/_label_model.py.  Every number is an integer, every
comparison exact.  Worlds: the three seeded worlds of tests/_box_cases.py (fill 0.3: many small pieces), a fill-0.5 volume (a few giant
ones), the generated 256^3 terrain (one huge piece: every link contended on one root) and hand-made shapes placed across the supercell
boundaries at 128."""
import ctypes as C
import time

import numpy as np
import pytest

import _label_model as model
from _box_cases import WORLDS, axis_sweep, random_boxes, streaming_scene, world_voxels, x_sweep
from _edit_model import all_device_words

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = 10001, 10002


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def preloaded(bm, torch_cuda):
    """world -> a scene of it with every brick resident, built on first use"""
    scenes = {}

    def get(world):
        if world not in scenes:
            scenes[world] = bm.Scene.from_voxels(world_voxels(world))
        return scenes[world]

    yield get
    for s in scenes.values():
        s.close()


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_label.py took {time.time() - t0:.1f} s")


def expected(bm, scene, lo, hi):
    """the model: the host routine on what read_region gives for the box"""
    return bm.host_label_volume(scene.read_region(lo, hi))


def check_box(bm, scene, lo, hi, what=""):
    labels, count = scene.label_region(lo, hi)
    want, n = expected(bm, scene, lo, hi)
    got = labels.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.int32
    assert int(count.item()) == n, f"{what}{lo} ... {hi}: {int(count.item())} components, the model has {n}"
    assert np.array_equal(got, want), f"{what}{lo} ... {hi}: {np.count_nonzero(got != want)} labels differ"
    return got, n


# ---------------------------------------------------------------- box edges in the seeded worlds
@pytest.mark.parametrize("sweep", ["x", "y", "z", "random"])
@pytest.mark.parametrize("world", ["cube", "flat", "tall"])
def test_box_edges(world, sweep, bm, torch_cuda, preloaded):
    dims = WORLDS[world]
    if sweep == "x":
        boxes = x_sweep(dims, "general")
    elif sweep == "random":
        boxes = random_boxes(dims, "general", n=150, seed=len(world))[:-1]  # (the box that contains the world: below)
    else:
        boxes = axis_sweep(dims, "general", "xyz".index(sweep))
    scene = preloaded(world)
    solid = 0
    for lo, hi in boxes:
        got, n = check_box(bm, scene, lo, hi, f"{world} {sweep} ")
        solid += n
    assert solid > len(boxes)
    if sweep == "random":
        lo, hi = boxes[-1]
        assert lo[0] >= dims[0], "the last box lies wholly outside"
        labels, count = scene.label_region(lo, hi)
        assert int(count.item()) == 0 and not labels.any().item()


@pytest.mark.parametrize("world", ["flat", "tall"])
def test_a_box_that_contains_the_world(world, bm, torch_cuda, preloaded):
    """labels against the host routine, and the table against numpy: its faces refer to the clipped box, the world"""
    dims = WORLDS[world]
    lo, hi = (-13, -3, -2), (dims[0] + 5, dims[1] + 4, dims[2] + 3)
    scene = preloaded(world)
    got, n = check_box(bm, scene, lo, hi, world + " ")
    comps = scene.components(lo, hi)
    want = model.model_records(got, lo, dims)
    assert len(comps) == n == len(want) and np.array_equal(comps.records, want)
    for bit in range(6):
        assert (want["faces"] >> bit & 1).any(), f"no component on face {model.FACES[bit]} of the world"


def test_the_whole_cube_world_in_one_call(bm, torch_cuda, preloaded):
    """about a million components: labels and count against the host routine, the full table against numpy"""
    dims = WORLDS["cube"]
    scene = preloaded("cube")
    got, n = check_box(bm, scene, (0, 0, 0), dims, "cube ")
    assert n > 900_000
    comps = scene.components((0, 0, 0), dims)
    want = model.model_records(got, (0, 0, 0), dims)
    assert len(want) == n and np.array_equal(comps.records, want)
    assert want["voxels"].max() > 1000 and (want["voxels"] == 1).sum() > 100_000


# ---------------------------------------------------------------- a few giant pieces, and one huge one
def test_fill_one_half(bm, torch_cuda):
    vol = np.zeros((128, 256, 256), np.uint8)
    vol[20:116, 70:166, 75:171] = model.seeded_volume(77, (96, 96, 96), 0.5)
    scene = bm.Scene.from_voxels(vol)
    try:
        got, n = check_box(bm, scene, (70, 66, 15), (175, 170, 120), "fill 0.5 ")
        sizes = np.bincount(got.reshape(-1))[1:]
        assert sizes.max() > 300_000 and n > 1000, "one giant piece and many crumbs"
        check_box(bm, scene, (101, 99, 33), (163, 150, 90), "fill 0.5, a cut ")
    finally:
        scene.close()


def test_generated_terrain(bm, torch_cuda):
    scene = bm.Scene(256, 256, device=0).generate().preload_all()
    try:
        got, n = check_box(bm, scene, (0, 0, 0), (256, 256, 256), "terrain ")
        sizes = np.bincount(got.reshape(-1))[1:]
        assert sizes.max() > 0.9 * np.count_nonzero(got), "the terrain is one huge component"
        comps = scene.components((0, 0, 0), (256, 256, 256))
        assert np.array_equal(comps.records, model.model_records(got, (0, 0, 0), (256, 256, 256)))
        # after a dig, remove_floating removes exactly the model's voxels: the crumbs of the noise and what the dig cut loose
        scene.edit([bm.edit_sphere(bm.BM_EDIT_CLEAR, (128, 128, 60), 40), bm.edit_sphere(bm.BM_EDIT_SET, (128, 128, 60), 10)])  # (leaves a ball in the air)
        vox = scene.voxels() != 0
        labels, _ = bm.host_label_volume(vox)
        recs = model.model_records(labels, (0, 0, 0), (256, 256, 256))
        loose = recs[(recs["faces"] & 0b011111) == 0]
        assert len(loose) > 0 and loose["voxels"].max() > 4000
        assert scene.remove_floating((0, 0, 0), (256, 256, 256)) == (len(loose), int(loose["voxels"].sum()))
        assert np.array_equal(scene.voxels() != 0, vox & ~np.isin(labels, loose["label"]))
    finally:
        scene.close()


# ---------------------------------------------------------------- hand-made shapes across the supercell boundaries
def placed(name, tall):
    """(world volume, lo, hi): the shape in a 256 x 256 x 128 world across x = 128 and y = 128, or in the 128 x 128 x 384 one across z = 128"""
    v = model.shape(name)
    nz, ny, nx = v.shape
    if tall:
        world = np.zeros((384, 128, 128), np.uint8)
        lo = (37, 21, 128 - nz // 2 - 1)
    else:
        world = np.zeros((128, 256, 256), np.uint8)
        lo = (128 - nx // 2 - 3, 128 - ny // 2 + 1, 5)
    world[lo[2]:lo[2] + nz, lo[1]:lo[1] + ny, lo[0]:lo[0] + nx] = v
    return world, lo, (lo[0] + nx, lo[1] + ny, lo[2] + nz)


@pytest.mark.parametrize("tall", [False, True])
@pytest.mark.parametrize("name", model.SHAPES)
def test_hand_made_shapes(name, tall, bm, torch_cuda):
    world, lo, hi = placed(name, tall)
    scene = bm.Scene.from_voxels(world)
    try:
        got, n = check_box(bm, scene, lo, hi, name + " ")
        assert n == model.SHAPE_COUNTS[name]
        wide_lo, wide_hi = tuple(v - 5 for v in lo), tuple(v + 6 for v in hi)
        _, n = check_box(bm, scene, wide_lo, wide_hi, name + " with a margin ")
        assert n == model.SHAPE_COUNTS[name]
        check_box(bm, scene, tuple(v + 3 for v in lo), tuple(v - 2 for v in hi), name + " cut ")
        comps = scene.components(wide_lo, wide_hi)
        assert np.array_equal(comps.records, model.model_records(comps.labels.cpu().numpy(), wide_lo, world.shape[::-1]))
        assert (comps.records["faces"] == 0).all() and comps.records["voxels"].sum() == world.sum()
    finally:
        scene.close()


@pytest.mark.parametrize("capacity", ["smaller", "equal", "larger"])
def test_checkerboard_table_capacity(capacity, bm, torch_cuda):
    """truncation gives exactly the first records; records past the count are untouched"""
    torch = torch_cuda
    world, lo, hi = placed("checkerboard", False)
    scene = bm.Scene.from_voxels(world)
    try:
        labels, count = scene.label_region(lo, hi)
        n = int(count.item())
        assert n == model.SHAPE_COUNTS["checkerboard"]
        want = model.model_records(labels.cpu().numpy(), lo, world.shape[::-1])
        assert (want["voxels"] == 1).all()
        cap = {"smaller": 301, "equal": n, "larger": n + 77}[capacity]
        table = torch.full((n + 100, 5), 0x7A7A7A7A7A7A7A7A, dtype=torch.int64, device="cuda:0")
        scene.label_components_raw(lo, hi, labels.data_ptr(), table.data_ptr(), cap)
        torch.cuda.synchronize()
        got = table.cpu().numpy()
        k = min(cap, n)
        assert np.array_equal(got[:k].view(model.COMPONENT_DTYPE).reshape(-1), want[:k])
        assert (got[k:] == 0x7A7A7A7A7A7A7A7A).all(), "a record past min(capacity, count) was written"
        # the mask of a truncated table: labels that are not in it give 0
        chosen = torch.ones(k, dtype=torch.uint8, device="cuda:0") * 3
        mask = torch.full(tuple(labels.shape), 9, dtype=torch.uint8, device="cuda:0")
        scene.label_mask_raw(lo, hi, labels.data_ptr(), table.data_ptr(), k, chosen.data_ptr(), mask.data_ptr())
        lab = labels.cpu().numpy()
        assert np.array_equal(mask.cpu().numpy(), np.where(np.isin(lab, want["label"][:k]) & (lab != 0), 3, 0).astype(np.uint8))
    finally:
        scene.close()


# ---------------------------------------------------------------- streaming
@pytest.mark.parametrize("world", ["cube", "tall"])
def test_streaming_scene_gives_the_preloaded_result(world, bm, torch_cuda, preloaded):
    dims = WORLDS[world]
    scene = streaming_scene(bm, torch_cuda, world)
    try:
        words, info = all_device_words(scene), scene.info()
        for lo, hi in [((0, 0, 0), dims), ((-3, 5, 7), (dims[0] - 9, dims[1] + 2, min(dims[2], 200) - 1)), ((100, 20, 30), (190, 110, 140))]:
            labels, count = scene.label_region(lo, hi)
            want, wcount = preloaded(world).label_region(lo, hi)
            assert int(count.item()) == int(wcount.item()) > 0 and torch_cuda.equal(labels, want), f"{world} {lo} ... {hi}"
        assert scene.info()["resident_bricks"] == info["resident_bricks"] < info["total_bricks"]
        assert np.array_equal(all_device_words(scene), words), "a label call wrote an index word"
        assert scene.process_load_queue() == 0, "a label call filed a request"
    finally:
        scene.close()


# ---------------------------------------------------------------- ordering
def test_ordering_and_repeatability(bm, torch_cuda):
    torch = torch_cuda
    scene = bm.Scene.from_voxels(world_voxels("cube"))
    try:
        lo, hi = (90, 80, 70), (170, 175, 150)
        before, _ = expected(bm, scene, lo, hi)
        side = torch.cuda.Stream()
        old, old_count = scene.label_region(lo, hi, stream=side.cuda_stream)   # issued before the edit, on another stream
        scene.carve_sphere((128, 128, 110), 30)
        new, new_count = scene.label_region(lo, hi)                             # issued after it
        torch.cuda.synchronize()
        after, n_after = expected(bm, scene, lo, hi)
        assert np.array_equal(old.cpu().numpy(), before) and not np.array_equal(before, after)
        assert np.array_equal(new.cpu().numpy(), after) and int(new_count.item()) == n_after != int(old_count.item())
        again, _ = scene.label_region(lo, hi)
        out = torch.full(tuple(new.shape), -1, dtype=torch.int32, device="cuda:0")
        mine, _ = scene.label_region(lo, hi, out=out, stream=side.cuda_stream)
        torch.cuda.synchronize()
        assert mine is out and torch.equal(again, new) and torch.equal(out, new), "the same call gives the same bytes"
    finally:
        scene.close()


# ---------------------------------------------------------------- floating pieces
def test_floating_and_remove_floating(bm, torch_cuda):
    world = np.zeros((128, 256, 256), np.uint8)
    world[0:4] = 1                              # the ground
    world[4:100, 123:134, 122:133] = 1          # a pillar across x = 128 and y = 128
    world[60:64, 30:40, 200:203] = 1            # a crumb that floats from the start
    scene = bm.Scene.from_voxels(world)
    try:
        dims = (256, 256, 128)
        assert scene.remove_floating((0, 0, 0), dims, anchor=("-z",)) == (1, 120)
        scene.carve_sphere((127, 128, 50), 11)   # cuts the pillar
        vox = scene.voxels().astype(np.uint8)
        labels, _ = bm.host_label_volume(vox)
        recs = model.model_records(labels, (0, 0, 0), dims)
        loose = recs[(recs["faces"] & 0b011111) == 0]
        assert len(loose) >= 1 and loose["voxels"].sum() > 4000
        want_mask = np.isin(labels, loose["label"]) & (labels != 0)
        comps = scene.components((0, 0, 0), dims)
        assert np.array_equal(comps.floating().cpu().numpy(), want_mask.astype(np.uint8))
        assert np.array_equal(comps.mask(comps.records["voxels"] > 10 ** 5).cpu().numpy() != 0, np.isin(labels, recs["label"][recs["voxels"] > 10 ** 5]) & (labels != 0))
        solid = scene.count_box((0, 0, 0), dims)
        pieces, voxels = scene.remove_floating((0, 0, 0), dims)
        assert (pieces, voxels) == (len(loose), int(loose["voxels"].sum()))
        assert scene.count_box((0, 0, 0), dims) == solid - voxels
        assert np.array_equal(scene.voxels() != 0, (vox != 0) & ~want_mask), "exactly the model's voxels go"
        assert scene.remove_floating((0, 0, 0), dims) == (0, 0)
        assert scene.count_box((0, 0, 0), dims) == solid - voxels
    finally:
        scene.close()


# ---------------------------------------------------------------- refusals
def test_refusals(bm, torch_cuda):
    torch = torch_cuda
    L = bm.load()
    scene = bm.Scene.from_voxels(world_voxels("tall"))
    bare = bm.Scene(128, 128, device=0)  # no world: not on the device
    try:
        labels = torch.full((10, 10, 12), -5, dtype=torch.int32, device="cuda:0")
        count = torch.full((2,), -5, dtype=torch.int64, device="cuda:0")
        three = C.c_int32 * 3

        def call(lo=(0, 0, 0), hi=(10, 10, 10), flags=0, lab=labels.data_ptr(), cnt=count.data_ptr(), s=scene):
            return L.bm_scene_label_region(s.gpuScene, C.byref(three(*lo)), C.byref(three(*hi)), flags, C.c_void_p(lab), C.c_void_p(cnt), None)

        big = 2 ** 20
        for kw in (dict(hi=(10, -1, 10)), dict(lo=(5, 0, 0), hi=(4, 10, 10)), dict(lo=(-big, -big, -big), hi=(big, big, big)),
                   dict(lo=(0, 0, 0), hi=(2 ** 16, 2 ** 15, 1)), dict(flags=1), dict(flags=0x80000000), dict(lab=None), dict(cnt=None),
                   dict(lab=labels.data_ptr() + 2), dict(cnt=count.data_ptr() + 4), dict(hi=(1000, 1000, 100))):  # (the last: 400 MB from a pointer into a small allocation)
            assert call(**kw) == EINVAL, kw
            assert b"bm_scene_label_region" in L.bm_last_error_string()
        assert call(s=bare) == ESTATE
        torch.cuda.synchronize()
        assert (labels == -5).all().item() and (count == -5).all().item(), "a refused call touched a buffer"
        # 2^31 - 2 voxels is the limit: one more is refused on the volume alone (the span check would refuse both)
        assert call(hi=(2 ** 16, 2 ** 15, 1)) == EINVAL and b"2^31 - 2" in L.bm_last_error_string()
        assert call(hi=(2 ** 16 - 1, 2 ** 15, 1)) == EINVAL and b"2^31 - 2" not in L.bm_last_error_string()
        # an empty box writes count 0 and nothing else; the limits that are allowed
        assert call(hi=(10, 0, 10)) == 0 and call(lo=(3, 3, 3), hi=(3, 3, 3), lab=None) == 0
        torch.cuda.synchronize()
        assert count[0].item() == 0 and count[1].item() == -5 and (labels == -5).all().item()
        assert call(hi=(12, 10, 10)) == 0
        torch.cuda.synchronize()
        assert (labels >= 0).all().item() and count[0].item() > 0
        # the Python door: wrong dtype, shape, layout or device raise before the library is called
        for bad in (torch.zeros((10, 10, 12), dtype=torch.int64, device="cuda:0"), torch.zeros((10, 10, 11), dtype=torch.int32, device="cuda:0"),
                    torch.zeros((10, 10, 24), dtype=torch.int32, device="cuda:0")[:, :, ::2], torch.zeros((10, 10, 12), dtype=torch.int32), np.zeros((10, 10, 12), np.int32)):
            with pytest.raises(ValueError):
                scene.label_region((0, 0, 0), (12, 10, 10), out=bad)
        with pytest.raises(ValueError):
            scene.label_region((5, 0, 0), (4, 10, 10))
        comps = scene.components((0, 0, 0), (12, 10, 10))
        with pytest.raises(ValueError):
            comps.mask(np.ones(len(comps) + 1))
        with pytest.raises(ValueError):
            comps.floating(anchor=("up",))
        # the other two calls refuse the same boxes, a negative capacity / count and misaligned tables
        table = torch.zeros((len(comps) + 1, 5), dtype=torch.int64, device="cuda:0")
        lo3, hi3 = three(0, 0, 0), three(12, 10, 10)
        lab = C.c_void_p(comps.labels.data_ptr())
        assert L.bm_scene_label_components(scene.gpuScene, C.byref(lo3), C.byref(hi3), lab, C.c_void_p(table.data_ptr()), -1, None) == EINVAL
        assert L.bm_scene_label_components(scene.gpuScene, C.byref(lo3), C.byref(hi3), lab, C.c_void_p(table.data_ptr() + 4), 5, None) == EINVAL
        assert L.bm_scene_label_components(scene.gpuScene, C.byref(lo3), C.byref(hi3), lab, None, 5, None) == EINVAL
        assert L.bm_scene_label_components(scene.gpuScene, C.byref(lo3), C.byref(three(12, 9, 10)), lab, C.c_void_p(table.data_ptr()), 5, None) == 0
        assert L.bm_scene_label_components(scene.gpuScene, C.byref(lo3), C.byref(three(12, -9, 10)), lab, C.c_void_p(table.data_ptr()), 5, None) == EINVAL
        assert L.bm_scene_label_mask(scene.gpuScene, C.byref(lo3), C.byref(hi3), lab, C.c_void_p(table.data_ptr()), -1, None, None, None) == EINVAL
        assert L.bm_scene_label_mask(scene.gpuScene, C.byref(lo3), C.byref(hi3), lab, C.c_void_p(table.data_ptr()), 2, None, None, None) == EINVAL
        torch.cuda.synchronize()
    finally:
        scene.close()
        bare.close()
