"""Voxel edits on the MI355X where the other edit tests do not look: cube-field updates on grids wider than the 254 cells one update
reaches (the box of the field that Scene::edit recomputes is then a part of the grid: halo rows and slices, offsets, the scratch
buffer, and the bytes outside the box), the cap at 254, and the device's words, bricks, LoD masks, slots and flags after edits of
preloaded and of streaming scenes, read back cell by cell.

The field is compared with the host build at every byte and with tests/_edit_model.py::reference_field, which follows the field's
definition (tests/test_field_reference.py validates it on the CPU); the device world with a numpy model of the voxels that the tests
edit alongside (assert_device_world).  Every comparison of field bytes, words, bricks and hit records is exact."""
import warnings

import numpy as np
import pytest

from _edit_model import (CUBIC_CELLS, LOADED, REQUESTED, UNLOADED, FieldModel, all_device_words, apply_to_model, apply_to_scene, assert_device_world, cell_of, changed_bricks,
                         cubic_field_plan, cubic_rays, field_sample_cells, field_update_tmp_bytes, flat_field_plan, model_box, random_batches, reference_field,
                         scratch_growth_plan, tall_field_plan)
from test_gpu_edit import CAM, G, assert_radiance, assert_same, oracle_clear, orender, render
from test_gpu_load import other_content
from test_gpu_query import assert_same_hits, oracle_hits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def device_mib_in_use(torch):
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) >> 20


# ---------------------------------------------------------------- B: field updates on grids wider than one update reaches
class FieldCase:
    """an empty world of size x size x height voxels, loaded from a device tensor, and its cell model"""

    def __init__(self, bm, torch, size, height, every_cell=False, seed=1):
        self.bm, self.torch = bm, torch
        volume = torch.zeros((height, size, size), dtype=torch.uint8, device="cuda:0")
        self.scene = bm.Scene.from_voxels(volume)
        self.peak_mib = device_mib_in_use(torch)
        del volume
        torch.cuda.empty_cache()
        self.model = FieldModel(size // 8, height // 8)
        self.every_cell = every_cell
        self.rng = np.random.default_rng(seed)
        self.kept = {}
        self.field = self.scene.device_cube_field()
        assert np.array_equal(self.field, self.scene.host_cube_field())

    def run(self, plan):
        for name, ops, want in plan:
            if ops:
                self.step(name, ops, want)
            if ">" in name:
                self.kept[name.split(">")[1]] = self.field
            if "=" in name:
                earlier = self.kept[name.split("=")[1]]
                assert np.array_equal(self.field, earlier), f"{name}: {np.count_nonzero(self.field != earlier)} field bytes differ from the earlier ones"

    def step(self, name, ops, want):
        bm, scene, m = self.bm, self.scene, self.model
        changed, box = m.apply(ops, want)  # asserts that the box is partial where the case says
        scene.edit([bm.edit_box(op, lo, hi) for op, lo, hi in ops])
        self.peak_mib = max(self.peak_mib, device_mib_in_use(self.torch))
        dev, host = scene.device_cube_field(), scene.host_cube_field()
        assert np.array_equal(dev, host), f"{name}: {np.count_nonzero(dev != host)} field bytes differ from the host build (update box {box})"
        # bytes outside the box keep their value
        inside = np.zeros(dev.shape[1:], bool)
        inside[box["rz0"]:box["rz1"], box["ry0"]:box["ry1"], box["rx0"]:box["rx1"]] = True
        assert np.array_equal(dev[:, ~inside], self.field[:, ~inside]), f"{name}: field bytes outside the update box changed"
        if self.every_cell:
            want_field = reference_field(m.occ)
            assert np.array_equal(dev, want_field), f"{name}: {np.count_nonzero(dev != want_field)} field bytes differ from the reference"
        else:
            cells = field_sample_cells(m.occ.shape, box, changed, self.rng)
            got = dev[:, cells[:, 2] + 1, cells[:, 1] + 1, cells[:, 0] + 1]
            want_values = reference_field(m.occ, cells)
            assert np.array_equal(got, want_values), f"{name}: {np.count_nonzero(got != want_values)} of {got.size} sampled field bytes differ from the reference"
        assert scene.info()["total_bricks"] == int(m.occ.sum()) and not scene.info()["failed"]
        self.field = dev
        print(f"{name}: {len(changed)} cells changed, update box x [{box['rx0']}, {box['rx1']}) y [{box['ry0']}, {box['ry1']}) z [{box['rz0']}, {box['rz1']}): exact", flush=True)


def test_field_updates_on_a_wide_flat_grid(bm, torch_cuda):
    """4096 x 4096 x 128 voxels (512 x 512 x 16 cells): update boxes free in x and y, clipped on some sides, spanning one axis"""
    torch = torch_cuda
    size, height = 4096, 128
    free, _ = torch.cuda.mem_get_info(0)
    if free < 12 << 30:
        size = 2176
        warnings.warn(f"only {free >> 20} MiB of device memory free: the wide-grid edit test runs on {size} x {size} x {height} instead of 4096 x 4096 x 128")
    case = FieldCase(bm, torch, size, height, seed=1)
    case.run(flat_field_plan(size // 8))
    assert case.scene.info()["total_bricks"] == 0
    peak = case.peak_mib
    case.scene.close()
    # on a fresh scene: a small box, one that spans the width (the scratch buffer grows), a small one again
    case = FieldCase(bm, torch, size, height, seed=2)
    plan = scratch_growth_plan(size // 8)
    m = FieldModel(size // 8, height // 8)
    sizes = [field_update_tmp_bytes(m.apply(ops, want)[1]) for _, ops, want in plan]
    assert sizes[0] < sizes[1] > sizes[2]
    case.run(plan)
    print(f"wide flat grid {size} x {size} x {height}: peak device memory in use {max(peak, case.peak_mib)} MiB")
    case.scene.close()


def test_field_updates_on_a_tall_thin_grid(bm, torch_cuda):
    """128 x 128 x 4096 voxels (16 x 16 x 512 cells): update boxes partial in z, halo slices that differ from the box; every cell"""
    case = FieldCase(bm, torch_cuda, 128, 4096, every_cell=True)
    case.run(tall_field_plan())
    assert not case.scene.voxels().any()
    print(f"tall thin grid 128 x 128 x 4096: peak device memory in use {case.peak_mib} MiB")
    case.scene.close()


def assert_distances_ulp(got, geometric, ulp):
    """the rule of test_gpu_load.py::assert_distances (geometric distance, or that less kEpsilon where the walk measures from the pushed
    entry point of the hit brick), 4 ulps of the coordinate range in use"""
    k_epsilon, tol = 0.001, 4 * ulp
    err = got.astype(np.float64) - geometric
    assert (err <= tol).all() and (err >= -k_epsilon - tol).all(), f"distance errors {err.min():.6f} ... {err.max():.6f}"


def test_field_updates_and_the_cap_on_a_cubic_grid(bm, torch_cuda):
    """2176^3 voxels (272^3 cells): update boxes partial on all three axes at once, field values of 254, rays through more than 254
    empty cells"""
    torch = torch_cuda
    size = CUBIC_CELLS * 8
    free, _ = torch.cuda.mem_get_info(0)
    if free < 24 << 30:
        pytest.skip(f"only {free >> 20} MiB of device memory free: the {size}^3 world needs a {size ** 3 >> 20} MiB volume and the scene next to it")
    case = FieldCase(bm, torch, size, size, seed=3)
    case.run(cubic_field_plan())
    inner = case.field[:, 1:-1, 1:-1, 1:-1]
    assert inner.max() == 254, f"the largest interior field byte is {inner.max()}"
    assert (inner == 254).sum() > 1000
    assert case.field[0, 1, 1, 7] == 254  # anchored at cell (6, 0, 0) along +x +y +z: a cube of 254 cells that avoids both voxels
    origins, directions, voxels, distances = cubic_rays()
    hits = case.scene.cast_rays(origins, directions)
    hit = np.array([v is not None for v in voxels])
    assert hit.sum() == 6 and (~hit).sum() == 24
    assert np.array_equal(hits.level, np.where(hit, 2, -1)), f"levels {hits.level}"
    assert np.isinf(hits.distance[~hit]).all() and (hits.voxel[~hit] == -1).all() and (hits.normal[~hit] == 0).all()
    assert np.array_equal(hits.voxel[hit], np.array([v for v in voxels if v is not None]))
    assert np.array_equal(hits.normal[hit], -directions[hit])
    print("cubic grid: distance errors", hits.distance[hit].astype(np.float64) - distances[hit])
    assert_distances_ulp(hits.distance[hit], distances[hit], 2.0 ** -12)  # coordinates in [2048, 4096)
    print(f"cubic grid {size}^3: peak device memory in use {case.peak_mib} MiB")
    case.scene.close()


# ---------------------------------------------------------------- C: the device world after edits
@pytest.fixture(scope="module")
def terrain(bm, torch_cuda):
    """voxels of the generated 256^3 world"""
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    vox = scene.voxels().copy()
    assert_device_world(scene, vox)
    scene.close()
    return vox


def loaded_slots(scene):
    """{(supercell, cell): device slot} of the loaded words"""
    out = {}
    for sc in range(scene.info()["supercells"]):
        w = scene.device_indices(sc)
        for cell in np.nonzero(w & np.uint32(LOADED))[0]:
            out[(sc, int(cell))] = int(w[cell] & np.uint32(0xFFF))
    return out


def test_preloaded_scene_after_random_edits(bm, torch_cuda, terrain):
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    model = terrain.copy()
    batches = random_batches()
    assert len(batches) >= 30
    before = loaded_slots(scene)
    pool_bytes = scene.info()["pool_bytes"]
    free_slots = set()
    freed = reused = grown = 0
    for k, batch in enumerate(batches):
        apply_to_scene(bm, scene, batch)
        apply_to_model(model, batch)
        loaded = assert_device_world(scene, model)
        assert loaded == scene.info()["total_bricks"], f"batch {k}: a preloaded scene holds a brick that is not resident"
        after = loaded_slots(scene)
        for key, slot in before.items():
            if key not in after:
                free_slots.add((key[0], slot))
                freed += 1
            else:
                assert after[key] == slot, f"batch {k}: a resident brick moved to another slot"
        for key, slot in after.items():
            if key not in before and (key[0], slot) in free_slots:
                free_slots.discard((key[0], slot))
                reused += 1
        now = scene.info()["pool_bytes"]
        grown += now > pool_bytes
        before, pool_bytes = after, now
        print(f"batch {k}: {loaded} bricks resident, {freed} slots freed and {reused} reused so far, {grown} batches grew a pool", flush=True)
    assert freed >= 100 and reused >= 1 and grown >= 1, f"freed {freed} slots, reused {reused}, {grown} batches grew a pool"
    assert np.array_equal(scene.device_cube_field(), scene.host_cube_field())
    scene.close()


def test_pools_that_grow_from_nothing(bm, torch_cuda):
    vol = other_content()
    solid = vol != 0
    scene = bm.Scene(G, G, device=0).generate().preload_all()
    scene.clear_box((0, 0, 0), (G, G, G))
    empty = np.zeros_like(solid)
    assert assert_device_world(scene, empty) == 0
    z, y, x = np.nonzero(solid)
    coords = np.stack([x, y, z], 1).astype(np.int32)
    for k in range(0, len(coords), 1 << 18):
        scene.set_voxels(coords[k:k + (1 << 18)], 1)
    assert_device_world(scene, vol)
    words = scene.device_indices(7)  # supercell (1, 1, 1) is all solid: 4096 bricks, every slot of a full pool
    assert ((words & np.uint32(LOADED)) != 0).all() and np.array_equal(np.sort(words & np.uint32(0xFFF)), np.arange(4096))
    scene.close()


# three regions in what the camera sees, each across the supercell border at y = 128 (the middle one also across x = 128 ... 160), and
# three blocks of sky on the camera's rays through pixels (48, 32), (76, 24) and (30, 40) of a 96 x 64 frame, in front of the terrain
REGIONS = (((100, 70, 60), (130, 160, 200)), ((130, 70, 60), (160, 160, 200)), ((160, 70, 60), (190, 160, 200)))
SKY = (((144, 48, 188), (150, 54, 194)), ((154, 35, 195), (160, 41, 200)), ((134, 57, 182), (140, 63, 188)))


def pick_brick(scene, model, bit, avoid):
    """a cell whose device word has `bit` set, outside the regions, with at least two voxels in the model: (supercell, cell, global cell)"""
    info = scene.info()
    for sc in range(info["supercells"]):
        w = scene.device_indices(sc)
        for cell in np.nonzero(w & np.uint32(bit))[0]:
            g = cell_of(info, sc, int(cell))
            if g in avoid or (100 < g[0] * 8 + 8 and g[0] * 8 < 190 and 70 < g[1] * 8 + 8 and g[1] * 8 < 160):
                continue
            if model[g[2] * 8:g[2] * 8 + 8, g[1] * 8:g[1] * 8 + 8, g[0] * 8:g[0] * 8 + 8].sum() >= 2:
                return sc, int(cell), g
    return None


def streaming_batch(bm, scene, model, k, sky, resident, requested):
    """the batch of state k on the scene and on the model: region k cleared and a subset set back, a block of sky set (sky variant), one
    voxel cleared in a resident and in a requested brick (where the state has them).  Returns the changed brick cells."""
    before = model.copy()
    lo, hi = REGIONS[k]
    scene.clear_box(lo, hi)
    z, y, x = np.nonzero(model[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]])
    x, y, z = x + lo[0], y + lo[1], z + lo[2]
    keep = (x + y + z) % 3 == 0
    assert keep.any() and (~keep).any()
    scene.set_voxels(np.stack([x[keep], y[keep], z[keep]], 1).astype(np.int32), 1)
    model[z[~keep], y[~keep], x[~keep]] = False
    edits = []
    if sky:
        slo, shi = SKY[k]
        assert not model[slo[2]:shi[2], slo[1]:shi[1], slo[0]:shi[0]].any(), "the block of sky is not empty"
        edits.append(bm.edit_box("set", slo, shi))
        model_box(model, "set", slo, shi)
    for pick in (resident, requested):
        if pick is None:
            continue
        g = pick[2]
        z, y, x = np.argwhere(model[g[2] * 8:g[2] * 8 + 8, g[1] * 8:g[1] * 8 + 8, g[0] * 8:g[0] * 8 + 8])[0]
        v = (g[0] * 8 + int(x), g[1] * 8 + int(y), g[2] * 8 + int(z))
        edits.append(bm.edit_box("clear", v, tuple(c + 1 for c in v)))
        model[v[2], v[1], v[0]] = False
    if edits:
        scene.edit(edits)
    return changed_bricks(before, model)


def settle(bm, torch, scene, cam):
    for _ in range(64):
        render(bm, torch, scene, cam)
        if scene.process_load_queue() == 0 and scene.process_load_queue() == 0:
            return
    pytest.fail("streaming did not reach a steady state")


@pytest.mark.parametrize("variant", ["sky", "removal"])
@pytest.mark.parametrize("overlapped", [0, 1], ids=["blocking", "overlapped"])
def test_edits_of_a_streaming_scene(overlapped, variant, bm, orc, torch_cuda, terrain):
    torch = torch_cuda
    sky = variant == "sky"
    scene = bm.Scene(G, G, device=0)
    scene.set_queue_capacity(1 << 16)
    scene.generate().set_streaming_mode(overlapped)
    model = terrain.copy()
    cam = bm.Camera(**CAM).update()
    info = scene.info()
    freed = set()

    def batch(k, resident=None, requested=None):
        before = loaded_slots(scene)
        words = {p[:2]: int(scene.device_indices(p[0])[p[1]]) for p in (resident, requested) if p is not None}
        changed = streaming_batch(bm, scene, model, k, sky, resident, requested)
        loaded = assert_device_world(scene, model, changed)
        print(f"state {k + 1}: {len(changed)} bricks changed, {loaded} of {scene.info()['total_bricks']} resident after the batch", flush=True)
        after = loaded_slots(scene)
        freed.update((key[0], slot) for key, slot in before.items() if key not in after)
        assert all(after[key] == slot for key, slot in before.items() if key in after), "a resident brick moved to another slot"
        if resident is not None:  # rewritten in place: the same slot, still loaded (its content: assert_device_world)
            w = int(scene.device_indices(resident[0])[resident[1]])
            assert w & LOADED and (w & 0xFFF) == (words[resident[:2]] & 0xFFF)
        if requested is not None:  # unloaded | lod, asked for again
            w = int(scene.device_indices(requested[0])[requested[1]])
            assert w & UNLOADED and not w & (LOADED | REQUESTED | 0xFFF)

    # state 1: nothing resident, nothing requested
    assert not (all_device_words(scene) & np.uint32(LOADED | REQUESTED)).any()
    batch(0)
    assert scene.info()["resident_bricks"] == 0
    # state 2: partly resident
    for _ in range(2):
        render(bm, torch, scene, cam)
        scene.process_load_queue()
    assert 0 < scene.info()["resident_bricks"] < scene.info()["total_bricks"]
    resident = pick_brick(scene, model, LOADED, ())
    assert resident is not None
    batch(1, resident=resident)
    # state 3: requests stand in the ring and are not serviced yet (overlapped: the ring has been copied out, the next call services it)
    render(bm, torch, scene, cam)
    if overlapped:
        scene.process_load_queue()
    resident = pick_brick(scene, model, LOADED, ())
    requested = pick_brick(scene, model, REQUESTED, ())
    assert resident is not None and requested is not None, "the state holds no resident or no requested brick outside the regions"
    batch(2, resident=resident, requested=requested)

    settle(bm, torch, scene, cam)
    assert not scene.info()["failed"]
    assert_device_world(scene, model)
    assert freed, "no batch emptied a resident brick"
    now = loaded_slots(scene)
    assert any((key[0], slot) in freed for key, slot in now.items()), "servicing reused no freed device slot"
    # the final frame equals the frame of the model loaded as a whole (so every brick it hits is resident: it requests nothing), and the
    # camera sees the new blocks of sky
    ref = bm.Scene.from_voxels(model)
    got, want = render(bm, torch, scene, cam), render(bm, torch, ref, cam)
    assert np.array_equal(got[1], want[1]), f"{np.count_nonzero((got[1] != want[1]).any(-1))} pixels whose hit records differ from the loaded model's"
    assert_radiance(got[0], want[0])
    assert got[2]["requests"] == 0
    if sky:
        px, py = np.meshgrid(np.arange(96) + 0.5, np.arange(64) + 0.5)
        hits = ref.cast_rays(bm.camera_pixel_rays(cam, 96, 64, px.ravel(), py.ravel()))
        for lo, hi in SKY:
            assert ((hits.voxel >= lo).all(1) & (hits.voxel < hi).all(1) & (hits.level == 2)).any(), f"no primary ray hits the block of sky at {lo}"
    w = None
    if not sky:  # only original voxels were removed: the oracle's world, edited in place, is the same world
        w = orc.World(G, G)
        oracle_clear(w, terrain & ~model)
        w.reset_device(True)
        assert_same(got, orender(orc, w, cam), counters=False)
    scene.preload_all()
    assert assert_device_world(scene, model) == scene.info()["total_bricks"]
    got = render(bm, torch, scene, cam)
    assert np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert_radiance(got[0], want[0])
    if w is not None:
        assert_same(got, orender(orc, w, cam))
    assert info["supercells"] == scene.info()["supercells"]
    ref.close()
    scene.close()


def rays_that_enter(rays, hits, lo, hi):
    """rays whose segment up to their hit passes through the box [lo, hi)"""
    o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    within = (o >= lo) & (o < hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    near = np.where(d != 0, np.minimum(t0, t1), np.where(within, -np.inf, np.inf))
    far = np.where(d != 0, np.maximum(t0, t1), np.where(within, np.inf, -np.inf))
    enter = np.maximum(near.max(1), 0)
    return (enter < far.min(1)) & (enter < hits["distance"])


def test_lod_queries_after_an_edit_match_the_oracle(bm, orc, torch_cuda):
    size, height = 1024, 256
    lod8, lod2 = 40 ** 2, 16 ** 2  # the thresholds of test_gpu_query.py::test_lod_mode_matches_the_oracle
    lo, hi = (480, 96, 48), (544, 736, 256)  # a trench from next to the LoD origin to 75 cells away from it
    scene = bm.Scene(size, height, device=0).generate().preload_all()
    scene.set_lod(lod8, lod2)
    scene.clear_box(lo, hi)
    world = orc.World(size, height)
    removed = np.zeros((height, size, size), bool)
    removed[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    oracle_clear(world, removed)
    del removed
    world.reset_device(True)
    world.set_lod(lod8, lod2)
    origin = np.array([0.5 * size, 0.125 * size, 0.8 * height], np.float32)
    campos = [int(np.float32(v) / np.float32(8)) for v in origin]
    # straight down into the trench along its length, and three cameras that look along it and into it
    xs, ys = np.meshgrid(np.arange(484, 544, 8), np.arange(100, 732, 5))
    o = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5, np.full(xs.size, height - 0.5)], 1).astype(np.float32)
    rays = [bm.pack_rays(o, np.tile(np.float32([0, 0, -1]), (len(o), 1)))]
    for pos, h, v in (((512, 100, 220), 0.0, -0.35), ((500, 60, 200), 0.05, -0.2), ((530, 400, 240), 3.1, -0.5)):
        cam = bm.Camera(position=pos, horizontal_angle=h, vertical_angle=v).update()
        px, py = np.meshgrid(np.linspace(0.5, 319.5, 30, dtype=np.float32), np.linspace(0.5, 179.5, 30, dtype=np.float32))
        rays.append(bm.camera_pixel_rays(cam, 320, 180, px.ravel(), py.ravel()))
    rays = np.concatenate(rays)
    want = oracle_hits(world, rays, campos)
    entering = rays_that_enter(rays, want, lo, hi)
    for lv in (0, 1, 2):
        assert (want["level"][entering] == lv).sum() > 50, f"level {lv} does not occur among the rays that enter the edited region"
    got = scene.cast_rays(rays, lod_origin=origin).packed
    assert_same_hits(got, want, "LoD after an edit")
    assert np.array_equal(scene.device_cube_field(), scene.host_cube_field())
    scene.close()
