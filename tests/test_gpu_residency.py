"""Which brick is resident where, from outside (csrc/residency.cpp, csrc/pool_book.h): a 256 x 256 x 128 world of four supercells, built from
voxels and reset to "nothing resident"; requests are raised by rays cast straight down onto chosen brick columns, serviced in both streaming
modes, crossed with edits, and the device world is compared cell by cell with a numpy model (assert_device_world) and with bm_scene_info
(resident_bricks, pool_bytes, failed).  The world: supercell 0 holds one layer of 256 bricks (one per column) with a second layer of 16 below
it, supercells 1 and 2 hold 3 and 5 bricks, supercell 3 is empty."""
import numpy as np
import pytest

from _edit_model import LOADED, assert_device_world

pytestmark = pytest.mark.gpu

G, H = 256, 128
LAYER_Z, LOWER_Z = 44, 20  # voxel heights of the two layers of supercell 0: brick cells z = 5 and z = 2
START = 16                 # bricks of a starting pool


def make_volume():
    v = np.zeros((H, G, G), np.uint8)
    v[LAYER_Z, 0:128, 0:128] = 1       # supercell 0: a brick in every one of its 16 x 16 columns
    v[LOWER_Z, 0:8, 0:128] = 1         # ... and a second one below it in the columns y = 0
    v[3, 5, 130:150] = 1               # supercell 1: 3 bricks
    v[100, 140:176, 7] = 1             # supercell 2: 5 bricks
    return v


@pytest.fixture(scope="module")
def volume():
    return make_volume()


def streaming_scene(bm, volume, overlapped):
    scene = bm.Scene.from_voxels(volume).reset_residency().set_streaming_mode(overlapped)
    info = scene.info()
    assert info["supercells"] == 4 and info["resident_bricks"] == 0 and info["total_bricks"] == 256 + 16 + 3 + 5
    assert info["pool_bytes"] == 3 * START * 64
    return scene


def request(scene, columns):
    """one ray straight down the middle of each brick column (cx, cy): it ends at the column's topmost brick, which is requested if it is not resident"""
    c = np.asarray(columns, np.float32).reshape(-1, 2)
    origins = np.concatenate([c * 8 + 4.5, np.full((len(c), 1), H - 0.5, np.float32)], 1).astype(np.float32)
    directions = np.tile(np.array([0, 0, -1], np.float32), (len(c), 1))
    return scene.cast_rays(origins, directions)


def service(scene, overlapped):
    """the call that services what has been requested: in overlapped mode the first call only copies the ring out"""
    if overlapped:
        assert scene.process_load_queue() == 0
    return scene.process_load_queue()


def layer_columns(n=256):
    return [(i % 16, i // 16) for i in range(n)]


def loaded_slots(scene, sc):
    w = scene.device_indices(sc)
    return w, np.sort(w[(w & np.uint32(LOADED)) != 0] & np.uint32(0xFFF))


@pytest.mark.parametrize("overlapped", [0, 1], ids=["blocking", "overlapped"])
def test_one_batch_of_256_requests_for_one_supercell(overlapped, bm, volume):
    scene = streaming_scene(bm, volume, overlapped)
    request(scene, layer_columns())
    assert service(scene, overlapped) == 256
    assert assert_device_world(scene, volume) == 256
    _, slots = loaded_slots(scene, 0)
    assert np.array_equal(slots, np.arange(256)), "the supercell's device slots are not a permutation of 0 ... 255"
    info = scene.info()
    assert info["resident_bricks"] == 256 and info["failed"] == 0
    assert info["pool_bytes"] == (256 + 2 * START) * 64, "the pools: supercell 0 grown to 256 bricks, two starting pools"
    assert info["stream_batches"] == 1


@pytest.mark.parametrize("overlapped", [0, 1], ids=["blocking", "overlapped"])
def test_requests_whose_bricks_an_edit_cleared_are_not_serviced(overlapped, bm, volume):
    scene = streaming_scene(bm, volume, overlapped)
    model = volume.copy()
    request(scene, layer_columns())
    if overlapped:
        assert scene.process_load_queue() == 0  # the ring is copied out with all 256 entries
    scene.clear_box((0, 0, LAYER_Z), (64, 128, LAYER_Z + 1))  # the layer's bricks of the columns x < 8
    model[LAYER_Z, 0:128, 0:64] = 0
    assert scene.process_load_queue() == 128
    assert assert_device_world(scene, model) == 128
    info = scene.info()
    assert info["resident_bricks"] == 128 and info["failed"] == 0
    assert info["pool_bytes"] == (128 + 2 * START) * 64


def test_a_freed_slot_goes_to_the_next_brick_of_the_supercell(bm, volume):
    scene = streaming_scene(bm, volume, 0)
    model = volume.copy()
    request(scene, layer_columns(32))
    assert scene.process_load_queue() == 32
    before = scene.info()["pool_bytes"]
    assert before == (32 + 2 * START) * 64
    w, slots = loaded_slots(scene, 0)
    assert np.array_equal(slots, np.arange(32))
    cell = 5 * 256 + 0 * 16 + 7  # the layer's brick of column (7, 0)
    freed = int(w[cell] & np.uint32(0xFFF))
    scene.clear_box((56, 0, LAYER_Z), (64, 8, LAYER_Z + 1))
    model[LAYER_Z, 0:8, 56:64] = 0
    assert scene.info()["resident_bricks"] == 31
    request(scene, [(3, 9)])  # a column that was not requested before
    assert scene.process_load_queue() == 1
    w, slots = loaded_slots(scene, 0)
    taken = 5 * 256 + 9 * 16 + 3
    assert (w[taken] & np.uint32(LOADED)) and int(w[taken] & np.uint32(0xFFF)) == freed, "the new brick did not take the freed slot"
    assert np.array_equal(slots, np.arange(32))
    assert assert_device_world(scene, model) == 32
    assert scene.info()["pool_bytes"] == before and scene.info()["failed"] == 0
    # the column whose upper brick went now ends at its lower one
    request(scene, [(7, 0)])
    assert scene.process_load_queue() == 1
    assert assert_device_world(scene, model) == 33


def test_a_change_of_mode_loses_no_request(bm, volume):
    scene = streaming_scene(bm, volume, 1)
    a, b, c = layer_columns(192)[:64], layer_columns(192)[64:128], layer_columns(192)[128:]
    request(scene, a)
    assert scene.process_load_queue() == 0  # ring 0 is being copied out: a snapshot is pending
    scene.set_streaming_mode(0)             # ... and is serviced by the switch
    assert scene.info()["resident_bricks"] == 64
    assert assert_device_world(scene, volume) == 64
    # again, with ring 1 the current ring
    scene.set_streaming_mode(1)
    request(scene, b)
    assert scene.process_load_queue() == 0  # ring 0 copied out, frames append to ring 1 from here on
    request(scene, c)
    scene.set_streaming_mode(0)             # b is serviced, c is carried over to ring 0
    assert scene.info()["resident_bricks"] == 128
    assert scene.process_load_queue() == 64
    assert assert_device_world(scene, volume) == 192
    info = scene.info()
    assert info["resident_bricks"] == 192 and info["failed"] == 0 and info["pool_bytes"] == (256 + 2 * START) * 64
    assert scene.process_load_queue() == 0


def test_reset_after_preload_and_edits(bm, volume):
    scene = bm.Scene.from_voxels(volume)
    model = volume.copy()
    scene.preload_all()
    assert scene.info()["resident_bricks"] == 280 and scene.info()["pool_bytes"] == 280 * 64
    scene.fill_box((200, 200, 64), (202, 202, 66))  # supercell 3 gets its first brick
    model[64:66, 200:202, 200:202] = 1
    scene.clear_box((0, 0, LAYER_Z), (16, 128, LAYER_Z + 1))  # 32 bricks of the layer go
    model[LAYER_Z, 0:128, 0:16] = 0
    scene.fill_box((0, 0, 120), (128, 8, 121))  # 16 new bricks at the top of supercell 0: they take freed slots
    model[120, 0:8, 0:128] = 1
    assert assert_device_world(scene, model) == 280 + 1 - 32 + 16
    assert scene.info()["pool_bytes"] == (280 + START) * 64
    scene.reset_residency()
    assert assert_device_world(scene, model) == 0, "a reset leaves a brick loaded"
    info = scene.info()
    assert info["resident_bricks"] == 0 and info["failed"] == 0
    assert info["pool_bytes"] == 4 * START * 64, "one starting pool per supercell that holds bricks"
    assert info["stream_batches"] == 0
    # and it streams from there
    request(scene, [(25, 25)])
    assert scene.process_load_queue() == 1
    assert assert_device_world(scene, model) == 1
