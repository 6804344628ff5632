"""brickmap_amd.settle on the MI355X (csrc/settle.hip): the device's volume, drops and record must equal bm_host_settle's -- the host routine
that tests/test_settle_host.py pins to the numpy model -- byte for byte, on the cases of tests/_settle_model.py: the smallest shapes at
which each part can go wrong (columns that are no multiple of a wave, waves that span rows, heights around the slices in flight, more
rounds than two batches, column groups that return early, tables that miss labels).  Then a live scene: a pillar cut through comes down
and lands.  Every number is an integer, every comparison exact."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

import _settle_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
RULES = open(os.path.join(ROOT, "brickmap_amd", "csrc", "settle.h")).read()
BATCH = int(re.search(r"kSettleBatch = (\d+);", RULES).group(1))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def st(bm):
    from brickmap_amd import settle
    return settle


@pytest.fixture(scope="module")
def scene(bm, torch_cuda):
    """an empty world of 128^3 voxels, the smallest there is"""
    s = bm.Scene.from_voxels(np.zeros((128, 128, 128), np.uint8))
    yield s
    s.close()


@pytest.fixture(scope="module", autouse=True)
def report_time():
    t0 = time.time()
    yield
    print(f"tests/test_gpu_settle.py took {time.time() - t0:.1f} s")


def on_device(torch, st, scene, labels, records, chosen, **kw):
    return st.settle_volume(scene, torch.from_numpy(np.ascontiguousarray(labels)).cuda(), records, chosen, **kw)


@pytest.mark.parametrize("name", model.NAMES)
def test_device_equals_the_host_routine(name, bm, st, torch_cuda, scene):
    labels, records, chosen, want = model.cases(bm)[name]
    out, drops, rec = st.host_settle(labels, records, chosen)
    got = on_device(torch_cuda, st, scene, labels, records, chosen)
    d_out = got.out.cpu().numpy()
    print(name, "host", rec, "device", got.record)
    assert d_out.dtype == np.uint8 and d_out.shape == labels.shape
    assert d_out.tobytes() == out.tobytes(), f"first difference at {np.argmax(d_out.ravel() != out.ravel())}"
    assert got.drops.dtype == np.int32 and got.drops.tobytes() == drops.tobytes()
    assert got.record.tobytes() == rec.tobytes(), (got.record, rec)
    if want is not None:
        assert got.drops[chosen != 0].tolist() == want
    if name == "two interlocked pieces":
        assert d_out.tobytes() == model.INTERLOCKED_OUT.tobytes()
    if name in ("n = 0", "chosen all zero"):
        assert np.array_equal(d_out, (labels != 0).astype(np.uint8)) and not got.drops.any()


def test_more_rounds_than_two_batches(bm, st, torch_cuda, scene):
    """the staircase settles one piece per round (tests/_settle_model.py says why): 20 rounds and the one that changes nothing.  Fewer
    cannot be, whatever a read sees; more than chosen + 2 = 22 the call itself refuses to run."""
    labels, records, chosen, want = model.cases(bm)["a staircase of 20 pieces"]
    d_labels = torch_cuda.from_numpy(labels).cuda()
    for batch in (0, 1, 3, 16):
        got, (ms, rounds, looks) = st.settle_times(scene, d_labels, records, chosen, batch=batch)
        b = batch or BATCH
        print(f"batch {b}: {rounds} rounds, {looks} looks, {ms} ms")
        assert got.drops[1:].tolist() == want and got.largest_drop == 20 and int(got.record["contacts"]) == 20 + 19
        assert 21 <= rounds <= 22 and rounds > 2 * BATCH and looks == -(-rounds // b) and len(ms) == 3


def test_two_runs_and_a_side_stream_give_the_same_bytes(bm, st, torch_cuda, scene):
    """the labels are written on the current stream just before the call on a side stream, which must see them"""
    torch = torch_cuda
    labels, records, chosen, _ = model.cases(bm)["70 x 17 x 33 at density 0.15"]
    out, drops, rec = st.host_settle(labels, records, chosen)
    a = on_device(torch, st, scene, labels, records, chosen)
    side = torch.cuda.Stream()
    staged = torch.from_numpy(labels).cuda()
    d_labels = torch.zeros_like(staged)
    big = torch.ones((4096, 4096), device="cuda")
    for _ in range(4):
        big = big @ big * 1e-4   # work in front of the copy on the producer's stream
    d_labels.copy_(staged)
    b = st.settle_volume(scene, d_labels, records, chosen, stream=side.cuda_stream)
    assert a.out.data_ptr() != b.out.data_ptr()
    assert a.out.cpu().numpy().tobytes() == b.out.cpu().numpy().tobytes() == out.tobytes()
    assert a.drops.tobytes() == b.drops.tobytes() == drops.tobytes() and a.record.tobytes() == b.record.tobytes() == rec.tobytes()


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_buffers_untouched(bm, st, torch_cuda, scene):
    torch = torch_cuda
    L = scene._L
    shape = (6, 5, 9)
    labels, records, chosen, _ = model.cases(bm)["height 7"]
    labels = labels[:6]
    n = len(records)
    d_labels = torch.from_numpy(np.ascontiguousarray(labels)).cuda()
    d_records = torch.from_numpy(records.view(np.int64).copy()).cuda()
    d_chosen = torch.from_numpy(chosen).cuda()
    need = st.settle_workspace_bytes(n, shape)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    out = torch.full(shape, 7, dtype=torch.uint8, device="cuda")
    drops = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")

    def call(extent=(9, 5, 6), l=d_labels.data_ptr(), r=d_records.data_ptr(), n=n, c=d_chosen.data_ptr(), o=out.data_ptr(), d=drops.data_ptr(), s=res.data_ptr(),
             w=ws.data_ptr(), wb=need, flags=0):
        return L.bm_settle(scene.gpuScene, (C.c_int32 * 3)(*extent) if extent else None, C.c_void_p(l), C.c_void_p(r), n, C.c_void_p(c), C.c_void_p(o), C.c_void_p(d),
                           C.c_void_p(s), C.c_void_p(w), wb, flags, None)

    def fired(fragment):
        msg = L.bm_last_error_string()
        return msg.startswith(b"bm_settle: ") and fragment in msg

    extent, null, aligned, overlaps = b"an extent below 1 or above 16384", b"null", b"aligned", b"overlaps"
    bad = [(dict(extent=None), null), (dict(extent=(0, 5, 6)), extent), (dict(extent=(9, 5, 16385)), extent), (dict(extent=(16384, 16384, 8)), b"more than 2^31 - 2 voxels"),
           (dict(flags=1), b"unknown flag"), (dict(n=-1), b"a negative number of records"), (dict(l=0), null), (dict(r=0), null), (dict(c=0), null), (dict(o=0), null),
           (dict(d=0), null), (dict(s=0), null), (dict(w=0), null), (dict(l=d_labels.data_ptr() + 2), aligned), (dict(d=drops.data_ptr() + 2), aligned),
           (dict(w=ws.data_ptr() + 2), aligned), (dict(r=d_records.data_ptr() + 4), aligned), (dict(s=res.data_ptr() + 4), aligned), (dict(wb=need - 1), b"smaller than"),
           (dict(o=d_labels.data_ptr() + 4), b"out overlaps labels"), (dict(w=d_labels.data_ptr()), overlaps), (dict(o=ws.data_ptr() + 8), overlaps),
           (dict(d=ws.data_ptr()), overlaps), (dict(s=ws.data_ptr() + need - 32), overlaps), (dict(c=ws.data_ptr() + 16), overlaps), (dict(r=ws.data_ptr()), overlaps)]
    for kw, fragment in bad:
        assert call(**kw) == EINVAL, kw
        assert fired(fragment), (kw, L.bm_last_error_string())
    own = C.c_void_p()   # an allocation of 512 bytes of its own: torch's tensors share theirs
    assert L.bm_buffer_alloc(scene.device, 512, C.byref(own)) == 0
    for kw in (dict(l=own.value), dict(o=own.value + 400), dict(r=own.value + 480), dict(w=own.value + 508)):
        assert call(**kw) == EINVAL and fired(b"does not lie inside"), (kw, L.bm_last_error_string())
    torch.cuda.synchronize()
    assert (out == 7).all().item() and (drops == -5).all().item() and not res.any().item() and not ws.any().item(), "nothing is launched and nothing written"
    assert L.bm_synchronize(scene.gpuScene) == 0 and L.bm_buffer_free(scene.device, own) == 0
    assert L.bm_debug_settle_times(scene.gpuScene, None, None, None, 0, None, None, None, None, None, 0, 0, None, 0, None, None) == EINVAL
    # a workspace that is only 4-byte aligned serves, and the call has waited when it returns
    want_out, want_drops, want_rec = st.host_settle(np.ascontiguousarray(labels), records, chosen)
    assert call(w=ws.data_ptr() + 4) == 0, L.bm_last_error_string()
    assert out.cpu().numpy().tobytes() == want_out.tobytes() and drops.cpu().numpy().tobytes() == want_drops.tobytes()
    assert res.cpu().numpy().tobytes() == want_rec.tobytes()
    assert call(n=0, r=0, c=0, d=0) == 0 and np.array_equal(out.cpu().numpy(), (labels != 0).astype(np.uint8))
    for bad_labels in (labels, d_labels.to(torch.int64), d_labels[:, :, ::2]):
        with pytest.raises(ValueError):
            st.settle_volume(scene, bad_labels, records, chosen)
    with pytest.raises(ValueError):
        st.settle_volume(scene, d_labels, records, chosen[:-1])


# ---------------------------------------------------------------- a live scene
def pillar_world():
    """128^3: ground two voxels thick, a pillar 4 x 4 from the ground to z = 40 with a slab on top, cut through between z = 10 and z = 16"""
    v = np.zeros((128, 128, 128), np.uint8)
    v[0:2] = 1
    v[2:40, 30:34, 30:34] = 1
    v[40:42, 26:38, 26:38] = 1
    v[10:16, 30:34, 30:34] = 0
    return v


def test_a_pillar_cut_through_comes_down_and_lands(bm, st, torch_cuda):
    vox = pillar_world()
    scene = bm.Scene.from_voxels(vox)
    try:
        lo, hi = (20, 20, 0), (44, 44, 50)
        before = scene.read_region(lo, hi)
        comps = scene.components(lo, hi)
        assert int(comps.loose().sum()) == 1
        pieces, voxels, largest = st.settle_floating(scene, lo, hi)
        top = vox[16:42].sum()
        assert (pieces, voxels, largest) == (1, int(top), 6)
        want = vox.copy()
        want[10:36] = vox[16:42]
        want[36:42] = 0
        after = scene.read_region((0, 0, 0), (128, 128, 128))
        assert np.array_equal(after, want != 0), "the top rests on the stump"
        assert int(after.sum()) == int(vox.sum()) and int(scene.read_region(lo, hi).sum()) == int(before.sum())
        assert not scene.components(lo, hi).loose().any()
        assert st.settle_floating(scene, lo, hi) == (0, 0, 0)
        assert np.array_equal(scene.read_region((0, 0, 0), (128, 128, 128)), want != 0)
        # a piece on an anchor face does not move: the lower part of the pillar is held by the bottom of a box that begins at z = 12
        scene.clear_box((30, 30, 20), (34, 34, 24))
        assert st.settle_floating(scene, (20, 20, 12), (44, 44, 50)) == (1, int(want[24:].sum()), 4)
        assert st.settle_floating(scene, (26, 26, 0), (38, 38, 50), anchor=("-z",)) == (0, 0, 0), "what stands on the ground is held by -z"
        # the floor is the bottom of the box: a cube in the air lands on the lowest slice of a box that ends above the ground
        scene.fill_box((5, 5, 40), (8, 8, 43))
        assert st.settle_floating(scene, (2, 2, 30), (12, 12, 50)) == (1, 27, 10)
        assert scene.read_region((5, 5, 30), (8, 8, 33)).all() and int(scene.read_region((2, 2, 2), (12, 12, 64)).sum()) == 27
    finally:
        scene.close()


def test_headless_main_settles_like_the_host_routine(bm, st, torch_cuda, tmp_path):
    """examples/headless_main --settle x0,y0,z0:x1,y1,z1 (C++ Scene::settle_floating): the numbers it prints are the host routine's"""
    exe = os.path.join(ROOT, "examples", "headless_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    vox = pillar_world()
    vox[45:47, 28:30, 28:36] = 1   # a second loose piece above the slab
    world = tmp_path / "world.raw"
    vox.tofile(world)
    r = subprocess.run([exe, "--voxels", str(world), "--settle", "20,20,0:44,44,50", "128", "128", "64", "48", "1", str(tmp_path / "frame.ppm")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    labels, records = model.label_and_table(bm, vox[0:50, 20:44, 20:44])
    _, _, rec = st.host_settle(labels, records, model.loose(records))
    m = re.search(r"settled (\d+) floating pieces, (\d+) voxels, largest drop (\d+)", r.stdout)
    assert m and [int(v) for v in m.groups()] == [int(rec["moved_pieces"]), int(rec["moved_voxels"]), int(rec["largest_drop"])] == [2, int(vox[16:].sum()), 9], r.stdout
    r = subprocess.run([exe, "--settle", "1,2,3", "128", "128", "64", "48", "1", str(tmp_path / "frame.ppm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--settle wants" in r.stderr
