"""Frame groups: a UNIFORM bm_render_frames launch of production frames hands its frames out F at a time, as (chunk, pixel part, frame)
items (csrc/trace.hip "FRAME GROUPS", frame_plan.cpp ring_group_of; F = 4, BM_RING_GROUP overrides it).  Who sits next to whom in a wave
changes, what a path computes does not: K frames of one launch are the same K frames as K single launches -- terminated-path counts,
traversal counters and ray digests exactly, radiance up to the order of the float-atomic additions.

One hit-record buffer shared by the frames of a launch holds the digest of the WHOLE launch (include/brickmap.h, bm_render_frames): a
ray's hash in words 4 and 5 is keyed with its sample counted from the FIRST frame's sample_base, so frame k's rays carry the key k where
a single launch of frame k keys them 0.  Words 6 and 7 (ray and cell counts) have no key and are the sums of the K single launches'
records; words 4 and 5 are, by that contract, those of ONE single launch of the K-sample frame at the first frame's sample_base -- the
same rays under the same keys -- and that single launch is the reference for them (its own words 6 and 7 must be the K launches' sums).

Shape: one superchunk (128^3, resident), 72 x 40 pixels (partial 16 x 16 tiles in x and y), 4 segments, 1 spp; K = 1, 3, 4, 5, 9 frames:
under one group, exactly one, one and a remainder, two and a remainder."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, W, H, MB, BASE = 128, 72, 40, 3, 3
KS = (1, 3, 4, 5, 9)
RGB_TOL = 1e-5  # of the frame's largest value: the paths are bit-identical, only the order of the additions differs (bench.py --verify's bar)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def scene(bm, torch_cuda):
    s = bm.Scene(G, G, device=0).generate()
    s.preload_all()
    yield s
    s.close()


@pytest.fixture(scope="module")
def cam(bm):
    return bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()


def frame(bm, k, flags=0):
    return bm.FrameParams(W, H, spp=1, sample_base=BASE + k, max_bounces=MB, flags=flags)


def zeros(torch, *shape, dtype=None):
    return torch.zeros(shape, dtype=dtype or torch.float32, device="cuda:0")


@pytest.fixture(scope="module")
def singles(bm, torch_cuda, scene, cam):
    """The reference, computed once: frames 0 ... 8 as SINGLE launches -- each into a buffer of its own, and one after the other into one
    buffer (a snapshot after every frame); then the same frames with the instrumented kernel (ray digest and counters, frame by frame)."""
    torch = torch_cuda
    assert bm.frame_plan(frame(bm, 0))["ring_group"] == 4 and not bm.tuning_overrides(), "these tests pin the product's own rule"
    n = max(KS)
    own, summed, running = [], [], zeros(torch, H, W, 4)
    for k in range(n):
        a = zeros(torch, H, W, 4)
        scene.render(cam, frame(bm, k), a)
        scene.render(cam, frame(bm, k), running)
        torch.cuda.synchronize()
        own.append(a.cpu().numpy())
        summed.append(running.cpu().numpy().copy())
    flags = bm.BM_FLAG_RAY_DIGEST | bm.BM_FLAG_COUNTERS
    digests, counters = [], []
    for k in range(n):
        a, d = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32)
        scene.counters_reset()
        scene.render(cam, frame(bm, k, flags), a, debug=d)
        torch.cuda.synchronize()
        counters.append(scene.counters())
        digests.append(d.cpu().numpy().view(np.uint32))
    scene.counters_reset()
    assert len(counters[0]) == 8 and any(counters[0].values())
    return dict(own=own, summed=summed, digests=digests, counters=counters, launch_digest={K: launch_digest(bm, torch, scene, cam, digests, K) for K in KS})


def launch_digest(bm, torch, scene, cam, digests, K):
    """Words 4-7 that ONE hit-record buffer shared by frames 0 ... K - 1 must hold (module docstring).  Words 6 and 7: the sums mod 2^32
    of the K single launches' records.  Words 4 and 5: of a SINGLE launch of the K-sample frame at the first frame's sample_base, whose
    rays are those of the K frames (its words 6 and 7 are checked to be the same sums) under the keys the shared buffer gives them."""
    want = np.zeros((H, W, 4), dtype=np.uint32)
    for k in range(K):
        want += digests[k][..., 4:8]  # (uint32: wraps mod 2^32)
    a, d = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32)
    scene.render(cam, bm.FrameParams(W, H, spp=K, sample_base=BASE, max_bounces=MB, flags=bm.BM_FLAG_RAY_DIGEST), a, debug=d)
    torch.cuda.synchronize()
    one = d.cpu().numpy().view(np.uint32)[..., 4:8]
    assert np.array_equal(one[..., 2:], want[..., 2:]), f"the {K}-sample frame does not trace the rays of the {K} frames"
    if K == 1:
        assert np.array_equal(one, want)  # (one frame: its keys are the single launch's)
    want[..., :2] = one[..., :2]
    return want


def assert_same_frame(got, want, what):
    err = float(np.abs(got[..., :3] - want[..., :3]).max())
    bound = RGB_TOL * float(np.abs(want[..., :3]).max())
    print(f"{what}: max |rgb difference| {err:.3e}, bound {bound:.3e}")
    assert np.array_equal(got[..., 3], want[..., 3]), f"{what}: terminated-path counts differ"
    assert err <= bound, f"{what}: rgb differs by {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("K", KS)
def test_grouped_frames_are_the_single_launches(K, bm, torch_cuda, scene, cam, singles):
    """K production frames as ONE launch, into one shared accumulation buffer (pixel stride 0) and into K slots of one allocation
    (pixel stride = a frame): per pixel and per slot the terminated-path counts of the single launches, rgb within 1e-5."""
    torch = torch_cuda
    params = [frame(bm, k) for k in range(K)]
    shared = zeros(torch, H, W, 4)
    scene.render_frames(cam, params, shared)
    slots = zeros(torch, K, H, W, 4)
    scene.render_frames(cam, params, [slots[k] for k in range(K)])
    torch.cuda.synchronize()
    assert np.all(singles["summed"][K - 1][..., 3] == K)
    assert_same_frame(shared.cpu().numpy(), singles["summed"][K - 1], f"K = {K}, shared buffer")
    got = slots.cpu().numpy()
    for k in range(K):
        assert_same_frame(got[k], singles["own"][k], f"K = {K}, slot {k}")


@pytest.mark.parametrize("K", KS)
def test_instrumented_sibling_walks_the_same_rays(K, bm, torch_cuda, scene, cam, singles):
    """The same launches with trace_paths<true, *, true, 2> (BM_FLAG_RAY_DIGEST | BM_FLAG_COUNTERS; the hand-out of the timed kernel): the
    eight traversal counters are the sums over the single launches, and words 4-7 of the shared hit-record buffer are those of the
    single launches (launch_digest: counts summed, hashes under the launch's keys); slots with record buffers of their own equal the
    single launches' frame by frame."""
    torch = torch_cuda
    flags = bm.BM_FLAG_RAY_DIGEST | bm.BM_FLAG_COUNTERS
    params = [frame(bm, k, flags) for k in range(K)]
    want_counters = {name: sum(singles["counters"][k][name] for k in range(K)) for name in singles["counters"][0]}
    want_digest = singles["launch_digest"][K]
    acc, dig = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32)
    scene.counters_reset()
    scene.render_frames(cam, params, acc, debugs=[dig] * K)
    torch.cuda.synchronize()
    got_counters = scene.counters()
    scene.counters_reset()
    assert got_counters == want_counters
    assert np.array_equal(dig.cpu().numpy().view(np.uint32)[..., 4:8], want_digest), "shared hit-record buffer: not the digest of the single launches"
    assert_same_frame(acc.cpu().numpy(), singles["summed"][K - 1], f"K = {K}, instrumented, shared buffer")
    # K slots, a record buffer each
    slots, digs = zeros(torch, K, H, W, 4), [zeros(torch, H, W, 8, dtype=torch.int32) for _ in range(K)]
    scene.render_frames(cam, params, [slots[k] for k in range(K)], debugs=digs)
    torch.cuda.synchronize()
    got_counters = scene.counters()
    scene.counters_reset()
    assert got_counters == want_counters
    for k in range(K):
        assert np.array_equal(digs[k].cpu().numpy().view(np.uint32)[..., 4:8], singles["digests"][k][..., 4:8]), f"slot {k}: ray digest differs"
        assert_same_frame(slots[k].cpu().numpy(), singles["own"][k], f"K = {K}, instrumented, slot {k}")


GROUP_SCRIPT = r'''
import json, sys
sys.path.insert(0, %r)
import numpy as np, torch, brickmap_amd as bm
G, W, H, MB, BASE, K = %d, %d, %d, %d, %d, 9
scene = bm.Scene(G, G, device=0).generate().preload_all()
cam = bm.Camera(position=(G / 2, G / 8, 0.8 * G), horizontal_angle=0.8, vertical_angle=-0.5).update()
flags = bm.BM_FLAG_RAY_DIGEST | bm.BM_FLAG_COUNTERS
shared = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
slots = torch.zeros((K, H, W, 4), dtype=torch.float32, device="cuda:0")
scene.render_frames(cam, [bm.FrameParams(W, H, spp=1, sample_base=BASE + k, max_bounces=MB) for k in range(K)], shared)
scene.render_frames(cam, [bm.FrameParams(W, H, spp=1, sample_base=BASE + k, max_bounces=MB) for k in range(K)], [slots[k] for k in range(K)])
acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
dig = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda:0")
scene.counters_reset()
scene.render_frames(cam, [bm.FrameParams(W, H, spp=1, sample_base=BASE + k, max_bounces=MB, flags=flags) for k in range(K)], acc, debugs=[dig] * K)
torch.cuda.synchronize()
np.savez(sys.argv[1], shared=shared.cpu().numpy(), slots=slots.cpu().numpy(), acc=acc.cpu().numpy(), dig=dig.cpu().numpy())
print("RESULT", json.dumps(dict(counters=scene.counters(), overrides=bm.tuning_overrides(), group=bm.frame_plan(bm.FrameParams(W, H, spp=1, max_bounces=MB))["ring_group"])))
''' % (ROOT, G, W, H, MB, BASE)


def test_group_size_changes_nothing_but_time(bm, torch_cuda, singles, tmp_path):
    """BM_RING_GROUP = 1 (frame after frame: the hand-out before there were groups), 2 and 8 (9 frames: a group and one frame) against
    the single launches of this process: the same counts, counters and digests, rgb within the bound."""
    K = 9
    want_counters = {name: sum(singles["counters"][k][name] for k in range(K)) for name in singles["counters"][0]}
    want_digest = singles["launch_digest"][K]
    for group in (1, 2, 8):
        out = str(tmp_path / f"group{group}.npz")
        r = subprocess.run([sys.executable, "-c", GROUP_SCRIPT, out], env=dict(os.environ, BM_RING_GROUP=str(group)), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][7:])
        assert res["overrides"] == {"BM_RING_GROUP": group} and res["group"] == group
        assert res["counters"] == want_counters
        data = np.load(out)
        assert np.array_equal(data["dig"].view(np.uint32)[..., 4:8], want_digest)
        assert_same_frame(data["shared"], singles["summed"][K - 1], f"BM_RING_GROUP={group}, shared buffer")
        assert_same_frame(data["acc"], singles["summed"][K - 1], f"BM_RING_GROUP={group}, instrumented")
        for k in range(K):
            assert_same_frame(data["slots"][k], singles["own"][k], f"BM_RING_GROUP={group}, slot {k}")


def test_shared_digest_that_would_overflow_is_refused(bm, torch_cuda, scene, cam):
    """One hit-record buffer for all frames of a launch counts the pixel's rays of the WHOLE launch in 16 bits and keys them with 24
    bits of sample index: a launch past either is refused, not rendered (each frame alone is inside the per-frame limits)."""
    torch = torch_cuda
    acc, dig = zeros(torch, H, W, 4), zeros(torch, H, W, 8, dtype=torch.int32)
    rays = [bm.FrameParams(W, H, spp=8192, sample_base=8192 * k, max_bounces=3, flags=bm.BM_FLAG_RAY_DIGEST) for k in range(2)]  # 2 x 8192 x 4 = 65536
    with pytest.raises(bm.BrickmapError, match="65536"):
        scene.render_frames(cam, rays, acc, debugs=[dig] * 2)
    keys = [bm.FrameParams(W, H, spp=1, sample_base=(1 << 17) * k, max_bounces=3, flags=bm.BM_FLAG_RAY_DIGEST) for k in range(129)]  # 2^17 x 128 + 1 > 2^24
    with pytest.raises(bm.BrickmapError, match="2\\^24"):
        scene.render_frames(cam, keys, acc, debugs=[dig] * 129)
    torch.cuda.synchronize()
    assert not acc.any() and not dig.any()
    scene.render_frames(cam, keys[:128], acc, debugs=[dig] * 128)  # 2^17 x 127 + 1 < 2^24, 128 x 4 rays: inside both
    torch.cuda.synchronize()
    assert torch.all(acc[..., 3] == 128)
