"""bm_launch_plan_of -- the plan of a bm_render_frames launch (csrc/frame_plan.cpp plan_launch), host only: which ring mode the launch
gets, how its frames are grouped, how many ticket-counter blocks and workgroups it takes, and every refusal with its message.  The
buffers are made-up addresses: the plan compares and subtracts them and never reads them.  Every expected value is worked out by
hand from the rules (a 64 x 48 frame is 4 x 3 tiles of 16 x 16 pixels = 3072 pixels, a 49 152-byte image, 98 304 bytes of hit records)."""
import ctypes as C
import dataclasses

import pytest

import brickmap_amd as bm
from brickmap_amd import _lib

W, H = 64, 48
PIXELS = W * H
IMAGE, RECORDS = PIXELS * 16, PIXELS * 32
A, D = 0x7F0000000000, 0x7E0000000000  # accumulation / hit-record buffers, 16-byte aligned
LONE = 12  # workgroups of one frame: ceil(12 tiles x 16 chunks x 16 pixels / 256)
CAM = bm.Camera(position=(128.0, 32.0, 205.0), horizontal_angle=0.8, vertical_angle=-0.5).update()
CAM2 = bm.Camera(position=(137.0, 37.0, 202.0), horizontal_angle=0.87, vertical_angle=-0.53).update()


@pytest.fixture(autouse=True)
def own_rules():
    assert not bm.tuning_overrides(), "these tests pin the product's own rules"


def frames(n, step=1, **kw):
    kw.setdefault("max_bounces", 3)
    spp = kw.pop("spp", 1)
    return [bm.FrameParams(W, H, spp=spp, sample_base=step * k, **kw) for k in range(n)]


def images(n, stride=IMAGE, base=A):
    return [base + stride * k for k in range(n)]


def test_one_frame():
    assert bm.launch_plan(CAM, frames(1), A) == dict(ring_mode=0, ring_group=1, sample_stride=0, pixel_stride=0, shared_digest=0, instrumented=0,
                                                    counter_blocks=1, refill_min=24, workgroups=LONE)
    one = bm.launch_plan(CAM, frames(1), A, [D])  # hit records in path order: the ordered, instrumented frame
    assert (one["ring_mode"], one["instrumented"], one["refill_min"], one["workgroups"]) == (0, 1, 16, LONE)


@pytest.mark.parametrize("count, group, blocks", [(2, 2, 1), (3, 3, 1), (4, 4, 1), (5, 4, 2), (20, 4, 5), (256, 4, 64)])
def test_production_frames_into_one_buffer_are_a_grouped_uniform_ring(count, group, blocks):
    assert bm.launch_plan(CAM, frames(count), A) == dict(ring_mode=2, ring_group=group, sample_stride=1, pixel_stride=0, shared_digest=0, instrumented=0,
                                                        counter_blocks=blocks, refill_min=32, workgroups=2 * LONE)


def test_uniform_launches_step_by_constants():
    stepping = bm.launch_plan(CAM, frames(20), images(20))  # one allocation, image after image
    assert (stepping["ring_mode"], stepping["pixel_stride"], stepping["sample_stride"], stepping["ring_group"], stepping["counter_blocks"]) == (2, PIXELS, 1, 4, 5)
    wide = bm.launch_plan(CAM, frames(3, step=7), images(3, stride=IMAGE + 160))
    assert (wide["ring_mode"], wide["pixel_stride"], wide["sample_stride"]) == (2, PIXELS + 10, 7)
    resting = bm.launch_plan(CAM, frames(3, step=0), A)  # equal sample_base in all frames: a stride of 0
    assert (resting["ring_mode"], resting["sample_stride"], resting["ring_group"]) == (2, 0, 3)
    assert bm.launch_plan([CAM] * 3, frames(3), [A] * 3) == bm.launch_plan(CAM, frames(3), A)  # (one camera / buffer or one per frame: the same call)


def plain_ring(plan, count, instrumented=0):
    assert plan == dict(ring_mode=1, ring_group=1, sample_stride=0, pixel_stride=0, shared_digest=0, instrumented=instrumented, counter_blocks=count,
                        refill_min=16 if instrumented else 32, workgroups=2 * LONE)


def test_what_alone_makes_a_launch_a_plain_ring():
    fs = frames(3)
    plain_ring(bm.launch_plan([CAM, CAM, CAM2], fs, A), 3)  # a second camera
    plain_ring(bm.launch_plan(CAM, fs[:2] + [dataclasses.replace(fs[2], sun_position=(0.05, 0.2))], A), 3)  # another sun
    plain_ring(bm.launch_plan(CAM, fs[:2] + [dataclasses.replace(fs[2], base_frame=2)], A), 3)  # another seed
    plain_ring(bm.launch_plan(CAM, fs[::-1], A), 3)  # sample_base falls
    plain_ring(bm.launch_plan(CAM, [fs[0], fs[1], dataclasses.replace(fs[2], sample_base=3)], A), 3)  # ... steps by 1, then by 2
    plain_ring(bm.launch_plan(CAM, fs, [A, A + IMAGE, A + 3 * IMAGE]), 3)  # buffers step by one image, then by two
    plain_ring(bm.launch_plan(CAM, fs, images(3, stride=IMAGE + 8)), 3)  # a buffer stride that is no multiple of a pixel's 16 bytes
    plain_ring(bm.launch_plan(CAM, fs, images(3)[::-1]), 3)  # buffers step backwards
    # hit records in path order (no BM_FLAG_RAY_DIGEST): ordered frames, buffers of their own, never uniform
    plain_ring(bm.launch_plan(CAM, fs, images(3), images(3, RECORDS, D)), 3, instrumented=1)
    plain_ring(bm.launch_plan(CAM, fs, images(3), [None, D, None]), 3, instrumented=1)  # ... one frame with records makes all frames ordered


def test_ordered_frames_of_one_view_are_a_uniform_ring_frame_after_frame():
    for count in (2, 7):
        assert bm.launch_plan(CAM, frames(count, flags=bm.BM_FLAG_ORDERED), images(count)) == dict(
            ring_mode=2, ring_group=1, sample_stride=1, pixel_stride=PIXELS, shared_digest=0, instrumented=0, counter_blocks=count, refill_min=16, workgroups=2 * LONE)


def test_several_samples_are_sample_items_and_size_the_grid():
    assert bm.frame_plan(bm.FrameParams(W, H, spp=4, max_bounces=3))["sample_items"] == 1  # the library's own choice
    for asked in (0, bm.BM_FLAG_SAMPLE_ITEMS):
        assert bm.launch_plan(CAM, frames(1, spp=4, flags=asked), A)["workgroups"] == 4 * LONE  # items, not pixels
        assert bm.launch_plan(CAM, frames(5, step=4, spp=4, flags=asked), A) == dict(ring_mode=2, ring_group=1, sample_stride=4, pixel_stride=0, shared_digest=0, instrumented=0,
                                                                                    counter_blocks=5, refill_min=32, workgroups=2 * 4 * LONE)
    # ordered frames keep pixel items whatever their spp
    assert bm.launch_plan(CAM, frames(1, spp=4, flags=bm.BM_FLAG_ORDERED), A)["workgroups"] == LONE


def test_counters_make_the_launch_instrumented():
    plan = bm.launch_plan(CAM, frames(3, flags=bm.BM_FLAG_COUNTERS), A)
    assert (plan["ring_mode"], plan["instrumented"], plan["ring_group"]) == (2, 1, 3)


def refused(fragment, *args, **kw):
    with pytest.raises(bm.BrickmapError, match=fragment):
        bm.launch_plan(*args, **kw)


def test_frame_count_and_null_buffers():
    refused("1 ... 256", CAM, [], [])
    refused("1 ... 256", CAM, frames(257), A)
    assert bm.launch_plan(CAM, frames(256), A)["ring_mode"] == 2
    refused("null accumulation buffer", CAM, frames(2), [A, None])


@pytest.mark.parametrize("field, first, other", [
    ("width", {}, dict(width=80)), ("height", {}, dict(height=64)), ("spp", {}, dict(spp=2)), ("max_bounces", {}, dict(max_bounces=2)),
    ("flags", {}, dict(flags=bm.BM_FLAG_ORDERED)), ("band_rows", {}, dict(band_rows=16)),
    ("shard_rank", dict(band_rows=16, shard_count=2), dict(band_rows=16, shard_count=2, shard_rank=1)), ("shard_count", {}, dict(shard_count=2))])
def test_frames_of_a_launch_must_agree(field, first, other):
    p = dataclasses.replace(bm.FrameParams(W, H, spp=1, max_bounces=3), **first)
    q = dataclasses.replace(p, **other)
    assert bm.launch_plan(CAM, [p, p], images(2))["ring_mode"] == 2 and bm.launch_plan(CAM, [q, q], images(2, stride=1 << 20))["ring_mode"] == 2
    refused("must agree", CAM, [p, q], images(2, stride=1 << 20))
    refused("must agree", CAM, [p, p, q], images(3, stride=1 << 20))


def test_plain_stores_need_buffers_of_their_own():
    po = frames(2, flags=bm.BM_FLAG_ORDERED)
    refused("accumulation buffers of their own", CAM, po, A)
    refused("accumulation buffers of their own", CAM, po, [A, A + IMAGE - 16])  # the last pixel of one is the first of the other
    refused("accumulation buffers of their own", CAM, po, [A + IMAGE - 16, A])
    assert bm.launch_plan(CAM, po, [A + IMAGE, A])["ring_mode"] == 1  # side by side, the second one first
    p = frames(2)
    refused("hit-record buffers of their own", CAM, p, images(2), [D, D])  # (records without the digest: ordered frames)
    refused("hit-record buffers of their own", CAM, p, images(2), [D, D + RECORDS - 32])
    refused("hit-record buffers of their own", CAM, p, images(2), [D + RECORDS - 32, D])
    refused("accumulation buffers of their own", CAM, p, A, images(2, RECORDS, D))  # ... which may not share their pixels either
    dig = frames(2, flags=bm.BM_FLAG_RAY_DIGEST)
    refused("hit-record buffers of their own", CAM, dig, images(2), [D, D])  # one digest buffer, two accumulation buffers
    refused("hit-record buffers of their own", CAM, dig, A, [D, D + 32])
    own = bm.launch_plan(CAM, dig, A, images(2, RECORDS, D))  # digests of their own: accepted, and like every launch with separate hit records a plain ring
    assert (own["ring_mode"], own["shared_digest"], own["instrumented"], own["counter_blocks"]) == (1, 0, 1, 2)


def test_a_shared_digest_needs_a_uniform_launch():
    dig = frames(3, flags=bm.BM_FLAG_RAY_DIGEST)
    assert bm.launch_plan(CAM, dig, A, [D] * 3) == dict(ring_mode=2, ring_group=3, sample_stride=1, pixel_stride=0, shared_digest=1, instrumented=1,
                                                       counter_blocks=1, refill_min=32, workgroups=2 * LONE)
    refused("uniform launch", [CAM, CAM2, CAM], dig, A, [D] * 3)
    refused("uniform launch", CAM, [dig[0], dig[1], dataclasses.replace(dig[2], sample_base=3)], A, [D] * 3)
    refused("uniform launch", CAM, dig[::-1], A, [D] * 3)
    refused("uniform launch", CAM, dig, A, [D, D, D + RECORDS])  # two frames share, the third has its own


def test_a_shared_digest_that_would_overflow_is_refused():
    rays = [bm.FrameParams(W, H, spp=8192, sample_base=8192 * k, max_bounces=3, flags=bm.BM_FLAG_RAY_DIGEST) for k in range(2)]  # 2 x 8192 x 4 = 65536
    refused("65536", CAM, rays, A, [D] * 2)
    assert bm.launch_plan(CAM, rays, A, images(2, RECORDS, D))["shared_digest"] == 0  # (every frame its own digest: inside the per-frame limit)
    keys = [bm.FrameParams(W, H, spp=1, sample_base=(1 << 17) * k, max_bounces=3, flags=bm.BM_FLAG_RAY_DIGEST) for k in range(129)]  # 2^17 x 128 + 1 > 2^24
    refused("2\\^24", CAM, keys, A, [D] * 129)
    plan = bm.launch_plan(CAM, keys[:128], A, [D] * 128)  # 2^17 x 127 + 1 < 2^24, 128 x 4 rays: inside both
    assert (plan["ring_mode"], plan["shared_digest"], plan["sample_stride"], plan["ring_group"], plan["counter_blocks"]) == (2, 1, 1 << 17, 4, 32)


def test_a_launch_past_the_round_budget_is_refused():
    """The kernel's hang guard: (tiles x 16 + 64) x (spp + 1) x (max_bounces + 2) x (2 cells + cells_height + 64) x frames must stay below 2^62."""
    side, bounces, grid, height = 65535, 10 ** 6, 1024, 256
    tiles = ((side + 15) // 16) ** 2
    per_frame = (tiles * 16 + 64) * (1 + 1) * (bounces + 2) * (2 * (grid // 8) + height // 8 + 64)
    first_refused = -(-(1 << 62) // per_frame)  # the smallest frame count whose product reaches 2^62
    assert 2 < first_refused <= 256 and per_frame * first_refused >= 1 << 62 > per_frame * (first_refused - 1)
    p = bm.FrameParams(side, side, spp=1, max_bounces=bounces, flags=bm.BM_FLAG_ORDERED)
    image = side * side * 16
    world = dict(grid_size=grid, grid_height=height)
    refused("launch too large", CAM, [p] * first_refused, images(first_refused, stride=image), **world)
    refused("launch too large", CAM, [p] * 256, images(256, stride=image), **world)
    plan = bm.launch_plan(CAM, [p] * (first_refused - 1), images(first_refused - 1, stride=image), **world)
    assert (plan["ring_mode"], plan["counter_blocks"], plan["workgroups"]) == (1, first_refused - 1, 2 * tiles)  # (too large an allocation for a uniform launch's 32-bit pixel offsets)
    # the world is part of the product: the same frames on a larger one are past the budget earlier
    refused("launch too large", CAM, [p] * (first_refused - 1), images(first_refused - 1, stride=image), grid_size=8192, grid_height=1024)


def test_a_refused_plan_is_all_zero():
    L = _lib.load()
    n = 2
    cams = (_lib.bm_camera * n)(CAM.to_c(), CAM.to_c())
    pars = (_lib.bm_frame_params * n)(*[p.to_c() for p in frames(n, flags=bm.BM_FLAG_ORDERED)])
    accs = (C.c_void_p * n)(A, A)
    raw = (C.c_uint8 * C.sizeof(_lib.bm_launch_plan))(*([0xAB] * C.sizeof(_lib.bm_launch_plan)))
    out = C.cast(raw, C.POINTER(_lib.bm_launch_plan))
    assert L.bm_launch_plan_of(n, cams, pars, accs, None, 256, 256, out) == 10001 and b"of their own" in L.bm_last_error_string()
    assert bytes(raw) == bytes(len(raw))
    raw[:] = [0xAB] * len(raw)
    assert L.bm_launch_plan_of(n, cams, pars, accs, None, 100, 256, out) == 10001 and b"world dimensions" in L.bm_last_error_string()  # not a multiple of 128
    assert bytes(raw) == bytes(len(raw))
    assert L.bm_launch_plan_of(n, cams, pars, accs, None, 256, 256, None) == 10001
