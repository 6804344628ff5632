"""bm_frame_plan_of reports the group size a uniform bm_render_frames launch of such frames gets (frame_plan.cpp ring_group_of; host
only): 4 for production frames whose item is a pixel, 1 -- frame after frame -- for ordered frames, which compare bit for bit with
single launches, and for (chunk, sample) items of several samples, whose lanes hold a pixel's samples side by side already."""
import brickmap_amd as bm


def test_plan_reports_the_group_size():
    assert not bm.tuning_overrides(), "this test pins the product's own rule"
    p1 = bm.frame_plan(bm.FrameParams(1920, 1080, spp=1, max_bounces=3))
    assert p1["ring_group"] == 4
    # the keys there were keep their order and their meaning
    assert list(p1)[:11] == ["flags", "ordered", "helpers", "sample_items", "xcd_handout", "refill_min", "refill_min_in_ring", "instrumented", "tiles_x", "tiles_y", "local_rows"]
    assert list(p1)[11:] == ["ring_group"]
    assert {k: v for k, v in p1.items() if k != "ring_group"} == dict(flags=0, ordered=0, helpers=1, sample_items=0, xcd_handout=0, refill_min=24, refill_min_in_ring=32,
                                                                     instrumented=0, tiles_x=120, tiles_y=68, local_rows=1080)
    assert bm.frame_plan(bm.FrameParams(1920, 1080, spp=1, max_bounces=3, flags=bm.BM_FLAG_ORDERED))["ring_group"] == 1
    assert bm.frame_plan(bm.FrameParams(1920, 1080, spp=1, max_bounces=3), hit_records=True)["ring_group"] == 1  # hit records in path order: ordered
    assert bm.frame_plan(bm.FrameParams(1920, 1080, spp=1, max_bounces=3, flags=bm.BM_FLAG_RAY_DIGEST), hit_records=True)["ring_group"] == 4  # the instrumented sibling
    for spp in (4, 8):
        asked = bm.frame_plan(bm.FrameParams(640, 360, spp=spp, max_bounces=3, flags=bm.BM_FLAG_SAMPLE_ITEMS))
        chosen = bm.frame_plan(bm.FrameParams(640, 360, spp=spp, max_bounces=3))  # (the library's own choice of (chunk, sample) items)
        assert asked["sample_items"] == chosen["sample_items"] == 1 and asked["ring_group"] == chosen["ring_group"] == 1
    # a frame so large that four frames' tickets would not fit a counter keeps the frame-after-frame hand-out
    big = bm.frame_plan(bm.FrameParams(65535, 65535, spp=1, max_bounces=3, band_rows=8, shard_rank=0, shard_count=2))
    assert big["xcd_handout"] == 1 and big["ring_group"] == 1
