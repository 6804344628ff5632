// frame_plan.h -- the pure-host plans (frame_plan.cpp): of a frame -- FrameConstants from a camera and frame parameters -- and of a
// launch of one or more frames -- what goes into the frame ring, which instantiation runs, how large the grid is.  Nothing here
// touches a device; Scene::render_frames (scene.cpp) issues what plan_launch decided, bm_launch_plan_of (capi.cpp) reports it.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/brickmap.h"
#include "device_types.h"

namespace bm {

void division_magic(uint32_t d, uint32_t* magic, int* shift); // floor(n / d) = umulhi(n, magic) >> shift for n < 2^30

// a wave of a multi-frame launch (the frame ring) with helper lanes takes new items once this many of its lanes are idle (plan_launch)
constexpr int kRingRefillMin = 32;
inline int ring_refill_min(int single_frame_refill_min, bool helpers, int override_refill_min) {
	return (helpers && !(override_refill_min >= 1 && override_refill_min <= 64)) ? kRingRefillMin : single_frame_refill_min;
}

// tuning overrides from the environment (tuning()): 0 / -1 = not set
struct Tuning {
	int refill_min = 0, xcd_handout = -1, helpers = -1, blocks_per_cu = 0, ring_group = 0;
};
const Tuning& tuning();

// the frames of a uniform launch are handed out in groups of this many (trace.hip "FRAME GROUPS"; ring_group_of)
constexpr int kRingGroup = 4, kMaxRingGroup = 64;
int ring_group_of(const FrameConstants& fc, int frames); // the group size a uniform launch of `frames` such frames gets (1: frame after frame)
void set_ring_group(FrameConstants* fc, int group, int frames); // ... written into the launch's first constants, with the hand-out's division by samples x group

// hit_records: the frame writes per-pixel hit records, which makes it an ORDERED frame unless it asks for the ray digest
int fill_frame_constants(const bm_camera* cam, const bm_frame_params* fp, FrameConstants* fc, bool hit_records = false);
// the instrumented instantiation of the trace kernel runs for frames that write hit records or count (BM_FLAG_COUNTERS)
inline bool instrumented_frame(uint32_t flags, bool hit_records) { return hit_records || (flags & BM_FLAG_COUNTERS); }

// ---- the plan of a launch of `count` frames (bm_render_frames)
constexpr int kMaxFramesPerLaunch = 256;
struct LaunchPlan {
	std::vector<FrameConstants> frames; // exactly what goes into the frame ring; entry 0 carries ring_uniform, the strides and the group
	int ring_mode = 0;                  // 0 one frame, 1 frame ring, 2 uniform frame ring (the RING argument of trace_paths)
	bool instrumented = false;          // hit records or BM_FLAG_COUNTERS
	bool shared_digest = false;         // ray-digest frames that all write ONE hit-record buffer (and one accumulation buffer)
	int counter_blocks = 0;             // ticket-counter blocks the launch zeroes: one per frame, per GROUP of frames in a uniform launch
	long long workgroups = 0;           // the grid before the cap by what the device keeps resident
};
// BM_EINVAL + set_error where the launch is refused (*out then holds nothing of use), or 0.  The buffer pointers are compared and
// subtracted, never dereferenced; dbgs may be null, and so may any of its entries.  cells, cells_height: the world, in bricks.
int plan_launch(int count, const bm_camera* cams, const bm_frame_params* fps, float* const* accums, uint32_t* const* dbgs, int cells, int cells_height, LaunchPlan* out);

} // namespace bm
