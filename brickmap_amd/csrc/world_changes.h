// world_changes.h -- the device half of a change of the host world, with one owner: what bm_scene_edit and bm_scene_write_region share.  The
// host world changes first (World::edit_supercell / write_region_supercell on every supercell the change reaches), then the touched cells go
// to the device on the load stream, behind every frame in flight: one copy of the staged batch, the pool moves, one scatter kernel and -- when
// some cell's occupancy changed -- the cube-field update (edit.hip), published as an upload batch, so every frame issued later waits for it.
// Every decision of that is change_book.h's (host only, scripted on the CPU by tests/change_book_check.cpp); this class holds the staging
// buffers and stage clocks and makes the calls.  A Scene holds one, makes its own state checks (on device, not failed, validate_edits,
// check_region) and forwards.  The one place where the host world can get ahead of the device: Residency::report then fails the scene.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/brickmap.h"
#include "change_book.h"
#include "error.h"
#include "frame_order.h"
#include "hip_owned.h"
#include "residency.h"
#include "walk_fields.h"
#include "world.h"

namespace bm {

class WorldChanges {
public:
	WorldChanges(int device, World* world, Residency* residency, WalkFields* fields, FrameOrder* order, const Stream* load_stream)
		: device_(device), world_(world), residency_(residency), fields_(fields), order_(order), load_stream_(load_stream) {}

	int init() { return edit_marks_.create(); }
	// a valid batch of edits on a scene that is on the device and has not failed
	int edit(int count, const bm_edit* edits, hipStream_t stream);
	// a region that has passed Scene::check_region (pitches filled in), with a known op.  A volume in device memory is packed into one brick per
	// covered cell on the load stream (region.hip), behind the work queued on the caller's stream, and those bricks are copied to pinned memory:
	// the call's one round trip -- the host world is authoritative and hands out the slots.
	int write_region(const bm_region& r, int op, const uint8_t* voxels, int where, hipStream_t stream);
	int last_edit_ms(float* scatter_ms, float* field_ms); // device time of the last batch that changed something
	int last_region_ms(float* pack_ms, float* copy_ms, float* scatter_ms, float* field_ms);

private:
	int stage(int sci, const std::vector<uint32_t>& old_words, const uint8_t* touched, CellBatch& b); // rebind, then CellBatch::add_supercell
	int submit(CellBatch& b, hipStream_t stream, hipEvent_t* marks); // marks[0 ... 2]: around the scatter and the field update

	int device_;
	World* world_;
	Residency* residency_;
	WalkFields* fields_;
	FrameOrder* order_;
	const Stream* load_stream_;
	// pinned + device staging of one batch (StagingLayout), grown on demand; the pinned staging is the batch's until its copy has run (edit_staging_)
	PinnedBuffer<char> h_edit_;
	DeviceBuffer<char> d_edit_;
	Turn edit_staging_;
	// region writes: the packed bricks of a device volume (64 bytes per covered cell, device + pinned, grown on demand)
	DeviceBuffer<char> d_region_;
	PinnedBuffer<Brick> h_region_;
	// the stage clocks (StageMarks; the region's made on first use) and the stages the last call recorded (change_book.h has the rules)
	StageMarks<3> edit_marks_;
	StageMarks<6> region_marks_;
	unsigned edit_clocked_ = 0, region_clocked_ = 0;
};

} // namespace bm
