// field_book.h -- what stands of the walk fields' derived planes: the sun plane with its shadow-height slice (sunfield.h, shadowheight.h) and the
// view plane (viewfield.h).  Host only, no HIP: the book holds no buffer, event or stream (walk_fields.h owns those and keeps the book); it is
// told what happens to the fields and decides what a launch that is about to read a plane has to build first.  tests/field_book_check.cpp
// scripts it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "shadowheight.h"
#include "sunfield.h"
#include "viewfield.h"

namespace bm {

class FieldBook {
public:
	enum Step { kNotUsable, kStands, kBuildSlice, kBuildPlane }; // kBuild*: usable once that has been built (built_*); the view plane has no slice
	// what a launch's sun needs: the plane is keyed on the cone (cone_dir, cone_extent); fx0 ... fy1 = the columns (half-open, inside the
	// grid) whose full tops the slice's build scans again
	struct SunStep {
		Step step = kNotUsable;
		float key[4] = {0.f, 0.f, 0.f, 0.f};
		SunPlan plan{};
		ShadowPlan shadow{}; // not valid: the build zeroes the slice
		int fx0 = 0, fx1 = 0, fy0 = 0, fy1 = 0;
	};
	// ... and its camera: the plane is keyed on the bits of the origin
	struct ViewStep {
		Step step = kNotUsable;
		float key[3] = {0.f, 0.f, 0.f};
		ViewPlan plan{};
	};

	// ---- what happens to the fields
	// allocated, for a grid of cells x cells x cells_height, with a ninth (sun) and a tenth (view) plane or without: whoever fills them has a new world
	void allocated(bool ninth, bool tenth, int cells, int cells_height) {
		sun_plane_ = ninth; view_plane_ = ninth && tenth;
		cells_ = cells; cells_height_ = cells_height;
		sun_built_ = view_built_ = false;
		sun_dirty_ = view_dirty_ = true;
		shadow_full_valid_ = false;
		shadow_zero_ = true; // (the slice is allocated zeroed)
	}
	void released() { sun_plane_ = sun_built_ = view_plane_ = view_built_ = false; }
	// some cell's occupancy changed: both planes are stale, each is rebuilt by the next launch that reads it -- a run of changes pays once
	void occupancy_changed() { sun_dirty_ = view_dirty_ = true; }
	// bricks of the columns lo ... hi (x, y; inclusive) changed their bits: the shadow heights count full bricks, their next build scans these columns as well
	void bits_changed(const int lo[2], const int hi[2]) {
		shadow_dirty_ = true;
		for (int k = 0; k < 2; ++k) { shadow_box_[k] = std::min(shadow_box_[k], lo[k]); shadow_box_[2 + k] = std::max(shadow_box_[2 + k], hi[k]); }
	}
	// the index grid was rewritten for another residency: the shadow heights count resident bricks, and only where all of them are (sun_launch's `preloaded`)
	void residency_rebuilt() { shadow_dirty_ = true; shadow_full_valid_ = false; }
	// the scratch that keeps every column's full top between builds is new: the next build scans every column (ask shadow_scan again)
	void shadow_scratch_reallocated() { shadow_full_valid_ = false; }

	// ---- a production launch is about to read a plane
	// The sun is a scene setting that stays put from frame to frame, so the plane is rebuilt only when the cone or the field has changed since
	// it was built; the slice also when only brick bits have, and then alone.  preloaded: every brick is resident -- a ray that ends at set-up
	// requests nothing, and in a streaming scene the requests of the shadow rays' walks are part of what brings the bricks in, so there the slice is zeroed.
	SunStep sun_launch(const float cone_dir[3], float cone_extent, bool preloaded) {
		SunStep s;
		if (!sun_plane_) return s;
		s.plan = sun_plan(cone_dir, cone_extent);
		if (!s.plan.valid) return s; // (the plane of another sun, if any, stays: the frames of this one keep their octant planes)
		for (int k = 0; k < 3; ++k) s.key[k] = cone_dir[k];
		s.key[3] = cone_extent;
		const bool stands = sun_built_ && !sun_dirty_ && std::memcmp(s.key, sun_key_, sizeof sun_key_) == 0; // the plane does; the shadow heights may still be stale
		s.step = kStands;
		if (stands && !(BM_SHADOWHEIGHT != 0 && shadow_dirty_)) return s;
		s.shadow = BM_SHADOWHEIGHT != 0 && preloaded ? shadow_plan(cone_dir, cone_extent) : ShadowPlan{};
		if (stands && !s.shadow.valid && shadow_zero_) { // (a batch of a streaming scene, or under a sun without shadow heights: the slice is zero and stays so, nothing to launch)
			shadow_dirty_ = false;
			shadow_plan_ = s.shadow;
			return s;
		}
		s.step = stands ? kBuildSlice : kBuildPlane;
		shadow_scan(&s);
		return s;
	}
	// the full tops do not depend on the sun: a scan of the whole world once, afterwards of the columns touched since
	void shadow_scan(SunStep* s) const {
		s->fx0 = s->fy0 = 0; s->fx1 = s->fy1 = cells_;
		if (!shadow_full_valid_) return;
		s->fx0 = std::max(0, shadow_box_[0]); s->fy0 = std::max(0, shadow_box_[1]);
		s->fx1 = std::min(cells_, shadow_box_[2] + 1); s->fy1 = std::min(cells_, shadow_box_[3] + 1);
		if (s->fx1 <= s->fx0 || s->fy1 <= s->fy0) s->fx0 = s->fx1 = s->fy0 = s->fy1 = 0;
	}
	// Built only for a camera that rests: the launch holds at least two frames from its first frame's origin (without a lens), or the production
	// launch before it started from that origin -- remembered also where the fields have no tenth plane.  A camera that moves every frame never
	// builds; a plane of another position goes unused.  frames: anything indexable whose elements have `origin` (float[3]) and `lens_radius`.
	template <class Frames>
	ViewStep view_launch(const Frames& frames, int count) {
		ViewStep v;
		const float* origin = frames[0].origin;
		const bool rested = view_last_valid_ && std::memcmp(origin, view_last_origin_, sizeof view_last_origin_) == 0;
		std::memcpy(view_last_origin_, origin, sizeof view_last_origin_);
		view_last_valid_ = true;
		if (!view_plane_) return v;
		v.plan = view_plan(origin, frames[0].lens_radius, 8.0f * static_cast<float>(cells_), 8.0f * static_cast<float>(cells_height_), cells_, cells_height_);
		if (!v.plan.valid) return v;
		std::memcpy(v.key, origin, sizeof v.key);
		if (view_built_ && !view_dirty_ && std::memcmp(origin, view_key_, sizeof view_key_) == 0) { v.step = kStands; return v; }
		int same = 0;
		for (int i = 0; i < count; ++i) same += std::memcmp(frames[i].origin, origin, sizeof v.key) == 0 && frames[i].lens_radius == 0.0f ? 1 : 0;
		if (same >= 2 || rested) v.step = kBuildPlane;
		return v;
	}

	// ---- a build was issued (one that was decided but could not be is not reported: the book stays as it was, the launch goes without the plane)
	void built(const SunStep& s) {
		std::memcpy(sun_key_, s.key, sizeof sun_key_);
		sun_plan_ = s.plan;
		sun_built_ = true;
		sun_dirty_ = shadow_dirty_ = false;
		shadow_plan_ = s.shadow;
		shadow_zero_ = !s.shadow.valid;
		if (s.shadow.valid) { // the scan has run
			shadow_full_valid_ = true;
			shadow_box_[0] = shadow_box_[1] = 1 << 30; shadow_box_[2] = shadow_box_[3] = -1;
		}
		if (s.step == kBuildPlane) sun_builds_++;
	}
	void built(const ViewStep& v) {
		std::memcpy(view_key_, v.key, sizeof view_key_);
		view_built_ = true;
		view_dirty_ = false;
		view_builds_++;
	}

	// ---- what stands.  The two planes differ in what a reader gets: the sun plane as it was last built, even if stale by now (bm_scene_sun_plane
	// and the shadow heights report the last build and its plans); the view plane only while it is not stale (bm_scene_view_plane reports none).
	bool has_sun_plane() const { return sun_plane_; }
	bool sun_readable() const { return sun_plane_ && sun_built_; }
	bool view_readable() const { return view_plane_ && view_built_ && !view_dirty_; }
	const float* sun_key() const { return sun_key_; }   // the keys of the last builds: what a launch's frames are compared with
	const float* view_key() const { return view_key_; }
	const SunPlan& sun_plan_built() const { return sun_plan_; }
	const ShadowPlan& shadow_plan_built() const { return shadow_plan_; }
	uint64_t sun_builds() const { return sun_builds_; } // builds of the plane (the slice alone is not counted)
	uint64_t view_builds() const { return view_builds_; }

private:
	int cells_ = 0, cells_height_ = 0;
	bool sun_plane_ = false, sun_built_ = false, sun_dirty_ = true; // there is a ninth plane / it has been built, for sun_key_ / the field has changed since
	float sun_key_[4] = {0.f, 0.f, 0.f, 0.f};
	SunPlan sun_plan_{};
	bool shadow_dirty_ = true;       // a brick's bits have changed since the slice was built
	bool shadow_zero_ = true;        // the slice holds zeros only (as allocated, or built for a sun or a scene without shadow heights)
	bool shadow_full_valid_ = false; // the scratch holds every column's full top of the world as it was at the last scan ...
	int shadow_box_[4] = {1 << 30, 1 << 30, -1, -1}; // ... and these columns were touched since (x0, y0, x1, y1; inclusive)
	ShadowPlan shadow_plan_{};
	uint64_t sun_builds_ = 0;
	bool view_plane_ = false, view_built_ = false, view_dirty_ = true; // likewise, for the origin in view_key_
	float view_key_[3] = {0.f, 0.f, 0.f};
	float view_last_origin_[3] = {0.f, 0.f, 0.f}; // origin of the first frame of the production launch before this one
	bool view_last_valid_ = false;
	uint64_t view_builds_ = 0;
};

} // namespace bm
