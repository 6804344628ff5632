// walk_fields.h -- what the walk reads instead of index words, with one owner: the octant cube field and behind it the sun plane and the view
// plane (sunfield.h, viewfield.h), the escape-height table with its column tops and the shadow-height slice (escape.h, shadowheight.h), the
// scratch of their updates and builds, their layout, and the book of which derived plane stands (field_book.h).  A Scene holds one and tells
// it what changed; which stream the work goes on, and its order against frames, stays the scene's business.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "change_book.h" // FieldChange: what a change of the world tells the fields
#include "device_types.h"
#include "error.h"
#include "field_book.h"
#include "field_layout.h"
#include "hip_owned.h"
#include "kernels.h"
#include "world.h"

namespace bm {

// the device time of a plane's last build
class BuildClock {
public:
	int create() { for (Event& ev : ev_) if (int e = ev.create()) return e; return 0; }
	hipEvent_t operator[](int i) const { return ev_[i]; }
	int stats(int device, uint64_t count, uint64_t* builds, float* last_build_ms) const; // count: the plane's builds so far (field_book.h)

private:
	Event ev_[2];
};

class WalkFields {
public:
	explicit WalkFields(int device) : device_(device) {}

	// Device layout of the cube field and the guard bytes round it: field_layout.h (host only)
	typedef FieldLayout Layout;
	static Layout layout(const WorldDims& d) { return field_layout(d.cells, d.cells_height); }
	static size_t tight_plane_bytes(const WorldDims& d) { return (static_cast<size_t>(d.cells) + 2) * (d.cells + 2) * (d.cells_height + 2); } // a plane with its border, rows not padded

	// Allocated, with guard bytes before and behind the planes (field_guard_bytes: the pair move looks one cell past a border), and set to 255
	// everywhere (the row padding reads as border cells: a stray offset ends a walk); the interior is the caller's -- a
	// host build copied up (upload), or the passes of edit.hip (update).  Writes the cf_*, cube_field and escape members of *view.
	int allocate(const WorldDims& d, DeviceScene* view);
	void release();
	int upload(const uint8_t* field); // the eight octant planes as the host builds them, rows tight (World::build_cube_field)

	// After a change of the index grid: the field passes over the box of cells whose occupancy changed (none: nothing but the book's note of the
	// touched columns; field_pass false: the field itself is already right, uploaded) and the escape heights of its columns, on `stream`;
	// the book hears of it.  prepare_update, before anything of the change is queued, sizes the passes' scratch: `busy` is the stream whose
	// earlier updates may still read it and is waited for before it grows (null: the caller has synchronised the device).
	int prepare_update(const FieldChange& c, hipStream_t busy);
	int update(const uint32_t* index_grid, const FieldChange& c, bool field_pass, hipStream_t stream);

	// What a launch needs built (field_book.h): prepare reserves the scratch of a sun build -- *ready false: none to be had, which is no error, the
	// launch goes without the plane and the book stays as it was -- and build issues it on `stream` between the clock's events and reports it.
	int prepare(FieldBook::SunStep* s, hipStream_t stream, bool* ready);
	int build(const FieldBook::SunStep& s, const uint32_t* index_grid, const uint32_t* pool_base, const uint32_t* arena, hipStream_t stream);
	int build(const FieldBook::ViewStep& v, hipStream_t stream);
	FieldBook& book() { return book_; }

	// readbacks, each the body of the C-ABI call of its name (include/brickmap.h); they wait for the device
	int device_cube_field(uint8_t* dst, size_t capacity, size_t* bytes);
	int sun_plane(uint8_t* dst, size_t capacity, size_t* bytes, int32_t* plan12);
	int view_plane(uint8_t* dst, size_t capacity, size_t* bytes, float* origin3);
	int escape_table(int32_t* dst, size_t capacity, size_t* count);
	int shadow_heights(uint32_t* dst, size_t capacity, size_t* count, uint64_t* bytes, int32_t* plan4);
	int sun_plane_stats(uint64_t* builds, float* ms) const { return sun_clock_.stats(device_, book_.sun_builds(), builds, ms); }
	int view_plane_stats(uint64_t* builds, float* ms) const { return view_clock_.stats(device_, book_.view_builds(), builds, ms); }
	// bm_scene_info's figures
	uint64_t cube_field_bytes() const { return 8 * l_.plane; } // (the octant planes; the sun plane, where there is one, is one more plane)
	uint64_t escape_bytes() const { return escape_entries(static_cast<uint32_t>(l_.pxy)) * sizeof(uint32_t); } // (the octants' slices; the shadow heights' slice: bm_scene_shadow_heights)
	uint64_t sun_plane_bytes() const { return book_.has_sun_plane() ? l_.plane + d_sun_tmp_.bytes() : 0; }

private:
	// the geometry members that FieldUpdate, EscapeUpdate, SunBuild and ViewBuild share (kernels.h)
	template <class U> U geometry() const {
		U u{};
		u.cells = cells_; u.cells_height = cells_height_;
		u.cf_shift = l_.shift; u.cf_pxy = static_cast<uint32_t>(l_.pxy); u.cf_plane = static_cast<uint32_t>(l_.plane);
		supergrid(u, 0);
		return u;
	}
	template <class U> auto supergrid(U& u, int) const -> decltype(void(u.sg_xy)) { u.sg_xy = sg_xy_; u.sg_xy2 = sg_xy_ * sg_xy_; }
	template <class U> void supergrid(U&, long) const {} // (ViewBuild has none)
	FieldUpdate field_update_box(const int lo[3], const int hi[3]) const;
	EscapeUpdate escape_update_box(int x0, int x1, int y0, int y1) const;
	SunBuild sun_build(const FieldBook::SunStep& s) const;
	// planes [first, first + count) of the cube field into a tight buffer; have false: there are none to report
	int read_planes(const char* what, bool have, int first, int count, uint8_t* dst, size_t capacity, size_t* bytes);
	int read_escape(size_t first, std::vector<uint32_t>* words); // words first ... first + size of the escape allocation

	int device_;
	int cells_ = 0, cells_height_ = 0, sg_xy_ = 0;
	Layout l_{};
	size_t guard_ = 0;                    // field_guard_bytes(l_)
	DeviceBuffer<uint8_t> d_field_alloc_; // head guard, the planes, tail guard
	uint8_t* plane0() const { return d_field_alloc_ + guard_; } // DeviceScene::cube_field: what every builder, edit pass and readback addresses
	// escape heights: the table the walk reads (a ninth slice behind the octants' eight holds the shadow heights), and every column's top and
	// bottom, kept for the updates.  Valid and rebuilt wherever the cube field is, on the same stream right behind it.
	DeviceBuffer<uint32_t> d_escape_;
	DeviceBuffer<int32_t> d_escape_cols_;
	DeviceBuffer<uint8_t> d_cf_tmp_, d_sun_tmp_, d_shadow_tmp_; // scratch: the field passes' intermediate planes, the sun build's, the full tops of the shadow heights
	BuildClock sun_clock_, view_clock_;
	FieldBook book_;
};

} // namespace bm
