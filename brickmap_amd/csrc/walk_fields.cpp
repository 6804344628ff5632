// walk_fields.cpp -- the cube field, the escape table and the planes derived from them: allocation, updates, builds and readbacks (walk_fields.h).
#include "walk_fields.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/brickmap.h"
#include "escape.h"
#include "frame_plan.h"

namespace bm {

int BuildClock::stats(int device, uint64_t count, uint64_t* builds, float* last_build_ms) const {
	if (!builds || !last_build_ms) { set_error("null argument"); return BM_EINVAL; }
	*builds = count;
	*last_build_ms = 0.0f;
	if (count == 0) return 0;
	BM_HIP(hipSetDevice(device));
	BM_HIP(hipEventSynchronize(ev_[1]));
	BM_HIP(hipEventElapsedTime(last_build_ms, ev_[0], ev_[1]));
	return 0;
}

int WalkFields::allocate(const WorldDims& d, DeviceScene* view) {
	const Layout l = layout(d);
	const size_t guard = field_guard_bytes(l); // before the first plane and behind the last: field_layout.h
	if (!l.fits) { set_error("world too large for the 32-bit cube-field offsets of the walk"); return BM_EINVAL; }
	// a ninth plane behind the eight is the sun plane of shadow rays and a tenth the view plane of primary rays, where they can be had: a scene
	// without them renders as before, so doing without is no error -- neither HIP's slot nor ours keeps it
	int planes = 8;
	for (const int want : {l.tenth ? 10 : 0, l.ninth ? 9 : 0}) {
		if (planes > 8 || !want) continue;
		if (d_field_alloc_.alloc(2 * guard + l.plane * want) == 0) planes = want;
		else { (void)hipGetLastError(); set_error(""); }
	}
	if (planes == 8) { if (int e = d_field_alloc_.alloc(2 * guard + l.plane * 8)) return e; }
	l_ = l;
	guard_ = guard;
	cells_ = d.cells; cells_height_ = d.cells_height; sg_xy_ = d.supergrid_xy;
	book_.allocated(planes >= 9, planes == 10, d.cells, d.cells_height);
	BM_HIP(hipMemset(d_field_alloc_, 255, d_field_alloc_.bytes())); // the guards too
	view->cf_shift = l.shift;
	view->cf_pxy = static_cast<uint32_t>(l.pxy);
	view->cf_plane = static_cast<uint32_t>(l.plane);
	division_magic(view->cf_pxy, &view->cf_magic, &view->cf_magic_shift);
	view->cube_field = plane0(); // behind the head guard: every offset of the planes is what it was
	// ... and the escape heights that go with it, with the slice of the shadow heights behind the octants' eight: zero = no dark cell
	if (int e = d_escape_.alloc((escape_entries(view->cf_pxy) + (BM_SHADOWHEIGHT != 0 ? view->cf_pxy : 0u)) * sizeof(uint32_t))) return e;
	BM_HIP(hipMemset(d_escape_, 0, d_escape_.bytes())); // (border and padding entries: never read, never written)
	if (int e = d_escape_cols_.alloc(escape_columns_bytes(d.cells))) return e;
	view->escape = d_escape_;
	return 0;
}

void WalkFields::release() {
	(void)d_field_alloc_.release();
	book_.released();
	(void)d_escape_.release();
	(void)d_escape_cols_.release();
}

int WalkFields::upload(const uint8_t* field) {
	const size_t X = static_cast<size_t>(cells_) + 2, Z = static_cast<size_t>(cells_height_) + 2;
	// 8 planes x Z slices, each X rows of X bytes -> rows of 2^shift bytes (the padding is never read)
	for (size_t o = 0; o < 8; ++o)
		BM_HIP(hipMemcpy2D(plane0() + o * l_.plane, static_cast<size_t>(1) << l_.shift, field + o * X * X * Z, X, X, X * Z, hipMemcpyHostToDevice));
	return 0;
}

// The box of the cube field that has to be recomputed when the occupancy of the cells in [lo, hi] (unbordered, inclusive) has changed:
// an entry can change up to 254 cells away from a changed cell (kernels.h FieldUpdate)
FieldUpdate WalkFields::field_update_box(const int lo[3], const int hi[3]) const {
	FieldUpdate fu = geometry<FieldUpdate>();
	const int lim[3] = {cells_, cells_, cells_height_};
	int r0[3], r1[3];
	for (int k = 0; k < 3; ++k) { // bordered coordinates: interior cells are 1 ... lim
		r0[k] = std::max(1, lo[k] + 1 - 254);
		r1[k] = std::min(lim[k] + 1, hi[k] + 1 + 254 + 1);
	}
	fu.rx0 = r0[0]; fu.rx1 = r1[0]; fu.ry0 = r0[1]; fu.ry1 = r1[1]; fu.rz0 = r0[2]; fu.rz1 = r1[2];
	fu.ay0 = std::max(1, fu.ry0 - 254); fu.ay1 = std::min(cells_ + 1, fu.ry1 + 254);
	fu.bz0 = std::max(1, fu.rz0 - 254); fu.bz1 = std::min(cells_height_ + 1, fu.rz1 + 254);
	return fu;
}

// the columns [x0, x1) x [y0, y1) of the escape-height table (escape.hip), clipped to the grid
EscapeUpdate WalkFields::escape_update_box(int x0, int x1, int y0, int y1) const {
	EscapeUpdate u = geometry<EscapeUpdate>();
	u.x0 = std::max(0, x0); u.x1 = std::min(cells_, x1); u.y0 = std::max(0, y0); u.y1 = std::min(cells_, y1);
	if (u.x1 < u.x0) u.x1 = u.x0;
	if (u.y1 < u.y0) u.y1 = u.y0;
	return u;
}

int WalkFields::prepare_update(const FieldChange& c, hipStream_t busy) {
	if (!c.occupancy()) return 0;
	const size_t need = field_update_tmp_bytes(field_update_box(c.box_lo, c.box_hi));
	if (need <= d_cf_tmp_.bytes()) return 0;
	if (busy) BM_HIP(hipStreamSynchronize(busy));
	return d_cf_tmp_.reserve(need);
}

int WalkFields::update(const uint32_t* index_grid, const FieldChange& c, bool field_pass, hipStream_t stream) {
	book_.bits_changed(c.touch_lo, c.touch_hi);
	if (!c.occupancy()) return 0;
	if (field_pass) {
		launch_field_update(index_grid, plane0(), d_cf_tmp_, field_update_box(c.box_lo, c.box_hi), stream);
		BM_HIP(hipGetLastError());
	}
	// the columns of the cells whose occupancy changed, then the quadrant passes over the whole table
	launch_escape_update(index_grid, d_escape_cols_, d_escape_, escape_update_box(c.box_lo[0], c.box_hi[0] + 1, c.box_lo[1], c.box_hi[1] + 1), stream);
	BM_HIP(hipGetLastError());
	book_.occupancy_changed();
	return 0;
}

SunBuild WalkFields::sun_build(const FieldBook::SunStep& s) const {
	SunBuild u = geometry<SunBuild>();
	const int n[3] = {cells_, cells_, cells_height_};
	u.plan = s.plan;
	u.shadow = s.shadow;
	u.fx0 = s.fx0; u.fx1 = s.fx1; u.fy0 = s.fy0; u.fy1 = s.fy1;
	u.nd = n[s.plan.dom]; u.n1 = n[s.plan.m1]; u.n2 = n[s.plan.m2];
	return u;
}

int WalkFields::prepare(FieldBook::SunStep* s, hipStream_t stream, bool* ready) {
	*ready = false;
	if (int e = sun_clock_.create()) return e;
	const SunBuild u = sun_build(*s);
	auto none = [] { (void)hipGetLastError(); set_error(""); return 0; }; // no scratch, no plane: neither HIP's slot nor ours keeps the failure
	if (sun_build_tmp_bytes(u) > d_sun_tmp_.bytes()) {
		BM_HIP(hipStreamSynchronize(stream)); // an earlier build may still use the scratch
		if (d_sun_tmp_.reserve(sun_build_tmp_bytes(u)) != 0) return none();
	}
	if (s->shadow.valid && shadow_build_tmp_bytes(u) > d_shadow_tmp_.bytes()) {
		BM_HIP(hipStreamSynchronize(stream));
		book_.shadow_scratch_reallocated();
		book_.shadow_scan(s);
		if (d_shadow_tmp_.reserve(shadow_build_tmp_bytes(u)) != 0) return none();
	}
	*ready = true;
	return 0;
}

int WalkFields::build(const FieldBook::SunStep& s, const uint32_t* index_grid, const uint32_t* pool_base, const uint32_t* arena, hipStream_t stream) {
	BM_HIP(hipEventRecord(sun_clock_[0], stream));
	launch_sun_build(index_grid, pool_base, arena, d_escape_cols_, d_escape_, plane0(), d_sun_tmp_, d_shadow_tmp_, sun_build(s), s.step == FieldBook::kBuildPlane, stream);
	BM_HIP(hipGetLastError());
	BM_HIP(hipEventRecord(sun_clock_[1], stream));
	book_.built(s);
	return 0;
}

int WalkFields::build(const FieldBook::ViewStep& v, hipStream_t stream) {
	if (int e = view_clock_.create()) return e;
	ViewBuild u = geometry<ViewBuild>();
	u.plan = v.plan;
	BM_HIP(hipEventRecord(view_clock_[0], stream));
	launch_view_build(d_escape_, plane0(), u, stream);
	BM_HIP(hipGetLastError());
	BM_HIP(hipEventRecord(view_clock_[1], stream));
	book_.built(v);
	return 0;
}

// every plane is Z slices of X rows padded to 2^shift bytes, and the planes follow each other: count X Z rows in all
int WalkFields::read_planes(const char* what, bool have, int first, int count, uint8_t* dst, size_t capacity, size_t* bytes) {
	const size_t X = static_cast<size_t>(cells_) + 2, Z = static_cast<size_t>(cells_height_) + 2, need = have ? count * X * X * Z : 0;
	if (bytes) *bytes = need;
	if (!dst || !have) return 0;
	if (capacity < need) { set_error(std::string(what) + " buffer too small"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	BM_HIP(hipMemcpy2D(dst, X, plane0() + first * l_.plane, static_cast<size_t>(1) << l_.shift, X, count * X * Z, hipMemcpyDeviceToHost));
	return 0;
}

int WalkFields::device_cube_field(uint8_t* dst, size_t capacity, size_t* bytes) { return read_planes("cube field", true, 0, 8, dst, capacity, bytes); }

int WalkFields::sun_plane(uint8_t* dst, size_t capacity, size_t* bytes, int32_t* plan12) {
	const bool have = book_.sun_readable();
	if (plan12) {
		const SunPlan p = have ? book_.sun_plan_built() : SunPlan{};
		const int32_t v[12] = {p.valid, p.octant, p.dom, p.m1, p.m2, p.lo1, p.hi1, p.lo2, p.hi2, p.clear, p.rise, kSunBins};
		std::memcpy(plan12, v, sizeof v);
	}
	return read_planes("sun plane", have, 8, 1, dst, capacity, bytes);
}

int WalkFields::view_plane(uint8_t* dst, size_t capacity, size_t* bytes, float* origin3) {
	const bool have = book_.view_readable();
	if (origin3) for (int k = 0; k < 3; ++k) origin3[k] = have ? book_.view_key()[k] : 0.0f;
	return read_planes("view plane", have, 9, 1, dst, capacity, bytes);
}

int WalkFields::read_escape(size_t first, std::vector<uint32_t>* words) {
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	BM_HIP(hipMemcpy(words->data(), d_escape_ + first, words->size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return 0;
}

// the device's escape heights, as thresholds [8][cells][cells]
int WalkFields::escape_table(int32_t* dst, size_t capacity, size_t* count) {
	const uint32_t pxy = static_cast<uint32_t>(l_.pxy), pl = static_cast<uint32_t>(l_.plane);
	const size_t plane = static_cast<size_t>(cells_) * cells_, need = 8 * plane;
	if (count) *count = need;
	if (!dst) return 0;
	if (capacity < need) { set_error("escape table buffer too small"); return BM_EINVAL; }
	std::vector<uint32_t> entries(escape_entries(pxy));
	if (int e = read_escape(0, &entries)) return e;
	for (int o = 0; o < 8; ++o)
		for (int y = 0; y < cells_; ++y)
			for (int x = 0; x < cells_; ++x) dst[o * plane + static_cast<size_t>(y) * cells_ + x] = escape_height_of(o, entries[escape_index(o, l_.shift, pxy, x, y)], pxy, pl);
	return 0;
}

// the shadow heights as last built: the table's entries per (y, x) -- the sun plane's offset of the column's first slice that is not dark, or 0; *bytes = what they take on the device (the slice and the build's scratch)
int WalkFields::shadow_heights(uint32_t* dst, size_t capacity, size_t* count, uint64_t* bytes, int32_t* plan4) {
	const uint32_t pxy = static_cast<uint32_t>(l_.pxy);
	const bool have = BM_SHADOWHEIGHT != 0 && book_.sun_readable();
	const size_t need = have ? static_cast<size_t>(cells_) * cells_ : 0;
	if (count) *count = need;
	if (bytes) *bytes = BM_SHADOWHEIGHT != 0 ? static_cast<uint64_t>(pxy) * sizeof(uint32_t) + d_shadow_tmp_.bytes() : 0;
	if (plan4) {
		const ShadowPlan p = have ? book_.shadow_plan_built() : ShadowPlan{};
		const int32_t v[4] = {p.valid, p.sun.rise, p.rise_hi, kSunHeightUnit};
		std::memcpy(plan4, v, sizeof v);
	}
	if (!dst || !have) return 0;
	if (capacity < need) { set_error("shadow heights buffer too small"); return BM_EINVAL; }
	std::vector<uint32_t> slice(pxy);
	if (int e = read_escape(escape_entries(pxy), &slice)) return e;
	for (int y = 0; y < cells_; ++y)
		for (int x = 0; x < cells_; ++x) dst[static_cast<size_t>(y) * cells_ + x] = slice[escape_index(0, l_.shift, pxy, x, y)];
	return 0;
}

} // namespace bm
