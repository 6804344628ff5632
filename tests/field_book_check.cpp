// field_book_check.cpp -- a program with its own main around csrc/field_book.h alone (no HIP, no scene), built plain and with
// -fsanitize=address,undefined by tests/test_field_book.py.  It scripts what happens to the walk fields of a scene of 32 x 32 x 16 cells --
// allocation, changes of occupancy and of brick bits, residency, scratch, launches, builds issued and not issued -- and after every step
// compares the book's decision and counters with values written out here by hand from the rules of field_book.h.
// prints "steps N" and "failures N".
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../brickmap_amd/csrc/field_book.h"

namespace {

using bm::FieldBook;

long failures = 0, steps = 0;
#define CHECK(cond)                                                                  \
	do {                                                                             \
		++steps;                                                                     \
		if (!(cond)) {                                                               \
			if (++failures <= 20) std::printf("line %d: %s\n", __LINE__, #cond);     \
		}                                                                            \
	} while (0)

constexpr int kCells = 32, kCellsHeight = 16;
constexpr float kExtent = 0.0005f;
// cones: x dominant and y dominant (horizontal dominant axis: shadow heights), z dominant (a plane, no shadow heights), below the horizon (no plane)
const float kSunX[3] = {0.8f, 0.3f, 0.52f}, kSunY[3] = {0.3f, 0.8f, 0.52f}, kSunZ[3] = {0.2f, 0.2f, 0.96f}, kSunDown[3] = {0.8f, 0.3f, -0.52f};

struct Frame {
	float origin[3];
	float lens_radius;
};
const Frame kA{{100.f, 90.f, 60.f}, 0.f}, kB{{101.f, 90.f, 60.f}, 0.f}, kC{{102.f, 90.f, 60.f}, 0.f}, kD{{103.f, 90.f, 60.f}, 0.f};

bool scan_is(const FieldBook::SunStep& s, int fx0, int fx1, int fy0, int fy1) { return s.fx0 == fx0 && s.fx1 == fx1 && s.fy0 == fy0 && s.fy1 == fy1; }
bool key_is(const float* key, const float* dir) { return std::memcmp(key, dir, 3 * sizeof(float)) == 0 && key[3] == kExtent; }

FieldBook fresh(bool ninth = true, bool tenth = true) {
	FieldBook b;
	b.allocated(ninth, tenth, kCells, kCellsHeight);
	return b;
}
// a book whose sun plane and slice stand for kSunX in a preloaded scene: one build of the plane
FieldBook standing() {
	FieldBook b = fresh();
	b.built(b.sun_launch(kSunX, kExtent, true));
	return b;
}
FieldBook::ViewStep view1(FieldBook& b, const Frame& f) { return b.view_launch(&f, 1); }
FieldBook::ViewStep view2(FieldBook& b, const Frame& f, const Frame& g) {
	const Frame fs[2] = {f, g};
	return b.view_launch(fs, 2);
}

void fresh_fields_with_both_planes() {
	FieldBook b = fresh();
	CHECK(b.has_sun_plane() && !b.sun_readable() && !b.view_readable() && b.sun_builds() == 0 && b.view_builds() == 0);
	FieldBook::SunStep s = b.sun_launch(kSunX, kExtent, true);
	CHECK(s.step == FieldBook::kBuildPlane && s.plan.valid == 1 && s.plan.dom == 0 && s.shadow.valid == 1 && key_is(s.key, kSunX));
	CHECK(scan_is(s, 0, 32, 0, 32)); // nothing scanned yet: every column
	b.built(s);
	CHECK(b.sun_builds() == 1 && b.sun_readable() && key_is(b.sun_key(), kSunX) && b.sun_plan_built().dom == 0 && b.shadow_plan_built().valid == 1);
	s = b.sun_launch(kSunX, kExtent, true);
	CHECK(s.step == FieldBook::kStands && b.sun_builds() == 1);
	s = b.sun_launch(kSunY, kExtent, true); // another cone: the plane again; the full tops do not depend on the sun and nothing was touched
	CHECK(s.step == FieldBook::kBuildPlane && s.plan.dom == 1 && s.shadow.valid == 1 && scan_is(s, 0, 0, 0, 0));
	b.built(s);
	CHECK(b.sun_builds() == 2 && key_is(b.sun_key(), kSunY) && b.sun_plan_built().dom == 1);
	s = b.sun_launch(kSunDown, kExtent, true); // no plan: not usable, and the standing plane and its key are left alone
	CHECK(s.step == FieldBook::kNotUsable && s.plan.valid == 0);
	CHECK(b.sun_builds() == 2 && b.sun_readable() && key_is(b.sun_key(), kSunY));
	CHECK(b.sun_launch(kSunY, kExtent, true).step == FieldBook::kStands);
	s = b.sun_launch(kSunY, 0.001f, true); // the extent is part of the key
	CHECK(s.step == FieldBook::kBuildPlane && s.key[3] == 0.001f);
	s = b.sun_launch(kSunZ, kExtent, true); // a plane without shadow heights: the slice is zeroed by the build
	CHECK(s.step == FieldBook::kBuildPlane && s.plan.dom == 2 && s.shadow.valid == 0);
	b.built(s);
	CHECK(b.sun_builds() == 3 && b.shadow_plan_built().valid == 0);
	b.released();
	CHECK(!b.has_sun_plane() && !b.sun_readable() && !b.view_readable() && b.sun_launch(kSunZ, kExtent, true).step == FieldBook::kNotUsable);
}

void occupancy_change() {
	FieldBook b = standing();
	b.built(view2(b, kA, kA));
	CHECK(b.sun_builds() == 1 && b.view_builds() == 1 && b.sun_readable() && b.view_readable());
	b.occupancy_changed();
	b.occupancy_changed(); // two changes in a row pay once
	CHECK(b.sun_readable() && !b.view_readable()); // the sun plane reads as last built, the view plane as none while it is stale
	FieldBook::SunStep s = b.sun_launch(kSunX, kExtent, true);
	CHECK(s.step == FieldBook::kBuildPlane && scan_is(s, 0, 0, 0, 0)); // (no brick's bits were reported: no column to scan)
	b.built(s);
	CHECK(b.sun_builds() == 2);
	CHECK(b.sun_launch(kSunX, kExtent, true).step == FieldBook::kStands && b.sun_builds() == 2);
}

void bits_only_change() {
	FieldBook b = standing();
	const int lo0[2] = {3, 5}, hi0[2] = {7, 6}, lo1[2] = {6, 2}, hi1[2] = {40, 9};
	b.bits_changed(lo0, hi0);
	b.bits_changed(lo1, hi1);
	FieldBook::SunStep s = b.sun_launch(kSunX, kExtent, true);
	CHECK(s.step == FieldBook::kBuildSlice && s.shadow.valid == 1);
	CHECK(scan_is(s, 3, 32, 2, 10)); // the union x 3 ... 40, y 2 ... 9, clipped to 32 cells, half-open
	b.built(s);
	CHECK(b.sun_builds() == 1); // the plane stood
	CHECK(b.sun_launch(kSunX, kExtent, true).step == FieldBook::kStands);
	const int lo2[2] = {1, 1};
	b.bits_changed(lo2, lo2);
	s = b.sun_launch(kSunX, kExtent, true);
	CHECK(s.step == FieldBook::kBuildSlice && scan_is(s, 1, 2, 1, 2)); // the box was empty again after the build
	const int out_lo[2] = {40, 40}, out_hi[2] = {50, 50};
	FieldBook c = standing();
	c.bits_changed(out_lo, out_hi);
	s = c.sun_launch(kSunX, kExtent, true);
	CHECK(s.step == FieldBook::kBuildSlice && scan_is(s, 0, 0, 0, 0)); // nothing of the box inside the grid: no column
}

void not_preloaded() {
	FieldBook b = standing();
	const int at[2] = {4, 4};
	b.bits_changed(at, at);
	FieldBook::SunStep s = b.sun_launch(kSunX, kExtent, false); // a streaming scene: no shadow plan; the slice holds heights and must be zeroed
	CHECK(s.step == FieldBook::kBuildSlice && s.shadow.valid == 0);
	b.built(s);
	CHECK(b.sun_builds() == 1 && b.shadow_plan_built().valid == 0);
	b.bits_changed(at, at);
	s = b.sun_launch(kSunX, kExtent, false); // a zero slice and a standing plane: nothing to launch, and the slice is clean
	CHECK(s.step == FieldBook::kStands && s.shadow.valid == 0);
	CHECK(b.sun_launch(kSunX, kExtent, true).step == FieldBook::kStands); // (clean: not even a launch that could have heights rebuilds it)
	FieldBook c = fresh();
	s = c.sun_launch(kSunX, kExtent, false); // the first build of a streaming scene: the plane, the slice zeroed
	CHECK(s.step == FieldBook::kBuildPlane && s.shadow.valid == 0 && scan_is(s, 0, 32, 0, 32));
}

void residency_and_scratch() {
	const int at[2] = {4, 4};
	FieldBook b = standing();
	b.residency_rebuilt();
	FieldBook::SunStep s = b.sun_launch(kSunX, kExtent, true);
	CHECK(s.step == FieldBook::kBuildSlice && s.shadow.valid == 1 && scan_is(s, 0, 32, 0, 32));
	b.built(s);
	CHECK(b.sun_builds() == 1 && b.sun_launch(kSunX, kExtent, true).step == FieldBook::kStands);
	b.bits_changed(at, at);
	b.shadow_scratch_reallocated();
	s = b.sun_launch(kSunX, kExtent, true);
	CHECK(s.step == FieldBook::kBuildSlice && scan_is(s, 0, 32, 0, 32));
	b.built(s);
	b.bits_changed(at, at);
	s = b.sun_launch(kSunX, kExtent, true);
	CHECK(s.step == FieldBook::kBuildSlice && scan_is(s, 4, 5, 4, 5));
	b.shadow_scratch_reallocated(); // ... between the decision and the build, as where the build finds its scratch too small
	b.shadow_scan(&s);
	CHECK(scan_is(s, 0, 32, 0, 32));
}

void view_plane() {
	FieldBook b = fresh();
	FieldBook::ViewStep v = view2(b, kA, kA); // two frames from one origin
	CHECK(v.step == FieldBook::kBuildPlane && v.plan.valid == 1 && v.plan.cell[0] == 12 && v.plan.cell[1] == 11 && v.plan.cell[2] == 7 && std::memcmp(v.key, kA.origin, sizeof v.key) == 0);
	b.built(v);
	CHECK(b.view_builds() == 1 && b.view_readable() && std::memcmp(b.view_key(), kA.origin, 3 * sizeof(float)) == 0);
	CHECK(view1(b, kB).step == FieldBook::kNotUsable);       // one frame from elsewhere
	CHECK(view2(b, kA, kC).step == FieldBook::kStands);      // the standing plane with a matching key: no build, rested or not
	CHECK(view2(b, kC, kD).step == FieldBook::kNotUsable);   // distinct origins after a different previous origin (kA)
	CHECK(view1(b, kC).step == FieldBook::kBuildPlane);      // the origin of the previous production launch
	CHECK(b.view_builds() == 1);                              // (decided, not issued)
	const Frame lens{{100.f, 90.f, 60.f}, 0.25f}, outside{{300.f, 90.f, 60.f}, 0.f};
	CHECK(view2(b, lens, lens).step == FieldBook::kNotUsable);       // a lens: no plan
	CHECK(view2(b, outside, outside).step == FieldBook::kNotUsable); // outside the world (256 voxels): no plan
	CHECK(view1(b, kB).step == FieldBook::kNotUsable);
	b.occupancy_changed(); // stale: rebuilt only under the rest rule
	CHECK(!b.view_readable());
	CHECK(view2(b, kA, kC).step == FieldBook::kNotUsable); // the key matches, but the plane is stale and the camera has not rested
	v = view1(b, kA);                                       // now it has
	CHECK(v.step == FieldBook::kBuildPlane);
	b.built(v);
	CHECK(b.view_builds() == 2 && b.view_readable() && view1(b, kA).step == FieldBook::kStands);
}

void missing_planes() {
	FieldBook b = fresh(true, false); // no tenth plane
	CHECK(b.has_sun_plane() && b.sun_launch(kSunX, kExtent, true).step == FieldBook::kBuildPlane);
	CHECK(view2(b, kA, kA).step == FieldBook::kNotUsable && view1(b, kA).step == FieldBook::kNotUsable && !b.view_readable());
	b.allocated(true, true, kCells, kCellsHeight); // the last origin was tracked all along: the camera has rested
	CHECK(view1(b, kA).step == FieldBook::kBuildPlane);
	FieldBook c = fresh(false, false); // no ninth plane, hence no tenth
	CHECK(!c.has_sun_plane() && c.sun_launch(kSunX, kExtent, true).step == FieldBook::kNotUsable && view2(c, kA, kA).step == FieldBook::kNotUsable);
	FieldBook d = fresh(false, true);
	CHECK(d.sun_launch(kSunX, kExtent, true).step == FieldBook::kNotUsable && view2(d, kA, kA).step == FieldBook::kNotUsable);
}

void build_not_issued() {
	FieldBook b = fresh();
	const FieldBook::SunStep s0 = b.sun_launch(kSunX, kExtent, true), s1 = b.sun_launch(kSunX, kExtent, true);
	CHECK(s0.step == FieldBook::kBuildPlane && s1.step == FieldBook::kBuildPlane && scan_is(s1, 0, 32, 0, 32) && s1.shadow.valid == 1);
	CHECK(b.sun_builds() == 0 && !b.sun_readable());
	const FieldBook::ViewStep v0 = view2(b, kA, kA), v1 = view2(b, kA, kA);
	CHECK(v0.step == FieldBook::kBuildPlane && v1.step == FieldBook::kBuildPlane && b.view_builds() == 0 && !b.view_readable());
	FieldBook c = standing();
	const int at[2] = {9, 8};
	c.bits_changed(at, at);
	const FieldBook::SunStep t0 = c.sun_launch(kSunX, kExtent, true), t1 = c.sun_launch(kSunX, kExtent, true);
	CHECK(t0.step == FieldBook::kBuildSlice && t1.step == FieldBook::kBuildSlice && scan_is(t0, 9, 10, 8, 9) && scan_is(t1, 9, 10, 8, 9) && c.sun_builds() == 1);
}

} // namespace

int main() {
	fresh_fields_with_both_planes();
	occupancy_change();
	bits_only_change();
	not_preloaded();
	residency_and_scratch();
	view_plane();
	missing_planes();
	build_not_issued();
	std::printf("steps %ld\nfailures %ld\n", steps, failures);
	return failures == 0 ? 0 : 1;
}
