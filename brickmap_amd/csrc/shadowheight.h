// shadowheight.h -- shadow heights: per column, the cells from which no ray of the sun cone can reach the sun.  The dual of sunfield.h's
// clear heights, in the same directed coordinates, slabs and minor bins (read sunfield.h first).  Plain C++ (host + device).
//
// A shadow ray delivers one bit, occluded or not.  Below a column's shadow height that bit is decided by geometry alone: every ray of the
// cone, from anywhere in the cell, enters a FULL cell (a resident brick with all 512 voxels set) before it can leave the world, and a ray
// that enters a full brick is stopped by its first voxel at every level of detail.  Such a ray needs no walk -- it is not even drawn
// (shadow_origin below; trace.hip, shade block).
//
// A ray that is never traced makes no brick request.  In a scene that streams its bricks in, the requests of the shadow rays' walks are part
// of what makes them resident, so shadow heights are built only where EVERY brick is resident (a preloaded scene, scene.cpp
// ensure_sun_plane); a streaming scene's slice is zero and its frames request what the parent's did.
//
// Only plans with a horizontal dominant axis D (SunPlan::clear) get shadow heights; m1 is then the other horizontal axis and z the
// second minor axis.  Heights are in 1 / kSunHeightUnit cells.
//
// FULL TOP full_top(w): the number of cells of column w, from z = 0 upwards without a gap, that are full (the index word says resident
// and has all eight bits of the 2^3 level of detail, and the brick's sixteen words are all ones).  Everything else -- partly filled,
// not resident, known at a coarser level only, full but above a gap -- counts as not full, which only lowers the heights.
//
// FACE VALUE S(slab, w, b): a ray that enters column (slab, w) through its D face in bin b of m1, at a height BELOW S, certainly enters a
// full cell before it leaves the grid:
//     S = max(full_top(w) * unit, min over the bins it can leave in (b + lo1 ... b + hi1) of the next slab's S - rise_hi),   S = 0 outside the grid.
// rise_hi is an UPPER bound of what a ray of the cone rises per slab (shadow_plan: the cone's upper z slope, rounded up, plus a margin).
// Proof, by induction from the far slab (whose next slab is outside the grid: S = full_top * unit).  Let the ray enter at height h < S.
// If h < full_top(w) * unit, the cell it enters, (slab, w, floor(h / unit)), is one of the column's full cells: done.  Otherwise
// h < S_next(state) - rise_hi for every state it can enter the next slab in.  Within this slab it meets either a voxel (occluded all the
// same) or nothing; it cannot leave the grid sideways, since a state outside the grid has S = 0 and h >= 0 is not below 0 - rise_hi; it
// cannot leave through the top, since S <= n_z * unit; and it enters the next slab at h' <= h + rise_hi < S_next of that state, where the
// induction holds.
//
// DARK CELL: cell (slab, w, z) is dark if (z + 1) * unit + rise_hi + kSunHeightMargin < S_next of every state a ray from ANYWHERE in the
// cell can enter the next slab in (bins 0 ... bins - 1 + hi1: every bin, no lower bound on the move along m1 of what is left of the
// slab; rise_hi bounds the rise of what is left as it bounds a whole slab's).  The margin is the one of the clear heights: the walk's
// rounded tmax is not the exact line.  DARK HEIGHT Zd(w): the number of dark cells from z = 0 upwards; the condition is monotone in z.
//
// A cell the sun plane stamps 255 ("nothing can be hit from here on") is never dark: the stamp is sound, so a ray from it hits nothing,
// and a ray from a dark cell hits something (tests/shadowheight_check.cpp asserts it).
//
// THE TABLE is a ninth slice of the escape allocation, laid out like an octant's slice.  An entry is the sun plane's byte offset of the
// first slice that is not dark, sun_plane_offset + (Zd + 1) * cf_pxy (slices carry a one-cell border), so that "dark" is one unsigned
// compare of the ray's own sun-plane offset with it; 0 = no dark cell.
#pragma once
#include <cstdint>

#include "sunfield.h"

// -DBM_SHADOWHEIGHT=0 builds the library without shadow heights: the slice stays zero and no kernel reads it.
// -DBM_SHADOWHEIGHT_XCD=1 puts them into the kernel instantiations with the XCD-aware hand-out as well (trace.hip).  They are kept out by
// default: those instantiations serve the big streaming frames, which have no shadow heights (above) and would pay the test for
// nothing: config 3 measured 0.7 % slower with the test than without (profiles/r10_shadow_heights.txt 3).
#ifndef BM_SHADOWHEIGHT
#define BM_SHADOWHEIGHT 1
#endif
#ifndef BM_SHADOWHEIGHT_XCD
#define BM_SHADOWHEIGHT_XCD 0
#endif

namespace bm {

struct ShadowPlan {
	SunPlan sun;
	int valid;    // 1: the sun has a plane with a horizontal dominant axis; shadow heights are built
	int rise_hi;  // height units a ray rises per slab, at most
};

// kShadowLoose (check program only, never the library): 1 = rise_hi replaced by the lower bound `rise`, 2 = no margin.  Both must be
// caught by tests/shadowheight_check.cpp.
#ifndef BM_SHADOWHEIGHT_LOOSE
#define BM_SHADOWHEIGHT_LOOSE 0
#endif

BM_JHD ShadowPlan shadow_plan(const float dir[3], float extent) {
	ShadowPlan sp{};
	sp.sun = sun_plan(dir, extent);
	if (!sp.sun.valid || !sp.sun.clear) return sp;
	// the cone's upper z slope, with sun_plan's own radius r (sunfield.h): (|d_z| + r) / (|d_D| - r)
	const double e = extent;
	double s = 1.0 - (1.0 - e) * (1.0 - e);
	s = s > 0.0 ? s : 0.0;
	{
		double q = s > 0.0 ? 1.0 : 0.0;
		for (int i = 0; i < 60 && q > 0.0; ++i) q = 0.5 * (q + s / q);
		s = q;
	}
	const double r = s * 1.05 + 2e-3;
	const double az = dir[2] < 0.0f ? -static_cast<double>(dir[2]) : dir[2], ad = dir[sp.sun.dom] < 0.0f ? -static_cast<double>(dir[sp.sun.dom]) : dir[sp.sun.dom];
	const double shi = (az + r) / (ad - r); // < 1 in a valid plan
	const double h = shi * kSunHeightUnit + 0.5;
	sp.rise_hi = static_cast<int>(h) + 1; // rounded up, and at least half a unit above
#if BM_SHADOWHEIGHT_LOOSE == 1
	sp.rise_hi = sp.sun.rise;
#endif
	sp.valid = 1;
	return sp;
}

constexpr int kShadowMargin =
#if BM_SHADOWHEIGHT_LOOSE == 2
	-kSunHeightUnit; // (loose: a cell counts as dark when only its floor is below the value)
#else
	kSunHeightMargin;
#endif

// full(w): full_top * kSunHeightUnit of column w of THIS slab (w inside the grid); next(w, b): S of the next slab, 0 outside the grid
template <class Next>
BM_JHD int shadow_next_least(int w, int glo, int ghi, Next next) {
	int least = 1 << 30;
	for (int g = glo; g <= ghi; ++g) {
		const int n = next(w + g / kSunBins, g % kSunBins);
		least = n < least ? n : least;
	}
	return least;
}
template <class Next>
BM_JHD int shadow_face_value(const ShadowPlan& p, int w, int b, int full, Next next) {
	const int n = shadow_next_least(w, b + p.sun.lo1, b + p.sun.hi1, next) - p.rise_hi;
	return n > full ? n : full;
}
// Zd of the column: the number of cells z with (z + 1) * unit + rise_hi + margin < S_next of every state, at most nz
template <class Next>
BM_JHD int shadow_dark_cells(const ShadowPlan& p, int w, int nz, Next next) {
	const int t = shadow_next_least(w, 0, kSunBins - 1 + p.sun.hi1, next) - p.rise_hi - kShadowMargin;
	const int z = t > 0 ? (t - 1) / kSunHeightUnit : 0;
	return z < nz ? z : nz;
}

// the table's entry: the sun-plane byte offset of the first slice that is not dark (slice z of the grid is slice z + 1 of a plane)
BM_JHD uint32_t shadow_entry(uint32_t sun_plane_offset, uint32_t cf_pxy, int dark_cells) {
	return dark_cells > 0 ? sun_plane_offset + static_cast<uint32_t>(dark_cells + 1) * cf_pxy : 0u;
}

// WHERE A SHADOW RAY STARTS.  The rule is applied where the ray is drawn (trace.hip, shade block), before it is a ray at all: a ray whose
// origin lies in a dark cell is never set up.  That needs the cell traverse.h ray_setup WOULD give it, bit for bit -- the origin is the
// hit point pushed out along the normal and may lie in the cell next to the one the extend ray ended in -- so the cell is computed here,
// once, for the kernel and for tests/shadow_origin_check.cpp: origin / 8.f truncated, then the bordered offset of cell_offset.
// `entry` is the index of the column's entry in the escape table (slice 8), `cell` the ray's byte offset on the sun plane (plane 8 of the
// cube field); the ray is dark iff cell < table[entry].  UNDECIDED where ray_setup would not take its short way -- an origin that is not
// strictly inside the box (NaN included), a cell outside the grid: such a ray is traced like any other.  An undecided origin has
// cell == kShadowUndecided, above every entry, and entry == 0, the table's first entry, whatever it holds: the caller may load and
// compare without asking, and the answer is "not dark".  (Straight-line on purpose: the kernel runs it for every lane of a shade pass.)
// grid_size, grid_height: the world's extents in voxels; cells, cells_height: in cells; cf_shift, cf_pxy: the field's row shift and slice
// pitch (device_types.h); sun_plane: the sun plane's byte offset in the cube field, 8 * cf_plane (FrameConstants::shadow_field_off).
constexpr uint32_t kShadowUndecided = 0xFFFFFFFFu;
struct ShadowOrigin {
	uint32_t entry, cell;
};
BM_JHD bool shadow_undecided(const ShadowOrigin& so) { return so.cell == kShadowUndecided; }
BM_JHD ShadowOrigin shadow_origin(float grid_size, float grid_height, int cells, int cells_height, int cf_shift, uint32_t cf_pxy, uint32_t sun_plane, float ox, float oy,
								  float oz) {
	// (`&`, not `&&`: nothing here is worth a branch, and the device compiler makes one of every `&&`)
	const bool inside = (ox > 0.f) & (ox < grid_size) & (oy > 0.f) & (oy < grid_size) & (oz > 0.f) & (oz < grid_height); // ray_setup's `inside`, the origin's part
	const float qx = inside ? ox / 8.f : -1.f, qy = inside ? oy / 8.f : -1.f, qz = inside ? oz / 8.f : -1.f;          // (never the conversion of a NaN)
	const int px = static_cast<int>(qx), py = static_cast<int>(qy), pz = static_cast<int>(qz);
	const bool decided = inside & (px >= 0) & (px < cells) & (py >= 0) & (py < cells) & (pz >= 0) & (pz < cells_height);
	const uint32_t column = (static_cast<uint32_t>(py + 1) << cf_shift) + static_cast<uint32_t>(px + 1);
	ShadowOrigin so;
	so.entry = jump_mul24(decided ? 8u : 0u, cf_pxy) + (decided ? column : 0u); // (the slice number as a lane's value: one multiply-add, and no constant for the compiler to carry round the caller's loop)
	so.cell = decided ? sun_plane + jump_mul24(static_cast<uint32_t>(pz + 1), cf_pxy) + column : kShadowUndecided;
	return so;
}

} // namespace bm
