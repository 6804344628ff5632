// sunfield.h -- the sun plane: a ninth plane of the cube field, read by shadow rays only, and the rules that fill it.
// Plain C++ (host + device) like escape.h and jump.h: sunfield.hip builds the plane with these functions, scene.cpp decides with
// sun_plan() whether a frame's sun gets one, and tests/sunfield_check.cpp replays the rules against a cell-by-cell walk on the CPU.
//
// Every shadow ray of a frame points into one narrow cone (traverse.h cone_sample: within acos(1 - cone_extent) of cone_dir).  An octant
// plane must hold for every direction of its octant: its byte is the largest empty CUBE, of which a shadow ray sweeps a thin frustum,
// and its escape threshold is the highest column of a whole 90-degree quadrant.  The sun plane holds for the cone only.
//
// All positions below are DIRECTED cell coordinates: along an axis whose direction component is negative, u = n - 1 - coordinate, so a
// ray of the cone moves towards larger u on every axis.  D is the cone's dominant axis (largest component), the other two are the
// minor axes m1 < m2, and a SLAB is the set of cells with one value of u_D.  Per slab crossed, a ray of the cone moves between slo_i and
// shi_i cells along minor axis i (sun_plan: the cone's half angle plus a margin; the plane is VALID only if every direction of the cone
// lies strictly inside one octant with z positive, and shi_i < 1).  A minor position is tracked in kSunBins bins per cell; the bin
// bounds lo_i = floor(slo_i * bins), hi_i = ceil(shi_i * bins) are what the rules use.
//
// FACE VALUE F(cell, b1, b2): a ray that enters the cell through its D face, in bins (b1, b2) of the minor axes, meets nothing but
// empty cells in this slab and the F - 1 slabs behind it.  During the slab it can reach minor offsets 0 ... (b_i + hi_i) / bins, and it
// leaves in one of the bins b_i + lo_i ... b_i + hi_i (counted on from the cell's first bin):
//     F = 0 where one of the cells it can reach in the slab is occupied or outside the grid,
//     F = min(254, 1 + min of the next slab's F over the bins it can leave in)  otherwise.
// BYTE of a cell (what steps.h field_state reads): 0 = occupied; otherwise the same expression for a ray ANYWHERE in the cell -- every
// bin, and no lower bound on the minor moves of what is left of the slab: bins 0 ... bins - 1 + hi_i -- but at least 1 (one move from
// an empty cell is always valid).  A byte n therefore says: no ray of the cone, from anywhere in the cell, enters an occupied cell
// before its D axis has moved n cells -- and no axis moves more cells than that before a jump of n ends (jump.h).  Cells outside the
// grid count as occupied, so a jump lands on the border at the latest, as with the octant planes.
//
// CLEAR HEIGHTS (D horizontal; m1 is then the other horizontal axis and m2 = z): the same recurrence in two dimensions, on heights in
// 1 / kSunHeightUnit cells.  C(slab, w, b) = the z position a ray must have when it enters column (slab, w) in bin b to stay above every
// column it can still reach: the tops of the columns of this slab it can reach, and the next slab's C over the bins it can leave in,
// less the rise of one slab (floor(slo_z * unit)).  A cell at or above its column's value (any bin, no rise for what is left of the
// slab) is stamped 255, "nothing can be hit from here on"; so is every cell that the quadrant rule of escape.h ends rays in.  With
// D = z the quadrant rule alone stamps.
#pragma once
#include <cstdint>

#include "jump.h"

// -DBM_SUNFIELD=0 builds the library without the sun plane: no ninth plane, no build, shadow rays on their octant planes.
// -DBM_SUNFIELD_XCD=0 keeps it out of the kernel instantiations with the XCD-aware hand-out (trace.hip).
#ifndef BM_SUNFIELD
#define BM_SUNFIELD 1
#endif
#ifndef BM_SUNFIELD_XCD
#define BM_SUNFIELD_XCD 1
#endif

namespace bm {

constexpr int kSunBins = 4;          // bins per cell and minor axis
constexpr int kSunHeightUnit = 256;  // clear heights: units per cell
constexpr int kSunHeightMargin = 4;  // ... and what a cell must be above its column's value by (the walk's rounded tmax is not the exact line)

struct SunPlan {
	int valid;            // 0: shadow rays keep their octant plane
	int octant;           // bit 0 / 1 / 2: the cone's direction is negative in x / y / z (bit 2 is never set in a valid plan)
	int dom, m1, m2;      // dominant axis, minor axes (m1 < m2)
	int lo1, hi1, lo2, hi2; // bins a ray moves along m1 / m2 per slab, at least and at most
	int clear;            // 1: D is horizontal, clear heights are built (m1 horizontal, m2 = z)
	int rise;             // height units a ray rises per slab, at least
};

// the cone: unit axis `dir`, every direction within acos(1 - extent) of it (FrameConstants::cone_dir / cone_extent)
BM_JHD SunPlan sun_plan(const float dir[3], float extent) {
	SunPlan p{};
	const double e = extent, s2 = 1.0 - (1.0 - e) * (1.0 - e);
	if (!(e >= 0.0) || !(e < 1.0)) return p;
	double s = s2 > 0.0 ? s2 : 0.0; // sin^2 of the half angle
	{ // square root by Newton steps: plain C++ for host and device
		double r = s > 0.0 ? 1.0 : 0.0;
		for (int i = 0; i < 60 && r > 0.0; ++i) r = 0.5 * (r + s / r);
		s = r;
	}
	// |d - dir| <= 2 sin(half angle / 2) < sin(half angle) * 1.05 for every unit direction d of the cone (half angle < 1 rad); the rest is
	// the margin for the sample's own rounding and for the rounded tmax of the walk
	const double r = s * 1.05 + 2e-3;
	double a[3];
	for (int k = 0; k < 3; ++k) {
		const double c = dir[k];
		if (!(c == c)) return p;
		a[k] = c < 0.0 ? -c : c;
		if (!(a[k] - r > 0.0)) return p; // the cone touches an octant boundary (or the horizon)
		if (c < 0.0) p.octant |= 1 << k;
	}
	if (p.octant & 4) return p; // the sun is below the horizon
	p.dom = a[0] >= a[1] ? (a[0] >= a[2] ? 0 : 2) : (a[1] >= a[2] ? 1 : 2);
	p.m1 = p.dom == 0 ? 1 : 0;
	p.m2 = p.dom == 2 ? 1 : 2;
	const double den_lo = a[p.dom] + r, den_hi = a[p.dom] - r;
	int lo[2], hi[2];
	const int m[2] = {p.m1, p.m2};
	for (int i = 0; i < 2; ++i) {
		const double slo = (a[m[i]] - r) / den_lo, shi = (a[m[i]] + r) / den_hi;
		if (!(shi < 1.0)) return p;
		const double l = slo * kSunBins - 0.02, h = shi * kSunBins + 0.02;
		lo[i] = l > 0.0 ? static_cast<int>(l) : 0;                        // floor
		hi[i] = static_cast<int>(h) + (static_cast<double>(static_cast<int>(h)) < h ? 1 : 0); // ceil
		if (hi[i] > kSunBins) hi[i] = kSunBins;
		if (i == 1 && p.dom != 2) {
			const double rise = slo * kSunHeightUnit - 0.5;
			p.rise = rise > 0.0 ? static_cast<int>(rise) : 0;
		}
	}
	p.lo1 = lo[0]; p.hi1 = hi[0]; p.lo2 = lo[1]; p.hi2 = hi[1];
	p.clear = p.dom != 2;
	p.valid = 1;
	return p;
}

// directed position <-> coordinate along `axis` of a grid of n cells
BM_JHD int sun_coord(const SunPlan& p, int axis, int n, int u) { return (p.octant >> axis & 1) ? n - 1 - u : u; }

// The recurrence of F and of the byte, for the cell at directed minor position (u1, u2) of a slab: the ray leaves the slab in bins
// g1lo ... g1hi / g2lo ... g2hi, counted from the cell's first bin.  blocked(u1, u2): the cell of THIS slab is occupied or outside the grid;
// next(u1, u2, b1, b2): F of the next slab, 0 outside the grid.
template <class Blocked, class Next>
BM_JHD int sun_slab_value(int u1, int u2, int g1lo, int g1hi, int g2lo, int g2hi, Blocked blocked, Next next) {
	for (int j = 0; j <= g2hi / kSunBins; ++j)
		for (int i = 0; i <= g1hi / kSunBins; ++i)
			if (blocked(u1 + i, u2 + j)) return 0;
	int least = 253;
	for (int g2 = g2lo; g2 <= g2hi; ++g2)
		for (int g1 = g1lo; g1 <= g1hi; ++g1) {
			const int f = next(u1 + g1 / kSunBins, u2 + g2 / kSunBins, g1 % kSunBins, g2 % kSunBins);
			least = f < least ? f : least;
		}
	return 1 + least;
}
template <class Blocked, class Next>
BM_JHD int sun_face_value(const SunPlan& p, int u1, int u2, int b1, int b2, Blocked blocked, Next next) {
	return sun_slab_value(u1, u2, b1 + p.lo1, b1 + p.hi1, b2 + p.lo2, b2 + p.hi2, blocked, next);
}
// the byte of an EMPTY cell, before the 255 stamps
template <class Blocked, class Next>
BM_JHD int sun_cell_byte(const SunPlan& p, int u1, int u2, Blocked blocked, Next next) {
	const int v = sun_slab_value(u1, u2, 0, kSunBins - 1 + p.hi1, 0, kSunBins - 1 + p.hi2, blocked, next);
	return v < 1 ? 1 : v;
}

// Clear heights.  height(w): (top + 1) * kSunHeightUnit of column w of THIS slab, 0 for an empty column or one outside the grid;
// next(w, b): C of the next slab, 0 outside the grid.
template <class Height, class Next>
BM_JHD int sun_clear_slab_value(int w, int glo, int ghi, int rise, Height height, Next next) {
	int c = height(w);
	if (ghi / kSunBins) { const int h = height(w + 1); c = h > c ? h : c; }
	for (int g = glo; g <= ghi; ++g) {
		const int n = next(w + g / kSunBins, g % kSunBins) - rise;
		c = n > c ? n : c;
	}
	return c;
}
template <class Height, class Next>
BM_JHD int sun_clear_face_value(const SunPlan& p, int w, int b, Height height, Next next) {
	return sun_clear_slab_value(w, b + p.lo1, b + p.hi1, p.rise, height, next);
}
// the first z cell of the column that is clear of everything
template <class Height, class Next>
BM_JHD int sun_clear_cell(const SunPlan& p, int w, Height height, Next next) {
	const int c = sun_clear_slab_value(w, 0, kSunBins - 1 + p.hi1, 0, height, next);
	return c > 0 ? (c + kSunHeightMargin + kSunHeightUnit - 1) / kSunHeightUnit : 0; // (nothing to stay above: every cell of the column)
}

// 255 from this z cell upwards: the cone's clear cell (or any large number where there is none) and the quadrant rule's threshold E of the
// cone's octant (escape.h: escaped above E)
BM_JHD int sun_first_stamped(int clear_cell, int quadrant_threshold) { return clear_cell < quadrant_threshold + 1 ? clear_cell : quadrant_threshold + 1; }

} // namespace bm
