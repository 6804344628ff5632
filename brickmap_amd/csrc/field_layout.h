// field_layout.h -- where the bytes of the cube field lie: the planes' pitches and the guard bytes round them.  Host only, no HIP: walk_fields.cpp
// allocates by these two functions and tests/step_pair_check.cpp checks on the CPU that no offset the walk looks at leaves the allocation.
#pragma once
#include <cstdint>

#include "sunfield.h"  // BM_SUNFIELD
#include "viewfield.h" // BM_VIEWFIELD

namespace bm {

// Device layout of the cube field: rows padded to a power of two (1 << shift bytes), pxy = bytes of a slice, plane = bytes of one plane.  The walk
// keeps a ray's cell as ONE 32-bit byte offset into the planes and steps slices with 23-bit immediates (traverse.h cell_offset).
struct FieldLayout {
	int shift;
	uint64_t pxy, plane;
	bool fits, ninth, tenth; // the eight octant planes' offsets fit / the sun plane's as well / and the view plane's, behind it
};
inline FieldLayout field_layout(int cells, int cells_height) {
	int shift = 2;
	while ((1 << shift) < cells + 2) ++shift;
	FieldLayout l{};
	l.shift = shift;
	l.pxy = static_cast<uint64_t>(cells + 2) << shift;
	l.plane = l.pxy * static_cast<uint64_t>(cells_height + 2);
	l.fits = l.pxy < (1ull << 23) && l.plane * 8 < (1ull << 32);
	l.ninth = BM_SUNFIELD != 0 && l.fits && l.plane * 9 < (1ull << 32);
	l.tenth = BM_VIEWFIELD != 0 && l.ninth && l.plane * 10 < (1ull << 32);
	return l;
}

// Guard bytes before the first plane and behind the last one that exists, 255 like every border.  A cell the walk COMMITS is always inside a
// bordered plane; the pair move (steps.h step_pair_ahead) also loads the byte of the cell one move beyond the one it commits, before it knows
// whether that one was a border cell -- at most one slice pitch outside the planes, the largest of the three increments.  One slice pitch each
// side, rounded up to 256 bytes so that DeviceScene::cube_field keeps the alignment of the allocation.
// (The octant of plane 0 has no negative increment, so the kernels, which extend an offset with zeros, never form an offset below 0; the head
// guard makes the bound hold for every increment in every plane, which is what the CPU check tries.)
inline uint64_t field_guard_bytes(const FieldLayout& l) { return (l.pxy + 255u) & ~static_cast<uint64_t>(255u); }

} // namespace bm
