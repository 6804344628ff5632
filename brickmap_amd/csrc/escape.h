// escape.h -- escape heights: the rule that ends the walk of a ray that can no longer meet a brick, and the table it reads.
// Plain C++ (host + device) like jump.h and steps.h: escape.hip builds the table with these functions, trace.hip / traverse.h test a
// ray against it, and tests/escape_check.cpp replays the rule against a cell-by-cell walk on the CPU.
//
// A ray only ever moves in the direction of its octant (bit 0 / 1 / 2 of the octant = direction negative in x / y / z; a zero
// component never moves and counts as positive).  For an octant that does not move down and a cell column (x, y)
//     E = max over the columns (x', y') of the octant's xy-quadrant that starts at (x, y), own column included, of top[x', y']
// with top = the highest z cell of the column whose index word is non-zero, -1 if there is none.  A ray of that octant in a cell with
// z > E has nothing but empty cells in the whole box from its cell to the far corner of the world, and it never leaves that box: it is
// a miss, whatever is left of its walk to the border.  Octants that move down mirror this: E = min of bottom[x', y'] (the lowest
// occupied z, cells_height if there is none), escaped when z < E.  "Occupied" is "index word non-zero", as in the cube field, so
// residency and LoD never change the table; edits rescan the columns they touch (escape.hip).
//
// The walk keeps a cell as the byte offset of its cube-field entry, z most significant within the octant's plane (traverse.h
// cell_offset).  An entry of the table is therefore stored as the offset of the FIRST ESCAPED SLICE of the octant's plane,
//     entry = octant * cf_plane + (E + 2) * cf_pxy    (not moving down: bordered z is z + 1, escaped from slice E + 1 on)
//     entry = octant * cf_plane + (E + 1) * cf_pxy    (moving down: escaped below slice E, whose bordered number is E + 1)
// and the test needs no coordinates: p - entry is >= 0 from the first escaped slice upwards, and the sign of the z increment turns the
// comparison round for rays that move down.
#pragma once
#include <cstdint>

#include "jump.h"

namespace bm {

// has the ray in cell `p` (byte offset of its cube-field entry, octant plane included) escaped?  `esc`: its octant's table entry at the
// column it started in; step_z: the offset increment of a z move (sign(dz) * slice pitch, 0 for dz == 0 -- then the rule of the octants
// that do not move down applies, and the entry is that of such an octant).  |p - esc| is less than a plane, which is less than 2^29.
BM_JHD bool escape_reached(uint32_t p, uint32_t esc, int step_z) {
	return static_cast<int32_t>((p - esc) ^ static_cast<uint32_t>(step_z)) >= 0;
}

// ---- the table's definition from an occupancy grid
BM_JHD bool escape_moves_down(int octant) { return (octant & 4) != 0; }
// the threshold of a quadrant that holds no occupied cell at all: every cell of the grid has escaped
BM_JHD int escape_none(int octant, int cells_height) { return escape_moves_down(octant) ? cells_height : -1; }
// one more column of the quadrant: `top` / `bottom` are the column's highest / lowest occupied z (-1 / cells_height when it is empty)
BM_JHD int escape_fold(int octant, int acc, int top, int bottom) {
	return escape_moves_down(octant) ? (bottom < acc ? bottom : acc) : (top > acc ? top : acc);
}
// one more cell of a column, from either end
BM_JHD void escape_column_fold(int& top, int& bottom, int z, bool occupied) {
	if (occupied && z > top) top = z;
	if (occupied && z < bottom) bottom = z;
}
// threshold <-> table entry
BM_JHD uint32_t escape_entry(int octant, int e, uint32_t cf_pxy, uint32_t cf_plane) {
	return static_cast<uint32_t>(octant) * cf_plane + static_cast<uint32_t>(e + (escape_moves_down(octant) ? 1 : 2)) * cf_pxy;
}
BM_JHD int escape_height_of(int octant, uint32_t entry, uint32_t cf_pxy, uint32_t cf_plane) {
	return static_cast<int>((entry - static_cast<uint32_t>(octant) * cf_plane) / cf_pxy) - (escape_moves_down(octant) ? 1 : 2);
}
// the table's element: every octant has one slice of the cube field's layout (bordered coordinates, rows padded to 2^cf_shift; the
// border and the padding are never read) -- the ray set-up has the row and column part of its cell's offset in hand, and the slice
// pitch with it: the look-up needs no constant of its own (the scheduler loop of trace.hip has no scalar register to spare)
BM_JHD uint32_t escape_index(int octant, int cf_shift, uint32_t cf_pxy, int x, int y) {
	return static_cast<uint32_t>(octant) * cf_pxy + (static_cast<uint32_t>(y + 1) << cf_shift) + static_cast<uint32_t>(x + 1);
}
BM_JHD size_t escape_entries(uint32_t cf_pxy) { return 8 * static_cast<size_t>(cf_pxy); }

} // namespace bm
