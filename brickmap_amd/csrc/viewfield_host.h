// viewfield_host.h -- the view plane of an occupancy grid built on the host with the functions of viewfield.h, from octant cube bytes and
// escape thresholds computed here by their definitions (world.cpp build_cube_field, escape.h): what tests/view_check.cpp walks rays
// through and what tools/sim/viewfield_plane.cpp hands to tools/viewfield_sim.py.  Host only; the library does not use it.
#pragma once
#include <cstdint>
#include <vector>

#include "escape.h"
#include "viewfield.h"

namespace bm {

struct ViewHostField {
	int n[3];
	std::vector<uint8_t> cube[8]; // [z][y][x]: edge of the largest empty cube with the cell as near corner along the octant, at most 254; 0 = occupied
	std::vector<int> top, bottom; // [y][x]: highest / lowest occupied z of the column, -1 / n[2] when it is empty
	size_t at(int x, int y, int z) const { return (static_cast<size_t>(z) * n[1] + y) * n[0] + x; }
	int threshold(int o, int x, int y) const { // E of octant o at column (x, y): the fold over the octant's xy-quadrant from the column on
		int acc = escape_none(o, n[2]);
		for (int yy = y; yy >= 0 && yy < n[1]; yy += (o & 2) ? -1 : 1)
			for (int xx = x; xx >= 0 && xx < n[0]; xx += (o & 1) ? -1 : 1) acc = escape_fold(o, acc, top[static_cast<size_t>(yy) * n[0] + xx], bottom[static_cast<size_t>(yy) * n[0] + xx]);
		return acc;
	}
};

// occ: one byte per cell, [z][y][x] over n[0] x n[1] x n[2] cells
inline ViewHostField view_host_field(const int n[3], const std::vector<uint8_t>& occ) {
	ViewHostField f;
	for (int k = 0; k < 3; ++k) f.n[k] = n[k];
	f.top.assign(static_cast<size_t>(n[0]) * n[1], -1);
	f.bottom.assign(f.top.size(), n[2]);
	for (int z = 0; z < n[2]; ++z)
		for (int y = 0; y < n[1]; ++y)
			for (int x = 0; x < n[0]; ++x) escape_column_fold(f.top[static_cast<size_t>(y) * n[0] + x], f.bottom[static_cast<size_t>(y) * n[0] + x], z, occ[f.at(x, y, z)] != 0);
	for (int o = 0; o < 8; ++o) {
		std::vector<uint8_t>& c = f.cube[o];
		c.assign(occ.size(), 0);
		const int s[3] = {(o & 1) ? -1 : 1, (o & 2) ? -1 : 1, (o & 4) ? -1 : 1};
		auto get = [&](int x, int y, int z) { return x < 0 || x >= n[0] || y < 0 || y >= n[1] || z < 0 || z >= n[2] ? 0 : static_cast<int>(c[f.at(x, y, z)]); };
		for (int iz = 0; iz < n[2]; ++iz) { // far end first
			const int z = s[2] > 0 ? n[2] - 1 - iz : iz;
			for (int iy = 0; iy < n[1]; ++iy) {
				const int y = s[1] > 0 ? n[1] - 1 - iy : iy;
				for (int ix = 0; ix < n[0]; ++ix) {
					const int x = s[0] > 0 ? n[0] - 1 - ix : ix;
					if (occ[f.at(x, y, z)]) continue;
					int m = 253;
					for (int k = 1; k < 8; ++k) {
						const int v = get(x + ((k & 1) ? s[0] : 0), y + ((k & 2) ? s[1] : 0), z + ((k & 4) ? s[2] : 0));
						m = v < m ? v : m;
					}
					c[f.at(x, y, z)] = static_cast<uint8_t>(m + 1);
				}
			}
		}
	}
	return f;
}

// the plane of a valid plan, [z][y][x]
inline void view_plane_host(const ViewPlan& v, const ViewHostField& f, std::vector<uint8_t>& plane) {
	plane.assign(f.cube[0].size(), 0);
	int e[8];
	for (int o = 0; o < 8; ++o) e[o] = f.threshold(o, v.cell[0], v.cell[1]);
	auto cube = [&](int o, int x, int y, int z) { return static_cast<int>(f.cube[o][f.at(x, y, z)]); };
	auto threshold = [&](int o) { return e[o]; };
	for (int z = 0; z < f.n[2]; ++z)
		for (int y = 0; y < f.n[1]; ++y)
			for (int x = 0; x < f.n[0]; ++x) {
				const int c[3] = {x, y, z};
				plane[f.at(x, y, z)] = static_cast<uint8_t>(view_cell_byte(v, f.n, c, cube, threshold));
			}
}

} // namespace bm
