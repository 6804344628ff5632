// sunfield_host.h -- the sun plane of an occupancy grid built on the host, slab by slab from the far end of the dominant axis as sunfield.hip
// builds it on the device, with the functions of sunfield.h: what tests/sunfield_check.cpp walks rays through and what
// tools/sim/sunfield_plane.cpp hands to tools/sunfield_sim.py.  Host only; the library does not use it.
#pragma once
#include <cstdint>
#include <vector>

#include "escape.h"
#include "sunfield.h"

namespace bm {

// occ, plane: one byte per cell, [z][y][x] over n[0] x n[1] x n[2] cells (n[0] == n[1]); p: a valid plan
inline void sun_plane_host(const SunPlan& p, const int n[3], const std::vector<uint8_t>& occ, std::vector<uint8_t>& plane) {
	plane.assign(occ.size(), 0);
	auto at = [&](int x, int y, int z) { return (static_cast<size_t>(z) * n[1] + y) * n[0] + x; };
	const int B = kSunBins, nd = n[p.dom], n1 = n[p.m1], n2 = n[p.m2];
	auto cell = [&](int ud, int u1, int u2, int c[3]) { c[p.dom] = sun_coord(p, p.dom, nd, ud); c[p.m1] = sun_coord(p, p.m1, n1, u1); c[p.m2] = sun_coord(p, p.m2, n2, u2); };
	// column tops; the quadrant threshold of the cone's octant as running maxima along y, then x (escape.hip)
	std::vector<int> top(static_cast<size_t>(n[0]) * n[1], -1), quad(top.size()), stamped(top.size());
	for (int z = 0; z < n[2]; ++z) for (int y = 0; y < n[1]; ++y) for (int x = 0; x < n[0]; ++x) if (occ[at(x, y, z)]) top[static_cast<size_t>(y) * n[0] + x] = z;
	for (int x = 0; x < n[0]; ++x) {
		int acc = -1;
		for (int k = 0, y = (p.octant & 2) ? 0 : n[1] - 1; k < n[1]; ++k, y += (p.octant & 2) ? 1 : -1) { acc = escape_fold(p.octant, acc, top[static_cast<size_t>(y) * n[0] + x], 0); quad[static_cast<size_t>(y) * n[0] + x] = acc; }
	}
	for (int y = 0; y < n[1]; ++y) {
		int acc = -1;
		for (int k = 0, x = (p.octant & 1) ? 0 : n[0] - 1; k < n[0]; ++k, x += (p.octant & 1) ? 1 : -1) { acc = escape_fold(p.octant, acc, quad[static_cast<size_t>(y) * n[0] + x], 0); quad[static_cast<size_t>(y) * n[0] + x] = acc; }
	}
	for (size_t i = 0; i < top.size(); ++i) stamped[i] = sun_first_stamped(1 << 20, quad[i]);
	if (p.clear) {
		std::vector<int> cn(static_cast<size_t>(n1) * B, 0), cc(cn.size());
		for (int ud = nd - 1; ud >= 0; --ud) {
			auto height = [&](int w) { if (w >= n1) return 0; int c[3]; cell(ud, w, 0, c); return (top[static_cast<size_t>(c[1]) * n[0] + c[0]] + 1) * kSunHeightUnit; };
			auto next = [&](int w, int b) { return w < n1 ? cn[static_cast<size_t>(w) * B + b] : 0; };
			for (int w = 0; w < n1; ++w) {
				int c[3]; cell(ud, w, 0, c);
				const size_t col = static_cast<size_t>(c[1]) * n[0] + c[0];
				stamped[col] = sun_first_stamped(sun_clear_cell(p, w, height, next), quad[col]);
				for (int b = 0; b < B; ++b) cc[static_cast<size_t>(w) * B + b] = sun_clear_face_value(p, w, b, height, next);
			}
			cn.swap(cc);
		}
	}
	std::vector<unsigned char> fn(static_cast<size_t>(n1) * n2 * B * B, 0), fc(fn.size());
	for (int ud = nd - 1; ud >= 0; --ud) {
		auto blocked = [&](int u1, int u2) { if (u1 >= n1 || u2 >= n2) return true; int c[3]; cell(ud, u1, u2, c); return occ[at(c[0], c[1], c[2])] != 0; };
		auto next = [&](int u1, int u2, int b1, int b2) { return u1 < n1 && u2 < n2 ? static_cast<int>(fn[((static_cast<size_t>(u2) * n1 + u1) * B + b2) * B + b1]) : 0; };
		for (int u2 = 0; u2 < n2; ++u2)
			for (int u1 = 0; u1 < n1; ++u1) {
				int c[3]; cell(ud, u1, u2, c);
				const size_t i = at(c[0], c[1], c[2]);
				plane[i] = occ[i] ? 0 : (c[2] >= stamped[static_cast<size_t>(c[1]) * n[0] + c[0]] ? 255 : static_cast<unsigned char>(sun_cell_byte(p, u1, u2, blocked, next)));
				for (int b2 = 0; b2 < B; ++b2) for (int b1 = 0; b1 < B; ++b1) fc[((static_cast<size_t>(u2) * n1 + u1) * B + b2) * B + b1] = static_cast<unsigned char>(sun_face_value(p, u1, u2, b1, b2, blocked, next));
			}
		fn.swap(fc);
	}
}

} // namespace bm
