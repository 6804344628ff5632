// shadowheight_host.h -- the dark heights of a grid built on the host, slab by slab from the far end of the dominant axis, with the functions
// of shadowheight.h: what tests/shadowheight_check.cpp walks rays through and what tools/sim/shadowheight_slice.cpp hands to
// tools/shadowheight_sim.py.  Host only; the library does not use it.
#pragma once
#include <cstdint>
#include <vector>

#include "shadowheight.h"

namespace bm {

// full: one byte per cell, [z][y][x] over n[0] x n[1] x n[2] cells, 1 = a resident brick with every voxel set; zd: dark cells per column, [y][x]
inline void shadow_heights_host(const ShadowPlan& p, const int n[3], const std::vector<uint8_t>& full, std::vector<int>& zd) {
	zd.assign(static_cast<size_t>(n[0]) * n[1], 0);
	if (!p.valid) return;
	const SunPlan& s = p.sun;
	const int B = kSunBins, nd = n[s.dom], n1 = n[s.m1], nz = n[2];
	auto column = [&](int ud, int w) { int c[3] = {0, 0, 0}; c[s.dom] = sun_coord(s, s.dom, nd, ud); c[s.m1] = sun_coord(s, s.m1, n1, w); return static_cast<size_t>(c[1]) * n[0] + c[0]; };
	std::vector<int> top(zd.size(), 0);
	for (int y = 0; y < n[1]; ++y)
		for (int x = 0; x < n[0]; ++x) {
			int z = 0;
			while (z < nz && full[(static_cast<size_t>(z) * n[1] + y) * n[0] + x]) ++z;
			top[static_cast<size_t>(y) * n[0] + x] = z * kSunHeightUnit;
		}
	std::vector<int> sn(static_cast<size_t>(n1) * B, 0), sc(sn.size());
	for (int ud = nd - 1; ud >= 0; --ud) {
		auto next = [&](int w, int b) { return w < n1 ? sn[static_cast<size_t>(w) * B + b] : 0; };
		for (int w = 0; w < n1; ++w) {
			const size_t col = column(ud, w);
			zd[col] = shadow_dark_cells(p, w, nz, next);
			for (int b = 0; b < B; ++b) sc[static_cast<size_t>(w) * B + b] = shadow_face_value(p, w, b, top[col], next);
		}
		sn.swap(sc);
	}
}

} // namespace bm
