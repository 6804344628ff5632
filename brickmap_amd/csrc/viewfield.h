// viewfield.h -- the view plane: a tenth plane of the cube field, read by primary rays only, and the rule that fills it.
// Plain C++ (host + device) like sunfield.h and escape.h: viewfield.hip builds the plane with these functions, scene.cpp decides with
// view_plan() whether a camera gets one, and tests/view_check.cpp replays the rule against a cell-by-cell walk on the CPU.
//
// Every primary ray of a frame without a lens starts at ONE point p, the camera's position.  An octant plane must hold for every
// direction of its octant: its byte is the largest empty CUBE.  The rays that reach a cell c from p form a thin PENCIL -- the directions
// from p to the points of c -- and far from the camera the pencil sweeps a sliver of that cube; the cube is cut short by cells the
// pencil never meets (the ground under a grazing ray).  The view plane holds for the pencil only.
//
// CONTRACT, for every cell c of the grid (the octant planes' contract, restricted to the rays from p):
//     byte 0          if and only if the cell's index word is non-zero;
//     byte 1 ... 254  n: for every ray from p whose reference walk (voxel.cuh:249-258, rounded tmax) visits c, every cell that walk visits
//                     from c on, until one axis has moved n cells, is empty and inside the grid -- what field_jump needs (jump.h);
//     byte 255        such a ray meets no occupied cell between c and the border of the grid.
//
// THE RULE.  Positions are DIRECTED cell coordinates relative to p: along an axis on which the cell lies below the camera's cell the
// coordinate is mirrored, so every ray through c moves towards larger values.  With a margin m on every cell face, the points of c
// are e with  l_k <= e_k <= h_k,  l_k = (distance of the cell's near face from p) - m,  h_k = l_k + 1 + 2 m.
//   * A cell that shares an index with the camera's cell on some axis can be visited by rays of either sign on that axis (the walk only
//     ever moves with its sign, so on every other axis the sign is exact): its byte is the minimum of the cube bytes of those octants.
//     So is the byte of a cell with l_k <= 0 on some axis (the camera is within m of the cell's face).
//   * Otherwise start from n = the cube byte of the cell's octant -- that cube is empty -- and extend shell by shell.  Shell j is the
//     cells at directed offsets u with max(u) = j: three faces u_a = j.  A ray of the pencil is inside the slab of face a, widened by m,
//     while its coordinate along a is in [l_a + j, h_a + j]; along another axis b it is then between
//         (l_a + j) * (1 / h_a) * l_b   and   (h_a + j) * (1 / l_a) * h_b        (every factor positive)
//     so the cells of the face it can touch have offsets  floor(low - near_b - m) ... floor(high - near_b + m), cut to 0 ... j.  If every
//     such cell of the three faces is empty and inside the grid, n = j + 1; the first shell with a blocked cell, or kViewCap, ends it.
//   * 255 where the escape rule (escape.h) of the camera's own column ends the rays that can visit the cell: z past the threshold of
//     the cell's octant -- of every octant a ray through it can have.
//
// WHY IT HOLDS.  tmax is a chain of rounded additions; let d_k be the error of the rounded crossing times of axis k.  The walk is in
// cell i during a time T with  t_k(i_k) - d_k <= T <= t_k(i_k + 1) + d_k  on every axis, so the EXACT line is, at T, inside the cell
// widened by d_k |dir_k| on axis k.  The walk visits c: the exact line passes through c widened; it visits a cell of shell j: the exact
// line passes through that cell widened, inside the widened slab.  Both are what the rectangles above bound, if m >= d_k |dir_k|.
// The additions of axis k round by at most half an ulp of tmax_k each, 2^-24 tmax_k, and tmax_k |dir_k| is the cells crossed so far:
// after K cells the position is off by at most 2^-24 (1 + 2 + ... + K) < 2^-25 K^2 cells, plus 2^-23 K for the rounding of tdelta and
// of the first tmax.  K <= 1026 (bm_scene_create).  The margin is
//     m = max(1 / 64, 2^-22 N^2),  N = the grid's longest side in cells
// -- eight times the bound: 1/64 up to 256 cells (where the bound is 2 * 10^-3), 1/16 at 512, 1/4 at 1026.
// A jump (jump.h) lands on the reference's tmax bit for bit, so what holds for the reference walk holds for the kernels'.
#pragma once
#include <cstdint>

#include "escape.h"
#include "jump.h"

// -DBM_VIEWFIELD=0 builds the library without the view plane: no tenth plane, no build, primary rays on their octant planes.
// -DBM_VIEWFIELD_XCD=0 keeps it out of the kernel instantiations with the XCD-aware hand-out (trace.hip).
#ifndef BM_VIEWFIELD
#define BM_VIEWFIELD 1
#endif
#ifndef BM_VIEWFIELD_XCD
#define BM_VIEWFIELD_XCD 1
#endif

namespace bm {

// the largest byte the extension gives.  A jump also ends at the binade end of the smallest tmax (jump.h), which no byte can move: on
// bench config 2 the replay (tools/viewfield_sim.py) counts 12.53 stops per primary ray with a cap of 64, of 96 and of 128, and 12.66 /
// 12.80 / 13.11 with 32 / 48 / 24 -- 64 is where a longer pencil stops paying, and the build's time grows with the cap
// (profiles/r12_view_plane.txt 0, 5)
constexpr int kViewCap = 64;

struct ViewPlan {
	int valid;     // 0: primary rays keep their octant planes
	int cell[3];   // the camera's cell
	double p[3];   // the camera's position in cells: fp32 origin / 8, as ray_setup computes it
	double margin; // m
};

BM_JHD double view_margin(int cells, int cells_height) {
	const double n = cells > cells_height ? cells : cells_height, m = n * n / 4194304.0;
	return m > 1.0 / 64 ? m : 1.0 / 64;
}

// origin: FrameConstants::origin (voxels); grid_size / grid_height: the world box in voxels, as DeviceScene has them.  No plane for a
// position that is not strictly inside the box (ray_setup's short way for an inside origin; a NaN fails every comparison) and none
// for a camera with a lens: its rays start on a disk, not at p.
BM_JHD ViewPlan view_plan(const float origin[3], float lens_radius, float grid_size, float grid_height, int cells, int cells_height) {
	ViewPlan v{};
	if (!(lens_radius == 0.0f)) return v;
	const float hi[3] = {grid_size, grid_size, grid_height};
	const int n[3] = {cells, cells, cells_height};
	for (int k = 0; k < 3; ++k) {
		if (!(origin[k] > 0.0f && origin[k] < hi[k])) return v;
		const float c = origin[k] / 8.0f;
		v.p[k] = c;
		v.cell[k] = static_cast<int>(c);
		if (v.cell[k] < 0 || v.cell[k] >= n[k]) return v;
	}
	v.margin = view_margin(cells, cells_height);
	v.valid = 1;
	return v;
}

BM_JHD int view_floor(double x) {
	const int i = static_cast<int>(x);
	return static_cast<double>(i) > x ? i - 1 : i;
}

// The byte of cell (c[0], c[1], c[2]) of a grid of n[0] x n[1] x n[2] cells.
// cube(o, x, y, z): the byte of octant plane o at a cell INSIDE the grid (0 = occupied);
// threshold(o): the escape threshold E of octant o at the camera's column (escape.h).
template <class Cube, class Threshold>
BM_JHD int view_cell_byte(const ViewPlan& v, const int n[3], const int c[3], Cube cube, Threshold threshold) {
	int ambiguous = 0, oct = 0;
	for (int k = 0; k < 3; ++k) {
		if (c[k] == v.cell[k]) ambiguous |= 1 << k;
		else if (c[k] < v.cell[k]) oct |= 1 << k;
	}
	int n0 = 254;
	bool escaped = true;
	for (int o = 0; o < 8; ++o) {
		if ((o & ~ambiguous) != oct) continue;
		const int b = cube(o, c[0], c[1], c[2]);
		n0 = b < n0 ? b : n0;
		const int e = threshold(o);
		escaped = escaped && (escape_moves_down(o) ? c[2] < e : c[2] > e);
	}
	if (n0 == 0) return 0;
	if (escaped) return 255;
	if (ambiguous) return n0;
	const double m = v.margin;
	double l[3], h[3], near[3], inv_l[3], inv_h[3]; // (reciprocals: the shells' bounds cost no division; their last-bit error is nothing to the margin)
	int s[3];
	for (int k = 0; k < 3; ++k) {
		s[k] = (oct >> k & 1) ? -1 : 1;
		near[k] = s[k] > 0 ? static_cast<double>(c[k]) - v.p[k] : v.p[k] - static_cast<double>(c[k] + 1);
		l[k] = near[k] - m;
		h[k] = near[k] + 1.0 + m;
		if (!(l[k] > 0.0)) return n0;
		inv_l[k] = 1.0 / l[k];
		inv_h[k] = 1.0 / h[k];
	}
	int reach = n0;
	for (int j = n0; j < kViewCap; ++j) {
		for (int a = 0; a < 3; ++a) {
			const int b = a == 2 ? 0 : a + 1, d = a == 0 ? 2 : a - 1;
			const double near_t = (l[a] + j) * inv_h[a], far_t = (h[a] + j) * inv_l[a];
			int b0 = view_floor(near_t * l[b] - near[b] - m), d0 = view_floor(near_t * l[d] - near[d] - m);
			if (b0 > j || d0 > j) continue; // the pencil has left the cube through another face before it reaches this one (the upper ends are never below the lower)
			int b1 = view_floor(far_t * h[b] - near[b] + m), d1 = view_floor(far_t * h[d] - near[d] + m);
			b0 = b0 < 0 ? 0 : b0; d0 = d0 < 0 ? 0 : d0;
			b1 = b1 > j ? j : b1; d1 = d1 > j ? j : d1;
			int u[3];
			u[a] = j;
			for (u[d] = d0; u[d] <= d1; ++u[d])
				for (u[b] = b0; u[b] <= b1; ++u[b]) {
					const int x = c[0] + s[0] * u[0], y = c[1] + s[1] * u[1], z = c[2] + s[2] * u[2];
					if (x < 0 || x >= n[0] || y < 0 || y >= n[1] || z < 0 || z >= n[2]) return reach;
					if (cube(oct, x, y, z) == 0) return reach;
				}
		}
		reach = j + 1;
	}
	return reach;
}

} // namespace bm
