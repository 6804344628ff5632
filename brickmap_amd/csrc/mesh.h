// mesh.h -- the rules of surface extraction (bm_mesh_quads, bm_mesh_triangles, include/brickmap.h), written once for the kernels of
// mesh.hip and the plain loops of mesh_host.cpp.  Needs no HIP header: tests/mesh_check.cpp builds it with a host compiler.
//
// All integers.  A face is (solid voxel p, direction d) with p + d empty; the meshed voxels are cut into the world's 8^3 brick cells;
// inside a cell every (direction, slice) has an 8 x 8 mask of faces, which the greedy cover turns into rectangles in a fixed order.
// What the kernels add to that is the layout of a cell's 10^3 neighbourhood as 100 rows of 10 bits (row r = 10 rz + ry, bit j = the
// voxel at cell-local (j - 1, ry - 1, rz - 1)) and the lane l = 8 d + s that owns a mask; both are here, so that the check program
// can walk a cell lane by lane without a device.
#pragma once
#include <cstdint>

#include "device_types.h"

namespace bm {

constexpr uint32_t kMeshHalo = 1, kMeshUnit = 2; // BM_MESH_HALO, BM_MESH_UNIT_FACES
constexpr int kMeshMaxExtent = 16384;            // voxels per axis of the volume
constexpr int64_t kMeshMaxVoxels = (int64_t{1} << 31) - 2;
constexpr int32_t kMeshMaxCoord = 1 << 23;       // the box lies within +- this, so every corner is an exact fp32 integer
constexpr int kMeshRows = 100;                   // (y, z) rows of a cell's neighbourhood
constexpr int kMeshLanes = 48;                   // masks of a cell: 6 directions x 8 slices
constexpr uint32_t kMeshScanBlock = 256;         // cells per workgroup of the offset scan

struct MeshParamsView {
	int32_t lo[3], extent[3];
	int64_t row_pitch, slice_pitch;
	uint32_t flags, reserved;
};

// the view of a bm_mesh_params (a template, so that this header needs no other)
template <class P>
inline MeshParamsView mesh_params_view(const P& p) {
	return {{p.lo[0], p.lo[1], p.lo[2]}, {p.extent[0], p.extent[1], p.extent[2]}, p.row_pitch, p.slice_pitch, p.flags, p.reserved};
}

// null, or why bm_mesh_quads and bm_host_mesh_quads refuse these parameters (pitches as given: 0 = tight)
inline const char* mesh_params_problem(const MeshParamsView& p) {
	if (p.flags & ~(kMeshHalo | kMeshUnit)) return "unknown flag";
	if (p.reserved != 0) return "reserved is not 0";
	const int least = (p.flags & kMeshHalo) ? 3 : 1;
	for (int k = 0; k < 3; ++k)
		if (p.extent[k] < least || p.extent[k] > kMeshMaxExtent) return "an extent below 1 (below 3 with BM_MESH_HALO) or above 16384";
	if (static_cast<int64_t>(p.extent[0]) * p.extent[1] > kMeshMaxVoxels / p.extent[2]) return "more than 2^31 - 2 voxels";
	if (p.row_pitch < 0 || p.slice_pitch < 0) return "negative pitch";
	if (p.row_pitch > (int64_t{1} << 40)) return "row_pitch above 2^40";
	const int64_t row = p.row_pitch ? p.row_pitch : p.extent[0];
	if (row < p.extent[0]) return "row_pitch below the extent along x";
	if (p.slice_pitch && p.slice_pitch / p.extent[1] < row) return "slice_pitch below row_pitch * the extent along y";
	if ((p.slice_pitch ? p.slice_pitch : row * p.extent[1]) > (int64_t{1} << 46) / p.extent[2]) return "a volume spanning more than 2^46 bytes";
	for (int k = 0; k < 3; ++k)
		if (p.lo[k] < -kMeshMaxCoord || p.lo[k] > kMeshMaxCoord - p.extent[k]) return "a box outside +-2^23 voxels";
	return nullptr;
}

// floor(a / 8) for a of either sign
BM_VHD int32_t mesh_floor8(int32_t a) { return a >> 3; }

// what the kernels and the loops need of the parameters: the meshed index range [m0, m1) per axis and the cells it spans
struct MeshDims {
	int32_t lo[3], extent[3];
	int32_t m0[3], m1[3];    // the voxels (volume indices) that emit faces
	int32_t cell0[3];        // first world cell per axis
	uint32_t ncell[3];       // cells per axis
	uint32_t cells;          // their product (below 2^24)
	uint32_t unit;
	int64_t row_pitch, slice_pitch; // resolved: never 0
};

inline MeshDims mesh_dims(const MeshParamsView& p) {
	MeshDims d;
	const int halo = (p.flags & kMeshHalo) ? 1 : 0;
	for (int k = 0; k < 3; ++k) {
		d.lo[k] = p.lo[k];
		d.extent[k] = p.extent[k];
		d.m0[k] = halo;
		d.m1[k] = p.extent[k] - halo;
		d.cell0[k] = mesh_floor8(p.lo[k] + d.m0[k]);
		d.ncell[k] = static_cast<uint32_t>(mesh_floor8(p.lo[k] + d.m1[k] - 1) - d.cell0[k] + 1);
	}
	d.cells = d.ncell[0] * d.ncell[1] * d.ncell[2];
	d.unit = (p.flags & kMeshUnit) ? 1u : 0u;
	d.row_pitch = p.row_pitch ? p.row_pitch : p.extent[0];
	d.slice_pitch = p.slice_pitch ? p.slice_pitch : d.row_pitch * p.extent[1];
	return d;
}

// bytes from the volume's first byte to one past its last
inline uint64_t mesh_span(const MeshDims& d) {
	return static_cast<uint64_t>(d.extent[2] - 1) * static_cast<uint64_t>(d.slice_pitch) + static_cast<uint64_t>(d.extent[1] - 1) * static_cast<uint64_t>(d.row_pitch) +
		   static_cast<uint64_t>(d.extent[0]);
}

// workspace: one 32-bit word per cell (rounded up to 16 bytes), then one 64-bit word per scan block and one for the total
inline uint32_t mesh_scan_blocks(const MeshDims& d) { return (d.cells + kMeshScanBlock - 1) / kMeshScanBlock; }
inline size_t mesh_cells_bytes(const MeshDims& d) { return (static_cast<size_t>(d.cells) * 4 + 15) & ~static_cast<size_t>(15); }
inline size_t mesh_workspace_bytes(const MeshDims& d) { return mesh_cells_bytes(d) + (static_cast<size_t>(mesh_scan_blocks(d)) + 1) * 8; }

// ---- a cell
// cell c in (z, y, x) order -> the volume index of its voxel (0, 0, 0), which may lie before the volume or the meshed box
BM_VHD void mesh_cell_origin(const MeshDims& d, uint32_t c, int32_t i0[3]) {
	const uint32_t q = c / d.ncell[0];
	const uint32_t ci[3] = {c - q * d.ncell[0], q % d.ncell[1], q / d.ncell[1]};
	for (int a = 0; a < 3; ++a) i0[a] = 8 * (d.cell0[a] + static_cast<int32_t>(ci[a])) - d.lo[a];
}

// per axis, bit k: the cell's voxel k lies in the meshed range
BM_VHD uint32_t mesh_valid8(const MeshDims& d, int a, int32_t i0) {
	uint32_t m = 0;
	for (int k = 0; k < 8; ++k)
		if (i0 + k >= d.m0[a] && i0 + k < d.m1[a]) m |= 1u << k;
	return m;
}

// the two in-slice axes of axis a, ascending: (y, z), (x, z), (x, y)
BM_VHD int mesh_axis_u(int a) { return a == 0 ? 1 : 0; }
BM_VHD int mesh_axis_v(int a) { return a == 2 ? 1 : 2; }

// what row r = 10 rz + ry must hold for a cell without faces because everything is solid: the cell's own rows all ten bits (the cell and
// its two x-facing slices), the rows of the y- and z-facing slices bits 1 ... 8, edge and corner rows nothing
BM_VHD uint32_t mesh_row_full_mask(int r) {
	const int ry = r % 10, rz = r / 10;
	const bool ey = ry == 0 || ry == 9, ez = rz == 0 || rz == 9;
	return ey && ez ? 0u : (ey || ez ? 0x1FEu : 0x3FFu);
}

// the face mask of lane l = 8 d + s from the cell's 100 rows: solid & ~neighbour, restricted to the meshed range (valid[axis])
BM_VHD uint64_t mesh_lane_mask(const uint16_t* rows, int l, const uint32_t valid[3]) {
	const int d = l >> 3, s = l & 7, a = d >> 1;
	const int step = (d & 1) ? 1 : -1;
	const uint32_t va8 = a == 0 ? valid[0] : (a == 1 ? valid[1] : valid[2]); // (selects: the axis differs from lane to lane)
	if (!((va8 >> s) & 1u)) return 0;
	uint64_t m = 0;
	if (a == 0) { // (u, v) = (y, z): one bit of 64 rows
		for (int v = 0; v < 8; ++v)
			for (int u = 0; u < 8; ++u) {
				const uint32_t row = rows[10 * (v + 1) + (u + 1)];
				const uint64_t bit = (row >> (s + 1)) & ~(row >> (s + 1 + step)) & 1u;
				m |= bit << (8 * v + u);
			}
	} else if (a == 1) { // (u, v) = (x, z): eight bits of row (s, v) against the row beside it in y
		for (int v = 0; v < 8; ++v) {
			const uint32_t row = rows[10 * (v + 1) + (s + 1)], other = rows[10 * (v + 1) + (s + 1 + step)];
			m |= static_cast<uint64_t>(((row & ~other) >> 1) & 0xFFu) << (8 * v);
		}
	} else { // (u, v) = (x, y): eight bits of row (v, s) against the row beside it in z
		for (int v = 0; v < 8; ++v) {
			const uint32_t row = rows[10 * (s + 1) + (v + 1)], other = rows[10 * (s + 1 + step) + (v + 1)];
			m |= static_cast<uint64_t>(((row & ~other) >> 1) & 0xFFu) << (8 * v);
		}
	}
	const uint32_t vu = a == 0 ? valid[1] : valid[0], vv = a == 2 ? valid[1] : valid[2];
	uint64_t keep = 0;
	for (int v = 0; v < 8; ++v)
		if ((vv >> v) & 1u) keep |= static_cast<uint64_t>(vu) << (8 * v);
	return m & keep;
}

// ---- the greedy cover of an 8 x 8 mask (bit 8 v + u): lowest set bit, its run along u, the rows below that hold the whole run; at most
// 64 rounds.  emit(u0, v0, w, h) per rectangle, in order.
template <class Emit>
BM_VHD void mesh_cover(uint64_t m, bool unit, Emit&& emit) {
	for (int round = 0; round < 64 && m != 0; ++round) {
		const int b = __builtin_ctzll(m);
		const int u0 = b & 7, v0 = b >> 3;
		int w = 1, h = 1;
		if (!unit) {
			const uint32_t run = (static_cast<uint32_t>(m >> (8 * v0)) & 0xFFu) >> u0; // bit 0 set, nothing at or above bit 8 - u0
			w = __builtin_ctz(~run);
			const uint32_t rect = ((1u << w) - 1u) << u0;
			while (v0 + h < 8 && (static_cast<uint32_t>(m >> (8 * (v0 + h))) & rect) == rect) ++h;
		}
		const uint64_t rect = static_cast<uint64_t>(((1u << w) - 1u) << u0);
		const uint64_t rows = h == 8 ? ~uint64_t{0} : (uint64_t{1} << (8 * h)) - 1;
		m &= ~(((rect * 0x0101010101010101ull) & rows) << (8 * v0));
		emit(u0, v0, w, h);
	}
}

// quads and faces of a mask, packed quads | faces << 16 (at most 32 and 64)
BM_VHD uint32_t mesh_cover_count(uint64_t m, bool unit) {
	uint32_t n = 0;
	mesh_cover(m, unit, [&](int, int, int w, int h) { n += 1u + (static_cast<uint32_t>(w * h) << 16); });
	return n;
}

// the 16 bytes of a quad: world voxel of its lowest solid voxel, shape = d | w << 4 | h << 8
struct MeshQuad {
	int32_t x, y, z;
	uint32_t shape;
};

// the quad of rectangle (u0, v0, w, h) of lane l in the cell whose voxel (0, 0, 0) is world voxel w0
BM_VHD MeshQuad mesh_quad(const int32_t w0[3], int l, int u0, int v0, int w, int h) {
	const int d = l >> 3, s = l & 7, a = d >> 1;
	// (selects, not an array indexed by the axis: the axis differs from lane to lane)
	const int32_t x = w0[0] + (a == 0 ? s : u0), y = w0[1] + (a == 1 ? s : (a == 0 ? u0 : v0)), z = w0[2] + (a == 2 ? s : v0);
	return {x, y, z, static_cast<uint32_t>(d) | static_cast<uint32_t>(w) << 4 | static_cast<uint32_t>(h) << 8};
}

// ---- a quad's two triangles, 18 floats: the plane at c_a (negative direction) or c_a + 1; corners c00, c10 = c00 + w e_u, c11, c01 =
// c00 + h e_v; counter-clockwise seen from outside.  A record whose direction is above 5 gives 18 zeros.
BM_VHD void mesh_quad_triangles(const MeshQuad& q, float* out) {
	const uint32_t d = q.shape & 15u;
	if (d > 5u) {
		for (int k = 0; k < 18; ++k) out[k] = 0.0f;
		return;
	}
	const int a = static_cast<int>(d >> 1), ua = mesh_axis_u(a), va = mesh_axis_v(a);
	const int32_t w = static_cast<int32_t>((q.shape >> 4) & 15u), h = static_cast<int32_t>((q.shape >> 8) & 15u);
	// e_u x e_v is +x for (y, z), -y for (x, z), +z for (x, y)
	const bool along = ((d & 1u) != 0) == (a != 1);
	const int32_t base[3] = {q.x, q.y, q.z};
	for (int k = 0; k < 3; ++k) { // (k is a constant once unrolled: selects, no array indexed by the axis)
		const int32_t c00 = base[k] + (k == a ? static_cast<int32_t>(d & 1u) : 0);
		const int32_t c10 = c00 + (k == ua ? w : 0), c01 = c00 + (k == va ? h : 0), c11 = c10 + (k == va ? h : 0);
		out[0 + k] = static_cast<float>(c00);
		out[3 + k] = static_cast<float>(along ? c10 : c01);
		out[6 + k] = static_cast<float>(c11);
		out[9 + k] = static_cast<float>(c00);
		out[12 + k] = static_cast<float>(c11);
		out[15 + k] = static_cast<float>(along ? c01 : c10);
	}
}

} // namespace bm
