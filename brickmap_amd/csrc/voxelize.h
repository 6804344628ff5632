// voxelize.h -- the rules of mesh voxelization (bm_voxelize, include/brickmap.h), written once for the kernels of voxelize.hip and
// the plain loops of voxelize_host.cpp.  Needs no HIP header: tests/voxelize_check.cpp builds it with a host compiler.
//
// Floats end at the snap: a vertex becomes an integer q in 1/256 voxel relative to the volume's origin, and every test below is an
// inequality of 64-bit integers, so every evaluation order gives the same bits.  Bounds (vx_snap refuses what exceeds them): |q| <= 2^22
// and an extent of at most 2^19 per axis, so an edge is below 2^20, a normal component below 2^40, and every sum of three products
// n_a * (k_a S - q_a) with k within 8 voxels of the triangle's bounds is below 2^62.
#pragma once
#include <cstdint>

#include "device_types.h"

namespace bm {

constexpr int kVxS = 256;                       // snapped units per voxel
constexpr int64_t kVxMaxQ = int64_t{1} << 22;   // |q|
constexpr int64_t kVxMaxSpan = int64_t{1} << 19; // max q - min q per axis: 2048 voxels
constexpr int kVxMaxExtent = 16384;             // voxels per axis of the volume
constexpr int64_t kVxMaxTriangles = int64_t{1} << 30;
constexpr uint32_t kVxSurface = 1, kVxSolid = 2; // BM_VOXELIZE_SURFACE, BM_VOXELIZE_SOLID
constexpr uint32_t kVxKeep = 1;                 // BM_VOXELIZE_KEEP
constexpr int kVxOk = 0, kVxRejected = 1, kVxDegenerate = 2;

struct VxParamsView {
	int32_t lo[3], extent[3];
	int64_t row_pitch, slice_pitch;
	uint32_t mode, flags;
};

// the view of a bm_voxelize_params (a template, so that this header needs no other)
template <class P>
inline VxParamsView voxelize_params_view(const P& p) {
	return {{p.lo[0], p.lo[1], p.lo[2]}, {p.extent[0], p.extent[1], p.extent[2]}, p.row_pitch, p.slice_pitch, p.mode, p.flags};
}

// null, or why bm_voxelize and bm_host_voxelize refuse these parameters (pitches as given: 0 = tight)
inline const char* voxelize_params_problem(const VxParamsView& p, int64_t n) {
	for (int k = 0; k < 3; ++k)
		if (p.extent[k] < 1 || p.extent[k] > kVxMaxExtent) return "an extent below 1 or above 16384";
	if (p.mode == 0 || (p.mode & ~(kVxSurface | kVxSolid))) return "unknown mode";
	if (p.flags & ~kVxKeep) return "unknown flag";
	if (p.row_pitch < 0 || p.slice_pitch < 0) return "negative pitch";
	if (p.row_pitch > (int64_t{1} << 40)) return "row_pitch above 2^40";
	const int64_t row = p.row_pitch ? p.row_pitch : p.extent[0];
	if (row < p.extent[0]) return "row_pitch below the extent along x";
	if (p.slice_pitch && p.slice_pitch / p.extent[1] < row) return "slice_pitch below row_pitch * the extent along y";
	if ((p.slice_pitch ? p.slice_pitch : row * p.extent[1]) > (int64_t{1} << 46) / p.extent[2]) return "a volume spanning more than 2^46 bytes";
	if (n < 0 || n > kVxMaxTriangles) return "a triangle count below 0 or above 2^30";
	return nullptr;
}
inline int64_t voxelize_row_pitch(const VxParamsView& p) { return p.row_pitch ? p.row_pitch : p.extent[0]; }
inline int64_t voxelize_slice_pitch(const VxParamsView& p) { return p.slice_pitch ? p.slice_pitch : voxelize_row_pitch(p) * p.extent[1]; }
// words of one row of a bit plane: bit x of the row for voxel x, and bit nx for the crossings beyond the volume
inline uint32_t voxelize_row_words(int nx) { return static_cast<uint32_t>(nx + 1 + 31) / 32u; }

// accepted parameters as the kernels and voxelize_workspace_bytes take them (kernels.h): a kernel argument, passed by value
struct VoxelizeDims {
	int32_t lo[3], extent[3];
	uint32_t words; // voxelize_row_words(extent[0])
	uint32_t mode, keep;
	int64_t row_pitch, slice_pitch; // resolved: never 0
};
inline VoxelizeDims voxelize_dims(const VxParamsView& p) {
	VoxelizeDims d;
	for (int k = 0; k < 3; ++k) { d.lo[k] = p.lo[k]; d.extent[k] = p.extent[k]; }
	d.words = voxelize_row_words(p.extent[0]);
	d.mode = p.mode;
	d.keep = p.flags & kVxKeep;
	d.row_pitch = voxelize_row_pitch(p);
	d.slice_pitch = voxelize_slice_pitch(p);
	return d;
}

// a snapped triangle: q[vertex][axis], its normal, and its bounds per axis
struct VxTri {
	int32_t q[3][3];
	int64_t n[3];
	int32_t mn[3], mx[3];
};

BM_VHD int64_t vx_max0(int64_t v) { return v > 0 ? v : 0; }
BM_VHD int64_t vx_min0(int64_t v) { return v < 0 ? v : 0; }
// floor(a / b), b > 0
BM_VHD int64_t vx_floor_div(int64_t a, int64_t b) {
	const int64_t q = a / b;
	return q * b > a ? q - 1 : q;
}

// snap the 9 floats of a triangle (xyz per vertex, world voxel units) about the volume's origin lo
BM_VHD int vx_snap(const float* v, const int32_t lo[3], VxTri& t) {
	bool ok = true;
	for (int i = 0; i < 3; ++i)
		for (int a = 0; a < 3; ++a) {
			const float p = v[3 * i + a] * 256.0f; // exact, or infinite
			int64_t q = 0;
			if (!(__builtin_fabsf(p) <= 1073741824.0f)) { // also a NaN
				ok = false;
			} else {
				q = static_cast<int64_t>(__builtin_rintf(p)) - int64_t{256} * lo[a]; // half to even
				if (q > kVxMaxQ || q < -kVxMaxQ) { ok = false; q = 0; }
			}
			t.q[i][a] = static_cast<int32_t>(q);
		}
	for (int a = 0; a < 3; ++a) {
		const int32_t q0 = t.q[0][a], q1 = t.q[1][a], q2 = t.q[2][a];
		t.mn[a] = q0 < q1 ? (q0 < q2 ? q0 : q2) : (q1 < q2 ? q1 : q2);
		t.mx[a] = q0 > q1 ? (q0 > q2 ? q0 : q2) : (q1 > q2 ? q1 : q2);
		if (static_cast<int64_t>(t.mx[a]) - t.mn[a] > kVxMaxSpan) ok = false;
	}
	if (!ok) return kVxRejected;
	const int64_t e1[3] = {int64_t{t.q[1][0]} - t.q[0][0], int64_t{t.q[1][1]} - t.q[0][1], int64_t{t.q[1][2]} - t.q[0][2]};
	const int64_t e2[3] = {int64_t{t.q[2][0]} - t.q[0][0], int64_t{t.q[2][1]} - t.q[0][1], int64_t{t.q[2][2]} - t.q[0][2]};
	t.n[0] = e1[1] * e2[2] - e1[2] * e2[1];
	t.n[1] = e1[2] * e2[0] - e1[0] * e2[2];
	t.n[2] = e1[0] * e2[1] - e1[1] * e2[0];
	return (t.n[0] | t.n[1] | t.n[2]) == 0 ? kVxDegenerate : kVxOk;
}

// ---- surface
// the voxels of axis a that pass test 1, clipped to [0, extent): k0 <= k <= k1 (empty when k0 > k1)
BM_VHD void vx_surface_range(const VxTri& t, int a, int extent, int& k0, int& k1) {
	k0 = ((t.mn[a] + (kVxS - 1)) >> 8) - 1; // the smallest k with (k + 1) S >= min
	k1 = t.mx[a] >> 8;                     // the largest k with k S <= max
	if (k0 < 0) k0 = 0;
	if (k1 > extent - 1) k1 = extent - 1;
}

// test 2 for the cube [k S, (k + size) S]^3: the triangle's plane meets it.  size = 1 is a voxel; a larger cube that fails holds no
// voxel that passes
BM_VHD bool vx_plane_meets(const VxTri& t, int kx, int ky, int kz, int size) {
	const int64_t S = kVxS, W = S * size;
	const int64_t d = t.n[0] * (kx * S - t.q[0][0]) + t.n[1] * (ky * S - t.q[0][1]) + t.n[2] * (kz * S - t.q[0][2]);
	const int64_t lo = vx_min0(t.n[0] * W) + vx_min0(t.n[1] * W) + vx_min0(t.n[2] * W);
	const int64_t hi = vx_max0(t.n[0] * W) + vx_max0(t.n[1] * W) + vx_max0(t.n[2] * W);
	return d + lo <= 0 && 0 <= d + hi;
}

// test 3 for one axis: the voxel's square in the plane (u, v) meets the triangle's projection
BM_VHD bool vx_projection_meets(const VxTri& t, int ax, const int k[3]) {
	const int u = ax == 2 ? 0 : ax + 1, v = ax == 0 ? 2 : ax - 1;
	// an edge component is below 2^20, k S - p0 below 2^24 for a voxel within the volume: factors of 32 bits, products of 64
	const int32_t S = kVxS, sgn = t.n[ax] >= 0 ? 1 : -1;
	const int32_t ku = k[u] * S, kv = k[v] * S;
	bool in = true;
	for (int i = 0; i < 3; ++i) {
		const int j = i == 2 ? 0 : i + 1;
		const int32_t a = -(t.q[j][v] - t.q[i][v]) * sgn, b = (t.q[j][u] - t.q[i][u]) * sgn;
		const int32_t c = (a > 0 ? a * S : 0) + (b > 0 ? b * S : 0);
		in = in && static_cast<int64_t>(a) * (ku - t.q[i][u]) + static_cast<int64_t>(b) * (kv - t.q[i][v]) + c >= 0;
	}
	return in;
}

// tests 1, 2 and 3 of voxel (kx, ky, kz)
BM_VHD bool vx_surface_voxel(const VxTri& t, int kx, int ky, int kz) {
	const int k[3] = {kx, ky, kz};
	for (int a = 0; a < 3; ++a)
		if (!(k[a] * kVxS <= t.mx[a] && (k[a] + 1) * kVxS >= t.mn[a])) return false;
	return vx_plane_meets(t, kx, ky, kz, 1) && vx_projection_meets(t, 0, k) && vx_projection_meets(t, 1, k) && vx_projection_meets(t, 2, k);
}

// voxels x8 ... x8 + 7 of row (y, z): bit i = vx_surface_voxel(t, x8 + i, y, z), with what does not depend on x taken once
BM_VHD uint32_t vx_surface_row8(const VxTri& t, int x8, int y, int z) {
	if (!(y * kVxS <= t.mx[1] && (y + 1) * kVxS >= t.mn[1] && z * kVxS <= t.mx[2] && (z + 1) * kVxS >= t.mn[2])) return 0;
	const int k0[3] = {x8, y, z};
	if (!vx_projection_meets(t, 0, k0)) return 0;
	uint32_t m = 0;
	for (int i = 0; i < 8; ++i) {
		const int k[3] = {x8 + i, y, z};
		const bool in = k[0] * kVxS <= t.mx[0] && (k[0] + 1) * kVxS >= t.mn[0] && vx_plane_meets(t, k[0], y, z, 1) && vx_projection_meets(t, 1, k) &&
						vx_projection_meets(t, 2, k);
		m |= (in ? 1u : 0u) << i;
	}
	return m;
}

// ---- solid
// the columns of axis a (1 = y, 2 = z) whose centre lies inside the triangle's bounds, clipped to [0, extent)
BM_VHD void vx_solid_range(const VxTri& t, int a, int extent, int& k0, int& k1) {
	k0 = (t.mn[a] - 128 + (kVxS - 1)) >> 8; // the smallest k with 256 k + 128 >= min
	k1 = (t.mx[a] - 128) >> 8;             // the largest k with 256 k + 128 <= max
	if (k0 < 0) k0 = 0;
	if (k1 > extent - 1) k1 = extent - 1;
}

// column (y, z) of a triangle with n_x != 0: covered or not; when covered, *k = the crossing's position clamped to [0, nx]
BM_VHD bool vx_solid_crossing(const VxTri& t, int y, int z, int nx, int* k) {
	const int32_t sgn = t.n[0] > 0 ? 1 : -1;
	const int32_t U = 256 * y + 128, V = 256 * z + 128;
	bool covered = true;
	for (int i = 0; i < 3; ++i) {
		const int j = i == 2 ? 0 : i + 1;
		const int32_t a = -(t.q[j][2] - t.q[i][2]) * sgn, b = (t.q[j][1] - t.q[i][1]) * sgn; // (factors of 32 bits, as in vx_projection_meets)
		const int64_t E = static_cast<int64_t>(a) * (U - t.q[i][1]) + static_cast<int64_t>(b) * (V - t.q[i][2]);
		covered = covered && (E > 0 || (E == 0 && (a > 0 || (a == 0 && b > 0))));
	}
	if (!covered) return false;
	// the smallest x with |n_x| (256 x + 128 - q0_x) >= R
	const int64_t A = t.n[0] * sgn;
	const int64_t R = -sgn * (t.n[1] * (U - t.q[0][1]) + t.n[2] * (V - t.q[0][2]));
	const int64_t c = -vx_floor_div(-R, A) + t.q[0][0] - 128; // 256 x >= ceil(R / A) + q0_x - 128
	const int64_t x = -vx_floor_div(-c, 256);
	*k = x < 0 ? 0 : (x > nx ? nx : static_cast<int>(x));
	return true;
}

// the prefix parity of a word of crossings: bit x of the result = the parity of bits 0 ... x
BM_VHD uint32_t vx_prefix_xor(uint32_t w) {
	w ^= w << 1;
	w ^= w << 2;
	w ^= w << 4;
	w ^= w << 8;
	w ^= w << 16;
	return w;
}

} // namespace bm
