// sunfield.hip -- builds the sun plane, the ninth plane of the cube field that shadow rays read (sunfield.h: the plan of a sun, the
// recurrences of the bytes and of the clear heights), from the index grid, the column tops and the escape table that escape.hip keeps:
// slab by slab along the cone's dominant axis, from the far end of the grid to the near one, two small kernels per slab --
//   1. clear heights of the slab's columns (D horizontal) and with them the first stamped cell of every column;
//   2. the face values of the slab's cells, one lane per (cell, bin, bin), and the cells' bytes: the sixteen lanes of a cell each take
//      a part of the bins a ray can leave the cell in and fold their minima.
// The whole plane is rebuilt when the world or the sun has changed and a frame is about to use it (scene.cpp ensure_sun_plane): on a
// 1024^3 world 2 x 128 launches; the cost is in profiles/r09_sunfield.txt.
#include <hip/hip_runtime.h>

#include "escape.h"
#include "global_mem.h"
#include "kernels.h"
#include "sunfield.h"

namespace bm {
namespace {

static_assert(kSunBins == 4, "sixteen lanes per cell: the fold below and the split of the leaving bins");

struct SunTmp { // the build's scratch, carved from one buffer (sun_build_tmp_bytes)
	int32_t* stamped;   // [cells y][cells x]: first z cell of the column that reads 255
	int32_t* clear[2];  // [n1][bins]: clear heights of the slab before / the slab being built
	uint8_t* face[2];   // [n2][n1][bins][bins]: face values likewise
};
__host__ __device__ inline SunTmp sun_tmp(uint8_t* tmp, const SunBuild& u) {
	const size_t n1 = static_cast<size_t>(u.n1), n2 = static_cast<size_t>(u.n2);
	SunTmp t;
	t.stamped = reinterpret_cast<int32_t*>(tmp);
	t.clear[0] = t.stamped + static_cast<size_t>(u.cells) * u.cells;
	t.clear[1] = t.clear[0] + n1 * kSunBins;
	t.face[0] = reinterpret_cast<uint8_t*>(t.clear[1] + n1 * kSunBins);
	t.face[1] = t.face[0] + n1 * n2 * kSunBins * kSunBins;
	return t;
}

// the cell at directed position (ud, v1, v2) of (D, m1, m2): m1 is x unless D is, m2 is z unless D is (sunfield.h)
__device__ __forceinline__ void sun_cell(const SunBuild& u, int ud, int v1, int v2, int& x, int& y, int& z) {
	const SunPlan& p = u.plan;
	const int cd = sun_coord(p, p.dom, u.nd, ud), c1 = sun_coord(p, p.m1, u.n1, v1), c2 = sun_coord(p, p.m2, u.n2, v2);
	x = p.dom == 0 ? cd : c1;
	y = p.dom == 1 ? cd : (p.dom == 0 ? c1 : c2);
	z = p.dom == 2 ? cd : c2;
}

__device__ __forceinline__ int quadrant_threshold(const uint32_t* escape, const SunBuild& u, int x, int y) {
	return escape_height_of(u.plan.octant, ld32(escape, escape_index(u.plan.octant, u.cf_shift, u.cf_pxy, x, y)), u.cf_pxy, u.cf_plane);
}

// D = z: the quadrant rule alone stamps.  One lane per column.
__global__ void sun_stamp_quadrant(const uint32_t* __restrict__ escape, int32_t* __restrict__ stamped, const SunBuild u) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= static_cast<uint32_t>(u.cells) * static_cast<uint32_t>(u.cells)) return;
	const int x = static_cast<int>(t % static_cast<uint32_t>(u.cells)), y = static_cast<int>(t / static_cast<uint32_t>(u.cells));
	((g_i32*)stamped)[t] = sun_first_stamped(1 << 20, quadrant_threshold(escape, u, x, y));
}

// clear heights of slab `ud`: one lane per (w, bin); bin 0 also settles the column
__global__ void sun_clear_slab(const int32_t* __restrict__ cols, const uint32_t* __restrict__ escape, int32_t* __restrict__ stamped, const int32_t* __restrict__ cn,
							   int32_t* __restrict__ cc, const SunBuild u, const int ud) {
	const SunPlan& p = u.plan;
	const int n1 = u.n1;
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= static_cast<uint32_t>(n1) * kSunBins) return;
	const int w = static_cast<int>(t / kSunBins), b = static_cast<int>(t % kSunBins);
	auto column = [&](int ww, int& x, int& y) { int z; sun_cell(u, ud, ww, 0, x, y, z); }; // (D and m1 are x and y, in either order)
	auto height = [&](int ww) {
		if (ww >= n1) return 0;
		int x, y; column(ww, x, y);
		return (ldi32(cols, static_cast<size_t>(y) * u.cells + x) + 1) * kSunHeightUnit; // (escape.hip escape_columns: top, -1 for an empty column)
	};
	auto next = [&](int ww, int bb) { return ww < n1 ? ldi32(cn, static_cast<size_t>(ww) * kSunBins + bb) : 0; };
	((g_i32*)cc)[t] = sun_clear_face_value(p, w, b, height, next);
	if (b == 0) {
		int x, y; column(w, x, y);
		((g_i32*)stamped)[static_cast<size_t>(y) * u.cells + x] = sun_first_stamped(sun_clear_cell(p, w, height, next), quadrant_threshold(escape, u, x, y));
	}
}

// face values and bytes of slab `ud`: lane t = ((u2 * n1 + u1) * bins + b2) * bins + b1
__global__ void sun_field_slab(const uint32_t* __restrict__ index_grid, const int32_t* __restrict__ stamped, const uint8_t* __restrict__ fn, uint8_t* __restrict__ fc,
							   uint8_t* __restrict__ field, const SunBuild u, const int ud) {
	const SunPlan& p = u.plan;
	const int n1 = u.n1, n2 = u.n2;
	const uint32_t total = static_cast<uint32_t>(n1) * static_cast<uint32_t>(n2) * (kSunBins * kSunBins);
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = t < total; // (a cell's sixteen lanes are live together; the fold below needs every lane of the wave to get there)
	const uint32_t cell = (live ? t : 0u) / (kSunBins * kSunBins);
	const int b1 = static_cast<int>(t % kSunBins), b2 = static_cast<int>(t / kSunBins % kSunBins);
	const int u1 = static_cast<int>(cell % static_cast<uint32_t>(n1)), u2 = static_cast<int>(cell / static_cast<uint32_t>(n1));
	auto blocked = [&](int v1, int v2) {
		if (v1 >= n1 || v2 >= n2) return true;
		int x, y, z; sun_cell(u, ud, v1, v2, x, y, z);
		return ld32(index_grid, index_word_at(u.sg_xy, u.sg_xy2, x, y, z)) != 0u;
	};
	auto next = [&](int v1, int v2, int g1, int g2) {
		return v1 < n1 && v2 < n2 ? static_cast<int>(ld8(fn, ((static_cast<size_t>(v2) * n1 + v1) * kSunBins + g2) * kSunBins + g1)) : 0;
	};
	if (live) st8(fc, t, static_cast<uint32_t>(sun_face_value(p, u1, u2, b1, b2, blocked, next)));
	// the byte: sun_cell_byte's minimum over the leaving bins 0 ... bins - 1 + hi, two values of either axis per lane
	const int last1 = kSunBins - 1 + p.hi1, last2 = kSunBins - 1 + p.hi2;
	int part = 254;
	if (live && 2 * b1 <= last1 && 2 * b2 <= last2)
		part = sun_slab_value(u1, u2, 2 * b1, 2 * b1 + 1 < last1 ? 2 * b1 + 1 : last1, 2 * b2, 2 * b2 + 1 < last2 ? 2 * b2 + 1 : last2, [](int, int) { return false; }, next);
	for (int off = 1; off < kSunBins * kSunBins; off <<= 1) { const int o = __shfl_xor(part, off, 64); part = o < part ? o : part; }
	if (live && b1 == 0 && b2 == 0) {
		int x, y, z; sun_cell(u, ud, u1, u2, x, y, z);
		const bool rect = blocked(u1 + 1, u2) || blocked(u1, u2 + 1) || blocked(u1 + 1, u2 + 1); // (hi >= 1 on both axes: the 2 x 2 cells)
		uint32_t v = rect ? 1u : static_cast<uint32_t>(part);
		v = z >= ldi32(stamped, static_cast<size_t>(y) * u.cells + x) ? 255u : v;
		v = blocked(u1, u2) ? 0u : v;
		st8(field, 8ull * u.cf_plane + static_cast<size_t>(z + 1) * u.cf_pxy + (static_cast<size_t>(y + 1) << u.cf_shift) + static_cast<size_t>(x + 1), v);
	}
}

} // namespace

size_t sun_build_tmp_bytes(const SunBuild& u) {
	const size_t n1 = static_cast<size_t>(u.n1), n2 = static_cast<size_t>(u.n2);
	return (static_cast<size_t>(u.cells) * u.cells + 2 * n1 * kSunBins) * sizeof(int32_t) + 2 * n1 * n2 * kSunBins * kSunBins; // sun_tmp
}

void launch_sun_build(const uint32_t* index_grid, const int32_t* cols, const uint32_t* escape, uint8_t* field, uint8_t* tmp, const SunBuild& u, hipStream_t stream) {
	const SunPlan& p = u.plan;
	const SunTmp t = sun_tmp(tmp, u);
	const int nd = u.nd;
	const uint32_t columns = static_cast<uint32_t>(u.cells) * static_cast<uint32_t>(u.cells), clear_lanes = static_cast<uint32_t>(u.n1) * kSunBins;
	const size_t face_bytes = static_cast<size_t>(t.face[1] - t.face[0]);
	const uint32_t face_lanes = static_cast<uint32_t>(face_bytes);
	// behind the far end of the grid: face values 0 (outside counts as occupied), clear heights 0
	(void)hipMemsetAsync(t.clear[0], 0, clear_lanes * sizeof(int32_t), stream);
	(void)hipMemsetAsync(t.face[0], 0, face_bytes, stream);
	if (!p.clear) hipLaunchKernelGGL(sun_stamp_quadrant, dim3((columns + 63) / 64), dim3(64), 0, stream, escape, t.stamped, u);
	for (int ud = nd - 1, k = 0; ud >= 0; --ud, k ^= 1) {
		if (p.clear) hipLaunchKernelGGL(sun_clear_slab, dim3((clear_lanes + 63) / 64), dim3(64), 0, stream, cols, escape, t.stamped, t.clear[k], t.clear[k ^ 1], u, ud);
		hipLaunchKernelGGL(sun_field_slab, dim3((face_lanes + 255) / 256), dim3(256), 0, stream, index_grid, t.stamped, t.face[k], t.face[k ^ 1], field, u, ud);
	}
}

} // namespace bm
