// sunfield.hip -- builds the sun plane, the ninth plane of the cube field that shadow rays read (sunfield.h: the plan of a sun, the
// recurrences of the bytes and of the clear heights), from the index grid, the column tops and the escape table that escape.hip keeps:
// slab by slab along the cone's dominant axis, from the far end of the grid to the near one, two small kernels per slab --
//   1. clear heights of the slab's columns (D horizontal) and with them the first stamped cell of every column;
//   2. the face values of the slab's cells, one lane per (cell, bin, bin), and the cells' bytes: the sixteen lanes of a cell each take
//      a part of the bins a ray can leave the cell in and fold their minima.
// The shadow heights (shadowheight.h) ride on kernel 1: the same lanes, one (column, bin) each, carry the recurrence of S beside that of the
// clear heights and write slice 8 of the escape table; a column scan before the first slab counts every column's full bricks.
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
struct ShadowTmp { // the shadow heights' scratch, a buffer of its own (shadow_build_tmp_bytes)
	int32_t* full;      // [cells y][cells x]: full_top * kSunHeightUnit of the column (shadowheight.h)
	int32_t* shade[2];  // [n1][bins]: S of the slab before / the slab being built
};
__host__ __device__ inline ShadowTmp shadow_tmp(uint8_t* tmp, const SunBuild& u) {
	ShadowTmp t;
	t.full = reinterpret_cast<int32_t*>(tmp);
	t.shade[0] = t.full + static_cast<size_t>(u.cells) * u.cells;
	t.shade[1] = t.shade[0] + static_cast<size_t>(u.n1) * kSunBins;
	return t;
}
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

// full tops: one lane per column of the box fx0 ... fx1 x fy0 ... fy1, upwards from z = 0 while the cell's brick is resident and has every bit set
__global__ void shadow_full_tops(const uint32_t* __restrict__ index_grid, const uint32_t* __restrict__ pool_base, const uint32_t* __restrict__ arena, int32_t* __restrict__ full,
								 const SunBuild u) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t nx = static_cast<uint32_t>(u.fx1 - u.fx0), ny = static_cast<uint32_t>(u.fy1 - u.fy0);
	if (t >= nx * ny) return;
	const int x = u.fx0 + static_cast<int>(t % nx), y = u.fy0 + static_cast<int>(t / nx);
	int z = 0;
	for (; z < u.cells_height; ++z) {
		const uint32_t word = ld32(index_grid, index_word_at(u.sg_xy, u.sg_xy2, x, y, z));
		if (!(word & kLoadedBit) || (word & 0xFF000u) != 0xFF000u) break; // resident, and solid at the 2^3 level of detail as well (the word's eight LoD bits)
		const size_t first = brick_first_word(ld32(pool_base, supercell_of(u.sg_xy, u.sg_xy2, x, y, z)), word);
		uint32_t all = 0xFFFFFFFFu;
		for (int k = 0; k < 4; ++k) { const u32x4 v = ld128(arena, static_cast<int64_t>((first + 4 * k) * sizeof(uint32_t))); all &= v.x & v.y & v.z & v.w; }
		if (all != 0xFFFFFFFFu) break;
	}
	((g_i32*)full)[static_cast<size_t>(y) * u.cells + x] = z * kSunHeightUnit;
}

// clear heights of slab `ud`: one lane per (w, bin); bin 0 also settles the column.  CLEAR: false = the shadow heights alone.
// SHADE: the shadow heights of the slab as well (shadowheight.h): S into sc, the column's entry into slice 8 of the escape table.
template <bool CLEAR, bool SHADE>
__global__ void sun_clear_slab(const int32_t* __restrict__ cols, uint32_t* __restrict__ escape, int32_t* __restrict__ stamped, const int32_t* __restrict__ cn,
							   int32_t* __restrict__ cc, const int32_t* __restrict__ full, const int32_t* __restrict__ sn, int32_t* __restrict__ sc, const SunBuild u, const int ud) {
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
	if (CLEAR) {
		((g_i32*)cc)[t] = sun_clear_face_value(p, w, b, height, next);
		if (b == 0) {
			int x, y; column(w, x, y);
			((g_i32*)stamped)[static_cast<size_t>(y) * u.cells + x] = sun_first_stamped(sun_clear_cell(p, w, height, next), quadrant_threshold(escape, u, x, y));
		}
	}
	if (SHADE) {
		auto shade_next = [&](int ww, int bb) { return ww < n1 ? ldi32(sn, static_cast<size_t>(ww) * kSunBins + bb) : 0; };
		int x, y; column(w, x, y);
		((g_i32*)sc)[t] = shadow_face_value(u.shadow, w, b, ldi32(full, static_cast<size_t>(y) * u.cells + x), shade_next);
		if (b == 0) st32(escape, escape_index(8, u.cf_shift, u.cf_pxy, x, y), shadow_entry(8u * u.cf_plane, u.cf_pxy, shadow_dark_cells(u.shadow, w, u.cells_height, shade_next)));
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
size_t shadow_build_tmp_bytes(const SunBuild& u) {
	return (static_cast<size_t>(u.cells) * u.cells + 2 * static_cast<size_t>(u.n1) * kSunBins) * sizeof(int32_t); // shadow_tmp
}

void launch_sun_build(const uint32_t* index_grid, const uint32_t* pool_base, const uint32_t* arena, const int32_t* cols, uint32_t* escape, uint8_t* field, uint8_t* tmp,
					  uint8_t* tmp_shadow, const SunBuild& u, bool with_field, hipStream_t stream) {
	const SunPlan& p = u.plan;
	const SunTmp t = sun_tmp(tmp, u);
	const ShadowTmp h = shadow_tmp(tmp_shadow, u);
	const int nd = u.nd;
	const uint32_t columns = static_cast<uint32_t>(u.cells) * static_cast<uint32_t>(u.cells), clear_lanes = static_cast<uint32_t>(u.n1) * kSunBins;
	const size_t face_bytes = static_cast<size_t>(t.face[1] - t.face[0]);
	const uint32_t face_lanes = static_cast<uint32_t>(face_bytes);
	const bool shade = BM_SHADOWHEIGHT != 0 && u.shadow.valid != 0; // (valid: the plan has clear heights, so every slab has a sun_clear_slab launch)
	// behind the far end of the grid: face values 0 (outside counts as occupied), clear heights 0, shadow values 0
	if (with_field) {
		(void)hipMemsetAsync(t.clear[0], 0, clear_lanes * sizeof(int32_t), stream);
		(void)hipMemsetAsync(t.face[0], 0, face_bytes, stream);
		if (!p.clear) hipLaunchKernelGGL(sun_stamp_quadrant, dim3((columns + 63) / 64), dim3(64), 0, stream, escape, t.stamped, u);
	}
	if (BM_SHADOWHEIGHT != 0) {
		if (shade) {
			(void)hipMemsetAsync(h.shade[0], 0, clear_lanes * sizeof(int32_t), stream);
			const uint32_t scanned = static_cast<uint32_t>(u.fx1 - u.fx0) * static_cast<uint32_t>(u.fy1 - u.fy0);
			if (scanned) hipLaunchKernelGGL(shadow_full_tops, dim3((scanned + 63) / 64), dim3(64), 0, stream, index_grid, pool_base, arena, h.full, u);
		} else {
			(void)hipMemsetAsync(escape + escape_entries(u.cf_pxy), 0, static_cast<size_t>(u.cf_pxy) * sizeof(uint32_t), stream); // no shadow heights for this sun
		}
	}
	const dim3 cg((clear_lanes + 63) / 64), cb(64);
	for (int ud = nd - 1, k = 0; ud >= 0; --ud, k ^= 1) {
		if (with_field && p.clear && shade) hipLaunchKernelGGL((sun_clear_slab<true, true>), cg, cb, 0, stream, cols, escape, t.stamped, t.clear[k], t.clear[k ^ 1], h.full, h.shade[k], h.shade[k ^ 1], u, ud);
		else if (with_field && p.clear) hipLaunchKernelGGL((sun_clear_slab<true, false>), cg, cb, 0, stream, cols, escape, t.stamped, t.clear[k], t.clear[k ^ 1], h.full, h.shade[k], h.shade[k ^ 1], u, ud);
		else if (shade) hipLaunchKernelGGL((sun_clear_slab<false, true>), cg, cb, 0, stream, cols, escape, t.stamped, t.clear[k], t.clear[k ^ 1], h.full, h.shade[k], h.shade[k ^ 1], u, ud);
		if (with_field) hipLaunchKernelGGL(sun_field_slab, dim3((face_lanes + 255) / 256), dim3(256), 0, stream, index_grid, t.stamped, t.face[k], t.face[k ^ 1], field, u, ud);
	}
}

} // namespace bm
