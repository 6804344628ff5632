// edit.hip -- device half of a voxel edit (bm_scene_edit, scene.cpp "voxel edits"): one scatter of the batch's dirty bricks and
// index words, then the part of the octant cube field that the batch can change, recomputed on the GPU.
//
// The cube field (world.cpp build_cube_field) is a DP over the grid; what it computes is, for a cell c of plane o,
//   E(c) = min(254, D(c)),  D(c) = min over occupied cells q in c's cone of max_k |q_k - c_k|
// (the cone: q - c has the sign of octant o's direction on every axis, or 0; the border counts as occupied, an occupied c gives 0).
// A cube of edge n anchored at c is empty iff no occupied cell of the cone lies within L-infinity distance n - 1, hence the form.
// min and max distribute, so D splits into three 1-D passes along the lines of the grid:
//   a1 = distance along x to the nearest occupied cell,  a2(y) = min_j max(j, a1(y + j dy)),  D(z) = min_l max(l, a2(z + l dz))
// -- two x passes (the x direction), four y passes (x and y directions), eight z passes (the planes).  Every value is capped at 254, so
// a cell more than 254 cells away (on some axis) from every cell whose occupancy changed keeps its value: the update covers the
// changed cells' bounding box grown by 254 cells on every side, clipped to the grid (FieldUpdate, kernels.h).
#include <hip/hip_runtime.h>

#include "global_mem.h"
#include "kernels.h"

namespace bm {
namespace {

constexpr int kFieldCap = 254; // largest cube edge the field stores (world.cpp)

// 16 lanes per dirty cell: its brick (when it has an arena slot) and its index word
__global__ void edit_scatter(const uint32_t* __restrict__ cells, const uint32_t* __restrict__ words, const uint32_t* __restrict__ slots,
							 const uint32_t* __restrict__ bricks, uint32_t count, uint32_t* __restrict__ index_grid, uint32_t* __restrict__ arena) {
	const uint32_t i = blockIdx.x * (blockDim.x / 16) + threadIdx.x / 16;
	const uint32_t w = threadIdx.x & 15;
	if (i >= count) return;
	const uint32_t slot = ld32(slots, i);
	if (slot != 0xFFFFFFFFu) st32(arena, (static_cast<size_t>(slot) << 4) + w, ld32(bricks, (static_cast<size_t>(i) << 4) + w));
	if (w == 0) st32(index_grid, ld32(cells, i), ld32(words, i));
}

// is the brick cell at bordered coordinates (x, y, z) (1 ... cells) occupied, i.e. is its index word non-zero?
__device__ __forceinline__ bool occupied(const uint32_t* index_grid, const FieldUpdate& u, int x, int y, int z) {
	// index_word_at (device_types.h), written out: here the supercell is computed in 64 bits, and the pass is compiled from that
	const uint32_t cx = x - 1, cy = y - 1, cz = z - 1;
	const size_t sc = (cx >> 4) + (cy >> 4) * static_cast<size_t>(u.sg_xy) + (cz >> 4) * static_cast<size_t>(u.sg_xy2);
	return ld32(index_grid, (sc << 12) + ((cx & 15) | ((cy & 15) << 4) | ((cz & 15) << 8))) != 0;
}

// x pass: one lane per line (x direction v, slice z, row y), scanned from the far end of what the box needs towards the near end
__global__ void field_pass_x(const uint32_t* __restrict__ index_grid, uint8_t* __restrict__ a1, const FieldUpdate u) {
	const uint32_t ny = u.ay1 - u.ay0, nz = u.bz1 - u.bz0, nx = u.rx1 - u.rx0;
	const uint64_t lines = 2ull * ny * nz;
	for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < lines; t += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
		const int y = u.ay0 + static_cast<int>(t % ny);
		const uint64_t r = t / ny;
		const int z = u.bz0 + static_cast<int>(r % nz);
		const int v = static_cast<int>(r / nz);
		const size_t row = ((static_cast<size_t>(v) * nz + (z - u.bz0)) * ny + (y - u.ay0)) * nx;
		// the value behind the first cell scanned: 0 at the border, else "254 or more" (anything further is more than 254 cells
		// from every cell of the box)
		int x, end, step, run;
		if (v == 0) { x = min(u.cells, u.rx1 - 1 + kFieldCap); run = x == u.cells ? 0 : kFieldCap; end = u.rx0 - 1; step = -1; }
		else { x = max(1, u.rx0 - kFieldCap); run = x == 1 ? 0 : kFieldCap; end = u.rx1; step = 1; }
		for (; x != end; x += step) {
			run = occupied(index_grid, u, x, y, z) ? 0 : min(kFieldCap, run + 1);
			if (x >= u.rx0 && x < u.rx1) st8(a1, row + (x - u.rx0), run);
		}
	}
}

// y pass: one lane per cell (x and y directions v, slice z of the z range, row y and column x of the box)
__global__ void field_pass_y(const uint8_t* __restrict__ a1, uint8_t* __restrict__ a2, const FieldUpdate u) {
	const uint32_t nx = u.rx1 - u.rx0, ny = u.ry1 - u.ry0, nz = u.bz1 - u.bz0, nya = u.ay1 - u.ay0;
	const uint64_t n = 4ull * nx * ny * nz;
	for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n; t += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
		const int x = static_cast<int>(t % nx);
		uint64_t r = t / nx;
		const int y = u.ry0 + static_cast<int>(r % ny);
		r /= ny;
		const int zz = static_cast<int>(r % nz);
		const int v = static_cast<int>(r / nz);
		const int dy = (v & 2) ? -1 : 1;
		const size_t line = ((static_cast<size_t>(v & 1) * nz + zz) * nya) * nx + x; // a1 at (row u.ay0, this column)
		int best = static_cast<int>(ld8(a1, line + static_cast<size_t>(y - u.ay0) * nx));
		for (int k = 1; k < best; ++k) {
			const int yy = y + k * dy;
			if (yy < 1 || yy > u.cells) { best = k; break; } // the border: occupied
			best = min(best, max(k, static_cast<int>(ld8(a1, line + static_cast<size_t>(yy - u.ay0) * nx))));
		}
		st8(a2, ((static_cast<size_t>(v) * nz + zz) * ny + (y - u.ry0)) * nx + x, best);
	}
}

// z pass: one lane per cell of the box and plane o; writes the device field (rows padded to 2^cf_shift bytes)
__global__ void field_pass_z(const uint8_t* __restrict__ a2, uint8_t* __restrict__ field, const FieldUpdate u) {
	const uint32_t nx = u.rx1 - u.rx0, ny = u.ry1 - u.ry0, nz = u.rz1 - u.rz0, nzb = u.bz1 - u.bz0;
	const uint64_t n = 8ull * nx * ny * nz;
	for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n; t += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
		const int x = static_cast<int>(t % nx);
		uint64_t r = t / nx;
		const int y = static_cast<int>(r % ny);
		r /= ny;
		const int z = u.rz0 + static_cast<int>(r % nz);
		const int o = static_cast<int>(r / nz);
		const int dz = (o & 4) ? -1 : 1;
		const size_t col = (static_cast<size_t>(o & 3) * nzb * ny + y) * nx + x; // a2 at (slice u.bz0, this row and column)
		const size_t pitch = static_cast<size_t>(ny) * nx;                       // a2 slice
		int best = static_cast<int>(ld8(a2, col + static_cast<size_t>(z - u.bz0) * pitch));
		for (int k = 1; k < best; ++k) {
			const int zz = z + k * dz;
			if (zz < 1 || zz > u.cells_height) { best = k; break; }
			best = min(best, max(k, static_cast<int>(ld8(a2, col + static_cast<size_t>(zz - u.bz0) * pitch))));
		}
		st8(field, static_cast<size_t>(o) * u.cf_plane + static_cast<size_t>(z) * u.cf_pxy + (static_cast<size_t>(u.ry0 + y) << u.cf_shift) + (u.rx0 + x), best);
	}
}

inline unsigned grid_for(uint64_t items) {
	const uint64_t blocks = (items + 255) / 256;
	return static_cast<unsigned>(blocks < 16384 ? (blocks ? blocks : 1) : 16384); // the kernels loop over what a grid does not cover
}

} // namespace

size_t field_update_tmp_bytes(const FieldUpdate& u) {
	const size_t nx = u.rx1 - u.rx0, nz = u.bz1 - u.bz0;
	return 2 * nz * static_cast<size_t>(u.ay1 - u.ay0) * nx + 4 * nz * static_cast<size_t>(u.ry1 - u.ry0) * nx;
}

void launch_edit_scatter(const uint32_t* cells, const uint32_t* words, const uint32_t* slots, const uint32_t* bricks, uint32_t count,
						 uint32_t* index_grid, uint32_t* arena, hipStream_t stream) {
	if (count == 0) return;
	const uint32_t per_block = 256 / 16;
	hipLaunchKernelGGL(edit_scatter, dim3((count + per_block - 1) / per_block), dim3(256), 0, stream, cells, words, slots, bricks, count, index_grid, arena);
}

void launch_field_update(const uint32_t* index_grid, uint8_t* field, uint8_t* tmp, const FieldUpdate& u, hipStream_t stream) {
	const size_t nx = u.rx1 - u.rx0, nz = u.bz1 - u.bz0;
	uint8_t* a1 = tmp;
	uint8_t* a2 = tmp + 2 * nz * static_cast<size_t>(u.ay1 - u.ay0) * nx;
	hipLaunchKernelGGL(field_pass_x, dim3(grid_for(2ull * (u.ay1 - u.ay0) * nz)), dim3(256), 0, stream, index_grid, a1, u);
	hipLaunchKernelGGL(field_pass_y, dim3(grid_for(4ull * nx * (u.ry1 - u.ry0) * nz)), dim3(256), 0, stream, a1, a2, u);
	hipLaunchKernelGGL(field_pass_z, dim3(grid_for(8ull * nx * (u.ry1 - u.ry0) * (u.rz1 - u.rz0))), dim3(256), 0, stream, a2, field, u);
}

} // namespace bm
