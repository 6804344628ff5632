// region.hip -- device halves of bm_scene_write_region and bm_scene_read_region (scene.cpp "dense regions"): a box of voxels as a dense
// volume V[z][y][x] of one byte per voxel in device memory, x contiguous, rows and slices at the caller's pitches.
//
//   pack   : the clipped box -> one 64-byte brick per brick cell it overlaps (bits outside the box are 0), in the cell order of the
//            box's cells, x fastest.  The host merges those into its world (World::write_region_supercell).
//   unpack : for every brick cell the clipped box overlaps, the device index word and -- when it is loaded -- the brick at
//            arena[pool_base + slot] -> the box's part of the cell as bytes 0 / 1; cells that are empty or not resident give 0
//   patch  : a list of (cell, brick) pairs -> the box's part of those cells (the bricks a streaming scene does not hold on the device)
//   zero   : a sub-box of the volume set to 0 (the parts of a read that lie outside the world)
//
// Shape of pack and unpack: one workgroup per run of 16 brick cells along x that starts at a multiple of 128 voxels, moved as 512
// chunks of 16 bytes through 1 KiB of LDS (brick_rows.h).  ALIGNED: V[0][0][0] lies at a world x that is a multiple of 16 and the base
// and both pitches are multiples of 16 bytes, so every chunk is a 16-byte aligned address: chunks wholly inside the box move as one
// 16-byte access, the (at most two per row) partial ones byte by byte.  The general instantiation moves every chunk byte by byte.
// Nothing outside the box is read or written.
#include <hip/hip_runtime.h>

#include "brick_rows.h"
#include "kernels.h"

namespace bm {
namespace {

// four voxel bytes at world x ... x + 3 of a row (at = the volume offset of world x), those outside [x0, x1) read as 0 and are not touched
__device__ __forceinline__ uint32_t ld_bytes(const uint8_t* p, int64_t at, int x, int x0, int x1) {
	const g_u8* q = (const g_u8*)p + at;
	uint32_t v = 0;
#pragma unroll
	for (int j = 0; j < 4; ++j)
		if (x + j >= x0 && x + j < x1) v |= static_cast<uint32_t>(q[j]) << (8 * j);
	return v;
}
__device__ __forceinline__ void st_bytes(uint8_t* p, int64_t at, int x, int x0, int x1, uint32_t v) {
	g_u8* q = (g_u8*)p + at;
#pragma unroll
	for (int j = 0; j < 4; ++j)
		if (x + j >= x0 && x + j < x1) q[j] = static_cast<uint8_t>(v >> (8 * j));
}

// a chunk of the workgroup's run (brick_rows.h) in the world and in the volume
struct Chunk {
	RowChunk rc;
	int x;         // world x of its first voxel
	bool row;      // the row lies in the box
	int64_t at;    // volume offset of world voxel (x, y, z)
};
__device__ __forceinline__ Chunk chunk_of(const RegionDims& d, uint32_t i) {
	Chunk c;
	c.rc = row_chunk(i);
	const int y = (d.c0[1] + static_cast<int>(blockIdx.y)) * 8 + static_cast<int>(c.rc.y()), z = (d.c0[2] + static_cast<int>(blockIdx.z)) * 8 + static_cast<int>(c.rc.z());
	c.x = (d.g0 + static_cast<int>(blockIdx.x)) * 128 + 16 * static_cast<int>(c.rc.k);
	c.row = y >= d.lo[1] && y < d.hi[1] && z >= d.lo[2] && z < d.hi[2];
	c.at = (static_cast<int64_t>(z) - d.org[2]) * d.slice_pitch + (static_cast<int64_t>(y) - d.org[1]) * d.row_pitch + (static_cast<int64_t>(c.x) - d.org[0]);
	return c;
}

// word t & 15 of the brick of cell (g * 16 + (t >> 4), cy, cz): its place among the box's cells, or -1 when the cell is not one of them
__device__ __forceinline__ int64_t box_cell(const RegionDims& d, uint32_t t) {
	const int cx = (d.g0 + static_cast<int>(blockIdx.x)) * 16 + static_cast<int>(t >> 4) - d.c0[0];
	if (cx < 0 || cx >= d.nc[0]) return -1;
	return (static_cast<int64_t>(blockIdx.z) * d.nc[1] + blockIdx.y) * d.nc[0] + cx;
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void region_pack(const uint8_t* __restrict__ vox, uint32_t* __restrict__ bricks, const RegionDims d) {
	__shared__ uint32_t rows[256];
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		const Chunk c = chunk_of(d, threadIdx.x + 256 * h);
		u32x4 v = {0u, 0u, 0u, 0u};
		if (c.row && c.x < d.hi[0] && c.x + 16 > d.lo[0]) {
			if (ALIGNED && c.x >= d.lo[0] && c.x + 16 <= d.hi[0]) v = ld128(vox, c.at);
			else {
				v.x = ld_bytes(vox, c.at, c.x, d.lo[0], d.hi[0]);
				v.y = ld_bytes(vox, c.at + 4, c.x + 4, d.lo[0], d.hi[0]);
				v.z = ld_bytes(vox, c.at + 8, c.x + 8, d.lo[0], d.hi[0]);
				v.w = ld_bytes(vox, c.at + 12, c.x + 12, d.lo[0], d.hi[0]);
			}
		}
		stage_chunk(rows, c.rc, v);
	}
	__syncthreads();
	const int64_t cell = box_cell(d, threadIdx.x);
	if (cell >= 0) st32(bricks, static_cast<size_t>(cell) * 16 + (threadIdx.x & 15), rows[threadIdx.x]);
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void region_unpack(uint8_t* __restrict__ vox, const uint32_t* __restrict__ index_grid, const uint32_t* __restrict__ pool_base,
													 const uint32_t* __restrict__ arena, const RegionDims d) {
	__shared__ uint32_t rows[256];
	{
		uint32_t word = 0;
		if (box_cell(d, threadIdx.x) >= 0) { // a cell of the clipped box: inside the world
			const uint32_t cx = static_cast<uint32_t>(d.g0 + static_cast<int>(blockIdx.x)) * 16 + (threadIdx.x >> 4), cy = static_cast<uint32_t>(d.c0[1]) + blockIdx.y,
						   cz = static_cast<uint32_t>(d.c0[2]) + blockIdx.z;
			// supercell_of and index_word_at (device_types.h), written out: through them the run's supercell is no longer found to be the
			// same for the whole workgroup, and the kernel computes it per lane
			const uint32_t sc = (cx >> 4) + (cy >> 4) * d.sg_xy + (cz >> 4) * d.sg_xy2;
			const uint32_t iw = ld32(index_grid, static_cast<size_t>(sc) * 4096 + (cx & 15) + (cy & 15) * 16 + (cz & 15) * 256);
			if (iw & kLoadedBit) word = ld32(arena, brick_first_word(ld32(pool_base, sc), iw) + (threadIdx.x & 15));
		}
		rows[threadIdx.x] = word;
	}
	__syncthreads();
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		const Chunk c = chunk_of(d, threadIdx.x + 256 * h);
		if (!(c.row && c.x < d.hi[0] && c.x + 16 > d.lo[0])) continue;
		const u32x4 v = staged_chunk(rows, c.rc);
		if (ALIGNED && c.x >= d.lo[0] && c.x + 16 <= d.hi[0]) st128(vox, c.at, v);
		else {
			st_bytes(vox, c.at, c.x, d.lo[0], d.hi[0], v.x);
			st_bytes(vox, c.at + 4, c.x + 4, d.lo[0], d.hi[0], v.y);
			st_bytes(vox, c.at + 8, c.x + 8, d.lo[0], d.hi[0], v.z);
			st_bytes(vox, c.at + 12, c.x + 12, d.lo[0], d.hi[0], v.w);
		}
	}
}

// four listed cells per workgroup, one lane per x-row: cells[3 i ...] = the brick cell's world coordinates, bricks[16 i ...] its bits
__global__ __launch_bounds__(256) void region_patch(uint8_t* __restrict__ vox, const int* __restrict__ cells, const uint32_t* __restrict__ bricks, uint32_t count,
													const RegionDims d) {
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), r = threadIdx.x & 63;
	if (i >= count) return;
	const int x = ldi32(cells, 3 * i) * 8, y = ldi32(cells, 3 * i + 1) * 8 + static_cast<int>(r & 7), z = ldi32(cells, 3 * i + 2) * 8 + static_cast<int>(r >> 3);
	if (!(y >= d.lo[1] && y < d.hi[1] && z >= d.lo[2] && z < d.hi[2])) return;
	const uint32_t word = ld32(bricks, static_cast<size_t>(i) * 16 + (r >> 2));
	uint32_t a, b;
	brick_row_bytes((word >> (8 * (r & 3))) & 0xFFu, &a, &b);
	const int64_t at = (static_cast<int64_t>(z) - d.org[2]) * d.slice_pitch + (static_cast<int64_t>(y) - d.org[1]) * d.row_pitch + (static_cast<int64_t>(x) - d.org[0]);
	st_bytes(vox, at, x, d.lo[0], d.hi[0], a);
	st_bytes(vox, at + 4, x + 4, d.lo[0], d.hi[0], b);
}

// rows [0, ny * nz) of nx bytes at vox + z * slice_pitch + y * row_pitch: workgroups stride over the rows, lanes over a row's bytes
__global__ __launch_bounds__(256) void region_zero(uint8_t* __restrict__ vox, int64_t row_pitch, int64_t slice_pitch, int64_t nx, int64_t ny, int64_t nz) {
	for (int64_t row = blockIdx.x; row < ny * nz; row += gridDim.x) {
		g_u8* q = (g_u8*)vox + (row / ny) * slice_pitch + (row % ny) * row_pitch;
		for (int64_t x = threadIdx.x; x < nx; x += 256) q[x] = 0;
	}
}

bool aligned16(const void* p, const RegionDims& d) {
	return reinterpret_cast<uintptr_t>(p) % 16 == 0 && d.row_pitch % 16 == 0 && d.slice_pitch % 16 == 0 && (d.org[0] & 15) == 0;
}
dim3 run_grid(const RegionDims& d) {
	return dim3(static_cast<unsigned>(((d.c0[0] + d.nc[0] - 1) >> 4) - d.g0 + 1), static_cast<unsigned>(d.nc[1]), static_cast<unsigned>(d.nc[2]));
}

} // namespace

void launch_region_pack(const uint8_t* voxels, uint32_t* bricks, const RegionDims& d, hipStream_t stream) {
	if (aligned16(voxels, d)) hipLaunchKernelGGL(region_pack<true>, run_grid(d), dim3(256), 0, stream, voxels, bricks, d);
	else hipLaunchKernelGGL(region_pack<false>, run_grid(d), dim3(256), 0, stream, voxels, bricks, d);
}

void launch_region_unpack(uint8_t* voxels, const uint32_t* index_grid, const uint32_t* pool_base, const uint32_t* arena, const RegionDims& d, hipStream_t stream) {
	if (aligned16(voxels, d)) hipLaunchKernelGGL(region_unpack<true>, run_grid(d), dim3(256), 0, stream, voxels, index_grid, pool_base, arena, d);
	else hipLaunchKernelGGL(region_unpack<false>, run_grid(d), dim3(256), 0, stream, voxels, index_grid, pool_base, arena, d);
}

void launch_region_patch(uint8_t* voxels, const int* cells, const uint32_t* bricks, uint32_t count, const RegionDims& d, hipStream_t stream) {
	hipLaunchKernelGGL(region_patch, dim3((count + 3) / 4), dim3(256), 0, stream, voxels, cells, bricks, count, d);
}

void launch_region_zero(uint8_t* voxels, int64_t row_pitch, int64_t slice_pitch, int64_t nx, int64_t ny, int64_t nz, hipStream_t stream) {
	const int64_t rows = ny * nz;
	hipLaunchKernelGGL(region_zero, dim3(static_cast<unsigned>(rows < 65536 ? rows : 65536)), dim3(256), 0, stream, voxels, row_pitch, slice_pitch, nx, ny, nz);
}

} // namespace bm
