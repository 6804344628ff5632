// brick_rows.h -- how a 256-thread workgroup moves a RUN of 16 brick cells along x between a dense volume of one byte per voxel and
// brick bits (load.hip: a brick row of a supercell; region.hip: a run of a box that starts at a multiple of 128 voxels).
//
// The run's voxels are 64 x-rows (y, z = 0 ... 7) of 128 contiguous bytes each.  They are handled as 512 CHUNKS of 16 bytes, two per
// lane (i = threadIdx.x and threadIdx.x + 256): chunk i is bytes 16 k ... 16 k + 15 (k = i & 7) of x-row r = i >> 3 (y = r & 7,
// z = r >> 3).  So a lane's 16-byte access covers the rows of two bricks, eight neighbouring lanes cover one whole 128-byte line and a
// wave instruction requests eight full lines.  A row's 8 + 8 voxels are byte r = y + 8 z of bricks 2 k and 2 k + 1 (voxel_bits.h).
// The 16 bricks of the run are staged in 1 KiB of LDS, rows[256]: word t = word (t & 15) of brick (t >> 4), so that they enter or
// leave it as 16 lanes x 4 bytes per brick.
#pragma once
#include "global_mem.h"
#include "voxel_bits.h"

namespace bm {

struct RowChunk {
	uint32_t r, k; // x-row of the run, 16-byte piece of its 128 bytes
	__device__ __forceinline__ uint32_t y() const { return r & 7; }
	__device__ __forceinline__ uint32_t z() const { return r >> 3; }
};
__device__ __forceinline__ RowChunk row_chunk(uint32_t i) { return RowChunk{i >> 3, i & 7}; }

// the chunk's 16 voxel bytes -> its row byte in each of its two bricks
__device__ __forceinline__ void stage_chunk(uint32_t* rows, RowChunk c, u32x4 v) {
	uint8_t* bytes = reinterpret_cast<uint8_t*>(rows);
	bytes[(2 * c.k) * 64 + c.r] = static_cast<uint8_t>(brick_row_bits(v.x, v.y));
	bytes[(2 * c.k + 1) * 64 + c.r] = static_cast<uint8_t>(brick_row_bits(v.z, v.w));
}
// the inverse: the chunk's 16 voxel bytes (0 / 1) from the two staged row bytes
__device__ __forceinline__ u32x4 staged_chunk(const uint32_t* rows, RowChunk c) {
	const uint8_t* bytes = reinterpret_cast<const uint8_t*>(rows);
	uint32_t a, b, e, f;
	brick_row_bytes(bytes[(2 * c.k) * 64 + c.r], &a, &b);
	brick_row_bytes(bytes[(2 * c.k + 1) * 64 + c.r], &e, &f);
	return u32x4{a, b, e, f};
}

} // namespace bm
