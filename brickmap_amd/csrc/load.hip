// load.hip -- device half of bm_scene_load_voxels (scene.cpp "dense voxels -> scene"): a dense volume V[z][y][x] of one byte per voxel,
// already in device memory, becomes the canonical build of that content -- the index words, pool bases and bricks World::load_voxels
// (the host route) stores for it.
//
//   classify : one streaming read of the volume; the 2x2x2 LoD mask of every brick cell goes to its index word as lod << 12
//              (0 = empty cell), in place in the index grid -- no side buffer per cell
//   number   : per supercell an exclusive scan of the 4096 occupancy flags in local cell order = the host slots; the words become
//              slot | loaded | lod << 12; the supercell's brick count is kept
//   scan     : exclusive scan of the counts = pool_base (exact-fit pools, as bm_scene_preload_all lays them out) and the total, which
//              the host reads to size the arena
//   pack     : a second read of the volume (brick rows without a brick are skipped); bricks go to arena[pool_base[sc] + slot]
//
// Shape of classify and pack: one workgroup per BRICK ROW -- the 16 brick cells of a supercell that share (by, bz) -- read as 512
// chunks of 16 bytes and assembled in 1 KiB of LDS (brick_rows.h).
// Temporary device memory: 4 bytes per supercell (the counts) and 8 bytes for the total; the cube-field passes that follow
// (edit.hip) take their 6 bytes per brick cell.
#include <hip/hip_runtime.h>

#include "brick_rows.h"
#include "kernels.h"

namespace bm {
namespace {

__device__ __forceinline__ uint32_t ld8x4(const uint8_t* p, size_t byte) { // four bytes of an unaligned volume, as the little-endian word
	const g_u8* q = (const g_u8*)p + byte;
	return q[0] | (static_cast<uint32_t>(q[1]) << 8) | (static_cast<uint32_t>(q[2]) << 16) | (static_cast<uint32_t>(q[3]) << 24);
}

// The workgroup's brick row (blockIdx.x = supercell * 256 + bz * 16 + by) -> rows[256]: word t = word (t & 15) of brick (t >> 4).
// ALIGNED: the volume starts on a 16-byte boundary (every row then does: grid_size is a multiple of 128).
template <bool ALIGNED>
__device__ __forceinline__ void read_brick_row(const uint8_t* __restrict__ vox, const LoadDims& d, uint32_t* rows) {
	const uint32_t sc = blockIdx.x >> 8, bz = (blockIdx.x >> 4) & 15, by = blockIdx.x & 15;
	const uint32_t sx = sc % d.sg_xy, sy = (sc / d.sg_xy) % d.sg_xy, sz = sc / d.sg_xy2;
	const size_t g = d.grid_size;
	uint8_t* bytes = reinterpret_cast<uint8_t*>(rows);
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		const RowChunk c = row_chunk(threadIdx.x + 256 * h);
		const size_t at = (static_cast<size_t>(sz * 128 + bz * 8 + c.z()) * g + (sy * 128 + by * 8 + c.y())) * g + sx * 128 + 16 * c.k;
		u32x4 v;
		if (ALIGNED) v = ld128(vox, at);
		else { v.x = ld8x4(vox, at); v.y = ld8x4(vox, at + 4); v.z = ld8x4(vox, at + 8); v.w = ld8x4(vox, at + 12); }
		// stage_chunk (brick_rows.h), written out: through the call load_pack is compiled with the operands of one OR exchanged
		bytes[(2 * c.k) * 64 + c.r] = static_cast<uint8_t>(brick_row_bits(v.x, v.y));
		bytes[(2 * c.k + 1) * 64 + c.r] = static_cast<uint8_t>(brick_row_bits(v.z, v.w));
	}
	__syncthreads();
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void load_classify(const uint8_t* __restrict__ vox, uint32_t* __restrict__ index_grid, const LoadDims d) {
	__shared__ uint32_t rows[256];
	read_brick_row<ALIGNED>(vox, d, rows);
	// word w of a brick holds bytes 4 w ... 4 w + 3 = rows (y = 4 (w & 1) ..., z = w >> 1): its octants are y >= 4 iff w & 1, z >= 4 iff
	// w >= 8, and x >= 4 is the high nibble of every byte (World::brick_lod, Scene.cpp:95)
	const uint32_t word = rows[threadIdx.x], w = threadIdx.x & 15;
	const uint32_t oct = (w & 1) * 2 + (w >> 3) * 4;
	uint32_t lod = ((word & 0x0F0F0F0Fu) ? 1u << oct : 0u) | ((word & 0xF0F0F0F0u) ? 2u << oct : 0u);
	lod |= __shfl_xor(lod, 1);
	lod |= __shfl_xor(lod, 2);
	lod |= __shfl_xor(lod, 4);
	lod |= __shfl_xor(lod, 8);
	if (w == 0) st32(index_grid, static_cast<size_t>(blockIdx.x) * 16 + (threadIdx.x >> 4), lod << 12); // cell = sc * 4096 + bz * 256 + by * 16 + bx
}

// one workgroup per supercell, one lane per brick row: 16 words in, 16 words out
__global__ __launch_bounds__(256) void load_number(uint32_t* __restrict__ index_grid, uint32_t* __restrict__ counts) {
	__shared__ uint32_t wave_total[4];
	const size_t at = (static_cast<size_t>(blockIdx.x) * 4096 + threadIdx.x * 16) * sizeof(uint32_t);
	u32x4 a = ld128(index_grid, at), b = ld128(index_grid, at + 16), c = ld128(index_grid, at + 32), e = ld128(index_grid, at + 48);
#define BM_EACH_WORD(F) F(a.x) F(a.y) F(a.z) F(a.w) F(b.x) F(b.y) F(b.z) F(b.w) F(c.x) F(c.y) F(c.z) F(c.w) F(e.x) F(e.y) F(e.z) F(e.w)
	uint32_t mine = 0;
#define BM_COUNT(v) mine += (v) != 0;
	BM_EACH_WORD(BM_COUNT)
#undef BM_COUNT
	// inclusive scan inside the wave, then the four wave totals
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t inc = mine;
#pragma unroll
	for (int s = 1; s < 64; s *= 2) {
		const uint32_t up = __shfl_up(inc, s);
		if (lane >= static_cast<uint32_t>(s)) inc += up;
	}
	if (lane == 63) wave_total[wave] = inc;
	__syncthreads();
	uint32_t slot = inc - mine;
	for (uint32_t v = 0; v < wave; ++v) slot += wave_total[v];
	if (threadIdx.x == 255) st32(counts, blockIdx.x, slot + mine);
#define BM_NUMBER(v) if (v) { (v) |= slot | kLoadedBit; ++slot; }
	BM_EACH_WORD(BM_NUMBER)
#undef BM_NUMBER
#undef BM_EACH_WORD
	st128(index_grid, at, a); st128(index_grid, at + 16, b); st128(index_grid, at + 32, c); st128(index_grid, at + 48, e);
}

// one workgroup: lane t owns the supercells [t * per, (t + 1) * per); total[0], total[1] = the 64-bit sum (it decides whether the
// 32-bit pool bases are valid: the host refuses a world of 2^32 bricks or more)
__global__ __launch_bounds__(256) void load_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ pool_base, uint32_t* __restrict__ total, uint32_t n) {
	__shared__ unsigned long long part[256];
	const uint32_t per = (n + 255) / 256;
	const uint32_t begin = min(n, threadIdx.x * per), end = min(n, begin + per);
	unsigned long long sum = 0;
	for (uint32_t i = begin; i < end; ++i) sum += ld32(counts, i);
	part[threadIdx.x] = sum;
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long run = 0;
		for (int i = 0; i < 256; ++i) { const unsigned long long p = part[i]; part[i] = run; run += p; }
		st32(total, 0, static_cast<uint32_t>(run));
		st32(total, 1, static_cast<uint32_t>(run >> 32));
	}
	__syncthreads();
	unsigned long long run = part[threadIdx.x];
	for (uint32_t i = begin; i < end; ++i) { st32(pool_base, i, static_cast<uint32_t>(run)); run += ld32(counts, i); }
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void load_pack(const uint8_t* __restrict__ vox, const uint32_t* __restrict__ index_grid, const uint32_t* __restrict__ pool_base,
												 uint32_t* __restrict__ arena, const LoadDims d) {
	__shared__ uint32_t rows[256];
	const uint32_t iw = ld32(index_grid, static_cast<size_t>(blockIdx.x) * 16 + (threadIdx.x >> 4));
	if (!__syncthreads_or(iw != 0)) return; // no brick in this row: nothing to read
	read_brick_row<ALIGNED>(vox, d, rows);
	// brick_first_word (device_types.h), written out: base and slot are added in 32 bits here, as in the walk (traverse.h)
	if (iw) st32(arena, (static_cast<size_t>(ld32(pool_base, blockIdx.x >> 8) + (iw & kIndexBits)) << 4) + (threadIdx.x & 15), rows[threadIdx.x]);
}

} // namespace

void launch_load_classify(const uint8_t* voxels, uint32_t* index_grid, const LoadDims& d, hipStream_t stream) {
	const dim3 grid(static_cast<unsigned>(d.supercells) * 256u);
	if (reinterpret_cast<uintptr_t>(voxels) % 16 == 0) hipLaunchKernelGGL(load_classify<true>, grid, dim3(256), 0, stream, voxels, index_grid, d);
	else hipLaunchKernelGGL(load_classify<false>, grid, dim3(256), 0, stream, voxels, index_grid, d);
}

void launch_load_number(uint32_t* index_grid, uint32_t* counts, uint32_t* pool_base, uint32_t* total, const LoadDims& d, hipStream_t stream) {
	hipLaunchKernelGGL(load_number, dim3(static_cast<unsigned>(d.supercells)), dim3(256), 0, stream, index_grid, counts);
	hipLaunchKernelGGL(load_scan, dim3(1), dim3(256), 0, stream, counts, pool_base, total, static_cast<uint32_t>(d.supercells));
}

void launch_load_pack(const uint8_t* voxels, const uint32_t* index_grid, const uint32_t* pool_base, uint32_t* arena, const LoadDims& d, hipStream_t stream) {
	const dim3 grid(static_cast<unsigned>(d.supercells) * 256u);
	if (reinterpret_cast<uintptr_t>(voxels) % 16 == 0) hipLaunchKernelGGL(load_pack<true>, grid, dim3(256), 0, stream, voxels, index_grid, pool_base, arena, d);
	else hipLaunchKernelGGL(load_pack<false>, grid, dim3(256), 0, stream, voxels, index_grid, pool_base, arena, d);
}

} // namespace bm
