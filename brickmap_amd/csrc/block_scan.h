// block_scan.h -- the exclusive scan of a 256-thread workgroup over 64-bit values, shared by the kernel files that lay out work on the
// device by scanning counts (voxelize.hip, mesh.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bm {

// exclusive scan of one 64-bit value per thread of a 256-thread workgroup; *total = the sum (as volume.hip's)
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* lds, uint64_t* total) {
	const uint32_t t = threadIdx.x;
	__syncthreads();
	lds[t] = v;
	__syncthreads();
	uint64_t sum = v;
#pragma unroll
	for (uint32_t d = 1; d < 256; d <<= 1) {
		const uint64_t other = t >= d ? lds[t - d] : 0;
		__syncthreads();
		sum += other;
		lds[t] = sum;
		__syncthreads();
	}
	*total = lds[255];
	return sum - v;
}

} // namespace bm
