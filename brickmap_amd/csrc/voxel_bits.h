// voxel_bits.h -- dense voxels (one byte each, non-zero = solid) -> brick bits; shared by the host route (world.cpp load_voxels)
// and the device route (load.hip) of bm_scene_load_voxels, so that both pack a row of voxels with the same arithmetic.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BM_VHD __host__ __device__ inline
#else
#define BM_VHD inline // world.cpp also builds with a plain host compiler (tools/sim)
#endif

namespace bm {

// four voxel bytes (x ascending = byte 0 first) -> four bits, bit i set iff byte i is non-zero.
// m: bit 7 of every non-zero byte (the add carries into bit 7 when any of the low seven bits is set; | v covers bit 7 itself).
// The multiply moves the bit of byte i from position 8 i to position 28 + i: the shifts 28 - 7 i of its four terms place no two
// products on the same bit (8 i - 7 j is distinct for every pair), so nothing carries.
BM_VHD uint32_t nonzero_bytes4(uint32_t v) {
	const uint32_t m = (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;
	return ((m >> 7) * 0x10204080u) >> 28;
}

// eight voxel bytes of one x-row of a brick (lo = x 0..3, hi = x 4..7) -> byte (y + 8 z) of the brick (bit = x + 8 y + 64 z, Scene.cpp:91-93)
BM_VHD uint32_t brick_row_bits(uint32_t lo, uint32_t hi) { return nonzero_bytes4(lo) | (nonzero_bytes4(hi) << 4); }

} // namespace bm
