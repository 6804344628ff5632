// voxel_bits.h -- dense voxels (one byte each, non-zero = solid) <-> brick bits; shared by the host routes (world.cpp) and the device
// routes (load.hip and region.hip through brick_rows.h, volume.hip) of bm_scene_load_voxels, bm_scene_write_region and bm_scene_read_region, so that all of them pack and
// unpack a row of voxels with the same arithmetic.
#pragma once
#include <cstdint>

#include "device_types.h" // BM_VHD

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

// the inverse: four bits (bit i = voxel i) -> four voxel bytes of 0 / 1, byte 0 = bit 0.  The multiply copies the nibble to bit
// positions 0, 7, 14 and 21, so that bit i lands on bit 8 i (and other bits elsewhere: 7 j + i = 8 i only for j = i); nothing carries.
BM_VHD uint32_t bits4_to_bytes(uint32_t nibble) { return ((nibble & 0xFu) * 0x00204081u) & 0x01010101u; }

// byte (y + 8 z) of a brick -> the eight voxel bytes of that x-row: *lo = x 0..3, *hi = x 4..7 (the inverse of brick_row_bits)
BM_VHD void brick_row_bytes(uint32_t bits, uint32_t* lo, uint32_t* hi) {
	*lo = bits4_to_bytes(bits);
	*hi = bits4_to_bytes(bits >> 4);
}

} // namespace bm
