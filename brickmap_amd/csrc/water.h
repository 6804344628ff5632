// water.h -- the rules of the spill-level field (bm_water_field, bm_water_mask, include/brickmap.h), written once for the kernels of
// water.hip and the plain loops of water_host.cpp.  Needs no HIP header: tests/water_check.cpp builds it with a host compiler.
//
// All integers.  L(p) = max(sea_level, the least over all paths of free voxels from p to an outlet of the largest z on the path) is a
// minimum over finitely many integers and therefore unique.  The device reaches it by the relaxation of travel.h with another step: the
// volume is cut into the same 8^3 tiles with the same workspace (TravelDims, the bricks, two lists, stamps, TravelTail), a wave settles
// one tile in registers -- one x-row per lane -- and rounds of such waves run until no tile is listed any more.  What a lane does in one
// sweep is water_row_sweep below, so that the check program can run a tile lane by lane without a device.
//
// Why late values do no harm.  A value only ever falls, within the finite set {0 ... nz, none}, and every value ever stored is the
// bottleneck of a real path from an outlet (raised to the sea): a value read late is merely larger than it will become, never wrong.  A
// tile whose neighbour's face value fell in round k is listed for round k + 1, a later kernel, so it sees that value then.  After round
// k every voxel whose best path crosses at most k - 1 tile faces is final; a best path can be taken without a repeated voxel, so it
// crosses fewer faces than the volume has voxels.
#pragma once
#include <cstddef>
#include <cstdint>

#include "travel.h"

namespace bm {

constexpr uint32_t kWaterNone = kTravelNone; // BM_WATER_NONE
constexpr uint32_t kWaterFaces = 0x3Fu;      // the flags: bit 0 ... 5 = the -x, +x, -y, +y, -z, +z face of the box is open (bm_component.faces)
// the tail is a TravelTail; beside the words travel.h names, the finish's closed count lies in its padding (the tail as 64-bit words:
// key, wet, rejected | pad0, ..., closed) and so does the number of tile visits, the sum of the lists' lengths (as 32-bit words)
constexpr uint32_t kWaterTailClosedWord64 = 5, kWaterTailVisitsWord = 12;

// a bm_water_params is a bm_travel_params with sea_level where max_steps is
template <class P>
inline TravelParamsView water_params_view(const P& p) {
	return {{p.extent[0], p.extent[1], p.extent[2]}, p.sea_level, p.row_pitch, p.slice_pitch, p.flags, p.reserved};
}

// null, or why bm_water_field and bm_host_water_field refuse these parameters: what travel_params_problem says, in its order, with the
// six face bits known, and a sea above the box
inline const char* water_params_problem(const TravelParamsView& p) {
	TravelParamsView q = p;
	q.flags = p.flags & ~kWaterFaces;
	if (const char* why = travel_params_problem(q)) return why;
	if (p.max_steps > static_cast<uint32_t>(p.extent[2])) return "sea_level above the extent along z";
	return nullptr;
}

// the dims (tiles, pitches, voxels) of a water call; `limit` means nothing here
inline TravelDims water_dims(const TravelParamsView& p) {
	TravelParamsView q = p;
	q.max_steps = 0;
	return travel_dims(q);
}

// ---- outlets
// the face bits of the box that voxel (x, y, z) lies on
BM_VHD uint32_t water_faces_of(const int32_t extent[3], int32_t x, int32_t y, int32_t z) {
	return (x == 0 ? 1u : 0u) | (x == extent[0] - 1 ? 2u : 0u) | (y == 0 ? 4u : 0u) | (y == extent[1] - 1 ? 8u : 0u) | (z == 0 ? 16u : 0u) | (z == extent[2] - 1 ? 32u : 0u);
}
// what an outlet at height z starts with
BM_VHD uint32_t water_start(uint32_t z, uint32_t sea) { return z > sea ? z : sea; }

// ---- a tile
// what a voxel at height z that holds t takes from a neighbour that holds `from`: the path through the neighbour, raised to z.  Branch-free;
// max(kWaterNone, z) == kWaterNone because z < 16384.
BM_VHD uint32_t water_step(uint32_t t, uint32_t from, uint32_t z, bool open) {
	const uint32_t c = from > z ? from : z, m = c < t ? c : t;
	return open ? m : t;
}

// One sweep of the lane that holds the x-row t[0 ... 7] of a tile at height z.  open: bit i = voxel i is free.  near[i]: the least value
// of voxel i of the four neighbouring rows (y - 1, y + 1, z - 1, z + 1) inside the tile as they stood before this sweep, kWaterNone where
// there is none -- one minimum serves all four, since max(min(a, b), z) == min(max(a, z), max(b, z)).  First every free voxel takes from
// near, then the row is walked up and down, which settles it in itself.  True when a value fell.
// Bound: the argument of travel_row_sweep.  After s sweeps every voxel is final whose best derivation inside the tile changes rows at
// most s times; a best derivation visits no voxel twice (cutting a loop out of a path cannot raise its largest z), so it changes rows
// fewer than 512 times, and sweep kTravelTileSweeps at the latest changes nothing.
BM_VHD bool water_row_sweep(uint32_t t[8], uint32_t open, const uint32_t near[8], uint32_t z) {
	uint32_t diff = 0;
BM_TRAVEL_UNROLL
	for (int i = 0; i < 8; ++i) {
		const uint32_t v = water_step(t[i], near[i], z, (open >> i) & 1u);
		diff |= v ^ t[i];
		t[i] = v;
	}
BM_TRAVEL_UNROLL
	for (int i = 1; i < 8; ++i) {
		const uint32_t v = water_step(t[i], t[i - 1], z, (open >> i) & 1u);
		diff |= v ^ t[i];
		t[i] = v;
	}
BM_TRAVEL_UNROLL
	for (int i = 6; i >= 0; --i) {
		const uint32_t v = water_step(t[i], t[i + 1], z, (open >> i) & 1u);
		diff |= v ^ t[i];
		t[i] = v;
	}
	return diff != 0;
}

// ---- the record and the mask
// wet: water stands in the voxel; its depth is L - z
BM_VHD bool water_wet(uint32_t level, uint32_t z) { return level != kWaterNone && level > z; }
// the key of travel_max_key taken over depths: its maximum names the largest depth and, among its voxels, the lowest index; 0 for a voxel
// that is not wet
BM_VHD uint64_t water_depth_key(uint32_t level, uint32_t z, uint32_t index) { return water_wet(level, z) ? travel_max_key(level - z, index) : 0u; }
// the mask's byte
BM_VHD uint32_t water_mask_byte(uint32_t level, uint32_t z, uint32_t min_depth) { return water_wet(level, z) && level - z >= min_depth ? 1u : 0u; }

// the 32 bytes of a bm_water_result
struct WaterRecord {
	uint64_t wet;
	uint32_t deepest, drains_rejected;
	uint64_t deepest_at, closed;
};
BM_VHD WaterRecord water_record(uint64_t key, uint64_t wet, uint32_t rejected, uint64_t closed) {
	if (key == 0) return {wet, 0u, rejected, 0u, closed};
	return {wet, static_cast<uint32_t>(key >> 32), rejected, static_cast<uint64_t>(0xFFFFFFFFu - static_cast<uint32_t>(key)), closed};
}

} // namespace bm
