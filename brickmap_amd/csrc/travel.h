// travel.h -- the rules of the travel field (bm_travel_field, bm_travel_paths, include/brickmap.h), written once for the kernels of
// travel.hip and the plain loops of travel_host.cpp.  Needs no HIP header: tests/travel_check.cpp builds it with a host compiler.
//
// All integers.  T(p) = the least number of face steps from an accepted seed to p through open voxels is a breadth-first distance and
// therefore unique.  The device reaches it by relaxation: the volume is cut into 8^3 tiles, a wave settles one tile in registers -- one
// x-row of eight voxels per lane, the layout of label_local -- and rounds of such waves run until no tile is listed any more.  What a
// lane does in one sweep is travel_row_sweep below, so that the check program can run a tile lane by lane without a device.
//
// Why late values do no harm.  A value only ever falls, and every value ever stored is the length of a real path from a seed: a value
// read late is merely larger than it will become, never wrong.  A tile whose neighbour's face value fell in round k is listed for round
// k + 1, a later kernel, so it sees that value then.  After round k every voxel whose shortest path crosses at most k - 1 tile faces is
// final, and a path of d steps crosses at most d faces.
#pragma once
#include <cstddef>
#include <cstdint>

#include "device_types.h"

// full unrolling keeps the rows in registers on the device; a plain host compiler does not know the pragma
#if defined(__clang__)
#define BM_TRAVEL_UNROLL _Pragma("unroll")
#else
#define BM_TRAVEL_UNROLL
#endif

namespace bm {

constexpr uint32_t kTravelNone = 0x7FFFFFFFu;                // BM_TRAVEL_NONE
constexpr uint32_t kTravelMaxSteps = 0x7FFFFFFEu - 1u;       // every finite value is below 2^31 - 2
constexpr int kTravelMaxExtent = 16384;                      // the limits of bm_distance_params
constexpr int64_t kTravelMaxVoxels = (int64_t{1} << 31) - 2;
constexpr int kTravelTileSweeps = 512;                       // a tile settles in fewer sweeps than it has voxels (travel_row_sweep)
constexpr uint32_t kTravelMaxWaves = 8192;                   // the grid of a round at most; its waves stride over the list
constexpr uint32_t kTravelBatch = 64;                        // rounds enqueued between two looks of the host at the next list's count (measured: DESIGN.md 4.18)
constexpr size_t kTravelTailBytes = 64;                      // the workspace's last bytes, see TravelTail

struct TravelParamsView {
	int32_t extent[3];
	uint32_t max_steps;
	int64_t row_pitch, slice_pitch;
	uint32_t flags, reserved;
};

// the view of a bm_travel_params (a template, so that this header needs no other)
template <class P>
inline TravelParamsView travel_params_view(const P& p) {
	return {{p.extent[0], p.extent[1], p.extent[2]}, p.max_steps, p.row_pitch, p.slice_pitch, p.flags, p.reserved};
}

// null, or why these extents are refused
inline const char* travel_extent_problem(const int32_t extent[3]) {
	for (int k = 0; k < 3; ++k)
		if (extent[k] < 1 || extent[k] > kTravelMaxExtent) return "an extent below 1 or above 16384";
	if (static_cast<int64_t>(extent[0]) * extent[1] > kTravelMaxVoxels / extent[2]) return "more than 2^31 - 2 voxels";
	return nullptr;
}

// null, or why bm_travel_field and bm_host_travel_field refuse these parameters (pitches as given: 0 = tight)
inline const char* travel_params_problem(const TravelParamsView& p) {
	if (p.flags != 0) return "unknown flag";
	if (p.reserved != 0) return "reserved is not 0";
	if (const char* why = travel_extent_problem(p.extent)) return why;
	if (p.row_pitch < 0 || p.slice_pitch < 0) return "negative pitch";
	if (p.row_pitch > (int64_t{1} << 40)) return "row_pitch above 2^40";
	const int64_t row = p.row_pitch ? p.row_pitch : p.extent[0];
	if (row < p.extent[0]) return "row_pitch below the extent along x";
	if (p.slice_pitch && p.slice_pitch / p.extent[1] < row) return "slice_pitch below row_pitch * the extent along y";
	if ((p.slice_pitch ? p.slice_pitch : row * p.extent[1]) > (int64_t{1} << 46) / p.extent[2]) return "a volume spanning more than 2^46 bytes";
	return nullptr;
}

// what the kernels and the loops need of the parameters
struct TravelDims {
	int32_t extent[3];
	uint32_t limit;                 // the largest value that is taken: max_steps, or kTravelMaxSteps without a limit
	uint32_t voxels;                // below 2^31 - 1
	uint32_t tiles[3], tile_count;  // 8^3 tiles per axis (the last one of an axis may be ragged) and in all
	int64_t row_pitch, slice_pitch; // resolved: never 0
};

inline TravelDims travel_dims(const TravelParamsView& p) {
	TravelDims d;
	for (int k = 0; k < 3; ++k) {
		d.extent[k] = p.extent[k];
		d.tiles[k] = static_cast<uint32_t>(p.extent[k] + 7) >> 3;
	}
	d.limit = p.max_steps != 0 && p.max_steps < kTravelMaxSteps ? p.max_steps : kTravelMaxSteps;
	d.voxels = static_cast<uint32_t>(static_cast<int64_t>(p.extent[0]) * p.extent[1] * p.extent[2]);
	d.tile_count = d.tiles[0] * d.tiles[1] * d.tiles[2];
	d.row_pitch = p.row_pitch ? p.row_pitch : p.extent[0];
	d.slice_pitch = p.slice_pitch ? p.slice_pitch : d.row_pitch * p.extent[1];
	return d;
}

// the dims of a field alone (bm_travel_paths): extents, no volume
inline TravelDims travel_field_dims(const int32_t extent[3]) { return travel_dims({{extent[0], extent[1], extent[2]}, 0u, 0, 0, 0u, 0u}); }

// bytes from the volume's first byte to one past its last
inline uint64_t travel_span(const TravelDims& d) {
	return static_cast<uint64_t>(d.extent[2] - 1) * static_cast<uint64_t>(d.slice_pitch) + static_cast<uint64_t>(d.extent[1] - 1) * static_cast<uint64_t>(d.row_pitch) +
		   static_cast<uint64_t>(d.extent[0]);
}

// The workspace: one 64-byte bit brick of blocked voxels per tile (byte y + 8 z of a brick = the x-row's bits, voxel_bits.h; voxels
// outside the volume count as blocked); two work lists of tile_count entries each (a tile is listed at most once per round); a round
// stamp per tile; the tail.  Every part is a multiple of 16 bytes; the stamps and the tail lie together and are zeroed by every call.
inline size_t travel_bricks_bytes(const TravelDims& d) { return static_cast<size_t>(d.tile_count) * 64; }
inline size_t travel_words_bytes(const TravelDims& d) { return (static_cast<size_t>(d.tile_count) * 4 + 15) & ~static_cast<size_t>(15); }
inline size_t travel_list_offset(const TravelDims& d, uint32_t which) { return travel_bricks_bytes(d) + which * travel_words_bytes(d); }
inline size_t travel_stamps_offset(const TravelDims& d) { return travel_bricks_bytes(d) + 2 * travel_words_bytes(d); }
inline size_t travel_tail_offset(const TravelDims& d) { return travel_bricks_bytes(d) + 3 * travel_words_bytes(d); }
inline size_t travel_workspace_bytes(const TravelDims& d) { return travel_tail_offset(d) + kTravelTailBytes; }

// the tail, zeroed by every call: the finish's key and count, the seeds' reject count, and the three list counts -- round k reads
// count[k % 3], appends under count[(k + 1) % 3] and zeroes count[(k + 2) % 3], which round k - 1 read and round k + 1 appends under
struct TravelTail {
	uint64_t key, reached;
	uint32_t rejected, pad0;
	uint32_t count[3], pad1;
	uint64_t pad2[3];
};
static_assert(sizeof(TravelTail) == kTravelTailBytes, "the tail's size");
constexpr uint32_t kTravelTailRejectedWord = 4, kTravelTailCountWord = 6; // the tail as 32-bit words

// ---- a tile
BM_VHD uint32_t travel_tile_index(const TravelDims& d, uint32_t tx, uint32_t ty, uint32_t tz) { return (tz * d.tiles[1] + ty) * d.tiles[0] + tx; }
BM_VHD uint32_t travel_voxel_index(const TravelDims& d, uint32_t x, uint32_t y, uint32_t z) {
	return (z * static_cast<uint32_t>(d.extent[1]) + y) * static_cast<uint32_t>(d.extent[0]) + x;
}

// One sweep of the lane that holds the x-row t[0 ... 7] of a tile.  open: bit i = voxel i may be entered.  near[i]: the least value of
// voxel i of the four neighbouring rows (y - 1, y + 1, z - 1, z + 1) inside the tile as they stood before this sweep, kTravelNone where
// there is none.  First every open voxel takes near + 1, then the row is walked up and down, which settles it in itself.  Candidates
// above `limit` (at most kTravelMaxSteps) are not taken; kTravelNone + 1 is above every limit.  True when a value fell.
// Bound: after s sweeps every voxel is final whose best derivation inside the tile changes rows at most s times; a derivation visits no
// voxel twice, so it changes rows fewer than 512 times, and sweep kTravelTileSweeps at the latest changes nothing.
// (Written without branches: a blocked voxel's limit is 0, and a candidate is at least 1.)
BM_VHD uint32_t travel_step(uint32_t t, uint32_t from, uint32_t lim) {
	const uint32_t c = from + 1u, m = c < t ? c : t;
	return c <= lim ? m : t;
}
BM_VHD bool travel_row_sweep(uint32_t t[8], uint32_t open, const uint32_t near[8], uint32_t limit) {
	uint32_t diff = 0;
BM_TRAVEL_UNROLL
	for (int i = 0; i < 8; ++i) {
		const uint32_t v = travel_step(t[i], near[i], ((open >> i) & 1u) ? limit : 0u);
		diff |= v ^ t[i];
		t[i] = v;
	}
BM_TRAVEL_UNROLL
	for (int i = 1; i < 8; ++i) {
		const uint32_t v = travel_step(t[i], t[i - 1], ((open >> i) & 1u) ? limit : 0u);
		diff |= v ^ t[i];
		t[i] = v;
	}
BM_TRAVEL_UNROLL
	for (int i = 6; i >= 0; --i) {
		const uint32_t v = travel_step(t[i], t[i + 1], ((open >> i) & 1u) ? limit : 0u);
		diff |= v ^ t[i];
		t[i] = v;
	}
	return diff != 0;
}

// what a voxel takes from a value across one of its faces (the halo of a tile: a constant of the round, applied once)
BM_VHD uint32_t travel_take(uint32_t t, uint32_t from, bool open, uint32_t limit) {
	return travel_step(t, from, open ? limit : 0u);
}

// ---- the record
// the key whose maximum names the largest finite value and, among its voxels, the lowest index (distance.h); 0 (no voxel gives it: an
// index is below 2^31) for none
BM_VHD uint64_t travel_max_key(uint32_t value, uint32_t index) {
	return value == kTravelNone ? 0u : (static_cast<uint64_t>(value) << 32 | (0xFFFFFFFFu - index));
}

// the 32 bytes of a bm_travel_result
struct TravelRecord {
	uint64_t reached;
	uint32_t farthest, seeds_rejected;
	uint64_t farthest_at, reserved;
};
BM_VHD TravelRecord travel_record(uint64_t key, uint64_t reached, uint32_t rejected) {
	if (key == 0) return {reached, kTravelNone, rejected, 0u, 0u};
	return {reached, static_cast<uint32_t>(key >> 32), rejected, static_cast<uint64_t>(0xFFFFFFFFu - static_cast<uint32_t>(key)), 0u};
}

// ---- paths
// The walk from start s over a field read through value(x, y, z) (inside the volume only): emit(k, x, y, z) for the first
// min(length, capacity) voxels, the start first; from p the next voxel is the first neighbour in the order -x, +x, -y, +y, -z, +z that
// lies inside the volume and holds T(p) - 1.  Returns T(s) + 1, 0 when the start is outside the volume or holds kTravelNone, -1 when a
// voxel has no such neighbour (the field was not made by bm_travel_field).  The loop is bounded by T(s) and by capacity.
template <class Value, class Emit>
BM_VHD int32_t travel_walk(const int32_t extent[3], int32_t sx, int32_t sy, int32_t sz, int32_t capacity, Value&& value, Emit&& emit) {
	if (sx < 0 || sy < 0 || sz < 0 || sx >= extent[0] || sy >= extent[1] || sz >= extent[2]) return 0;
	uint32_t t = value(sx, sy, sz);
	if (t >= kTravelNone) return 0;
	const int32_t length = static_cast<int32_t>(t) + 1;
	int32_t x = sx, y = sy, z = sz;
	emit(0, x, y, z);
	for (int32_t k = 1; k < length && k < capacity; ++k) {
		bool found = false;
		int32_t nx = x, ny = y, nz = z;
BM_TRAVEL_UNROLL
		for (int f = 0; f < 6; ++f) {
			const int32_t s = (f & 1) ? 1 : -1;
			const int32_t qx = x + (f >> 1 == 0 ? s : 0), qy = y + (f >> 1 == 1 ? s : 0), qz = z + (f >> 1 == 2 ? s : 0);
			const bool inside = qx >= 0 && qy >= 0 && qz >= 0 && qx < extent[0] && qy < extent[1] && qz < extent[2];
			if (!found && inside && value(qx, qy, qz) == t - 1u) {
				nx = qx;
				ny = qy;
				nz = qz;
				found = true;
			}
		}
		if (!found) return -1;
		x = nx;
		y = ny;
		z = nz;
		--t;
		emit(k, x, y, z);
	}
	return length;
}

} // namespace bm
