// foot.h -- the rules of ground navigation (bm_foot_room, bm_foot_field, bm_foot_paths, include/brickmap.h), written once for the kernels
// of foot.hip and the plain loops of foot_host.cpp.  Needs no HIP header: tests/foot_check.cpp builds it with a host compiler.
//
// All integers.  A byte volume V[z][y][x] (non-zero = blocked, z up) gives a room byte per voxel: the low 7 bits R = the free voxels from
// this one upwards, capped at 127 (0 = blocked; everything above the volume is free), bit 7 = free with a blocked voxel -- or the floor
// under z = 0 -- below.  An agent of `height` h STANDS on p when p is supported and R(p) >= h.  A MOVE p -> q goes to one of the four
// neighbouring columns, between two stands, with -drop <= dz <= climb, and the lower of the two has R >= h + |dz|: the agent rises or
// falls in the lower voxel's column and crosses sideways at the upper height.  Every move costs 1, so W(p), the least number of moves
// from a seed, is a breadth-first distance in a directed graph: unique, and no order of evaluation can change it.
//
// The device goes level by level.  The stands that hold k are a segment of one queue of linear voxel indices; round k + 1 gives every
// legal target of such a stand min(W, k + 1) with an atomic, and the lane whose atomic returns kFootNone appends the target.  A stand
// enters the queue once, every store is final, and two lanes that find q in one round offer the same value: the field's bytes depend on
// no order.  Only the order inside a level does, and nothing visible reads it.
//
// BM_FOOT_TOWARD asks for the moves from p to a seed: the same search over reversed moves, which is the search with climb and drop
// exchanged (the condition on the lower voxel is symmetric).  FootDims::up and ::down are the two as the search uses them.
#pragma once
#include <cstddef>
#include <cstdint>

#include "device_types.h"

namespace bm {

constexpr uint32_t kFootNone = 0x7FFFFFFFu;            // BM_FOOT_NONE
constexpr uint32_t kFootMaxSteps = 0x7FFFFFFEu - 1u;   // every finite value is below 2^31 - 2
constexpr uint32_t kFootToward = 1u, kFootNoFloor = 2u; // BM_FOOT_TOWARD, BM_FOOT_NO_FLOOR
constexpr uint32_t kFootRoomCap = 127u, kFootSupported = 0x80u;
constexpr int kFootMaxHeight = 32, kFootMaxClimb = 32, kFootMaxDrop = 64;
constexpr int kFootMaxExtent = 16384;                  // the limits of bm_travel_params
constexpr int64_t kFootMaxVoxels = (int64_t{1} << 31) - 2;
constexpr int kFootSlices = 16;                        // slices whose loads the column walk of foot_room keeps in flight per wait
constexpr int kFootHeights = 4;                        // room bytes of a neighbouring column a lane of foot_level loads per wait
constexpr uint32_t kFootMaxWaves = 1024;               // the grid of a round at most; its waves stride over the front
constexpr uint32_t kFootBatch = 16;                    // rounds enqueued between two looks of the host at the next front's size
constexpr size_t kFootTailBytes = 64;                  // the workspace's last bytes, see FootTail

struct FootParamsView {
	int32_t extent[3];
	uint32_t max_steps;
	int64_t row_pitch, slice_pitch;
	uint32_t flags, reserved;
	int32_t height, climb, drop, reserved2;
};

// the view of a bm_foot_params (a template, so that this header needs no other)
template <class P>
inline FootParamsView foot_params_view(const P& p) {
	return {{p.extent[0], p.extent[1], p.extent[2]}, p.max_steps, p.row_pitch, p.slice_pitch, p.flags, p.reserved, p.height, p.climb, p.drop, p.reserved2};
}

// null, or why these extents are refused
inline const char* foot_extent_problem(const int32_t extent[3]) {
	for (int k = 0; k < 3; ++k)
		if (extent[k] < 1 || extent[k] > kFootMaxExtent) return "an extent below 1 or above 16384";
	if (static_cast<int64_t>(extent[0]) * extent[1] > kFootMaxVoxels / extent[2]) return "more than 2^31 - 2 voxels";
	return nullptr;
}

// null, or why the foot calls refuse these parameters (pitches as given: 0 = tight); the order is that of travel_params_problem, then the agent
inline const char* foot_params_problem(const FootParamsView& p) {
	if ((p.flags & ~(kFootToward | kFootNoFloor)) != 0) return "unknown flag";
	if (p.reserved != 0 || p.reserved2 != 0) return "reserved is not 0";
	if (const char* why = foot_extent_problem(p.extent)) return why;
	if (p.row_pitch < 0 || p.slice_pitch < 0) return "negative pitch";
	if (p.row_pitch > (int64_t{1} << 40)) return "row_pitch above 2^40";
	const int64_t row = p.row_pitch ? p.row_pitch : p.extent[0];
	if (row < p.extent[0]) return "row_pitch below the extent along x";
	if (p.slice_pitch && p.slice_pitch / p.extent[1] < row) return "slice_pitch below row_pitch * the extent along y";
	if ((p.slice_pitch ? p.slice_pitch : row * p.extent[1]) > (int64_t{1} << 46) / p.extent[2]) return "a volume spanning more than 2^46 bytes";
	if (p.height < 1 || p.height > kFootMaxHeight) return "a height outside 1 ... 32";
	if (p.climb < 0 || p.climb > kFootMaxClimb) return "a climb outside 0 ... 32";
	if (p.drop < 0 || p.drop > kFootMaxDrop) return "a drop outside 0 ... 64";
	return nullptr;
}

// what the kernels and the loops need of the parameters
struct FootDims {
	int32_t extent[3];
	uint32_t limit;                 // the largest value that is taken: max_steps, or kFootMaxSteps without a limit
	uint32_t voxels, columns;       // below 2^31 - 1; nx * ny
	uint32_t queue;                 // entries of the queue: ceil(nz / 2) * columns, since two stands of a column are never adjacent
	int32_t height, up, down;       // the search goes from a stand to the stands of a neighbouring column at dz in -down ... up
	uint32_t floor;                 // 1: the bottom of the volume supports
	int64_t row_pitch, slice_pitch; // of the byte volume, resolved: never 0
};

inline FootDims foot_dims(const FootParamsView& p) {
	FootDims d;
	for (int k = 0; k < 3; ++k) d.extent[k] = p.extent[k];
	d.limit = p.max_steps != 0 && p.max_steps < kFootMaxSteps ? p.max_steps : kFootMaxSteps;
	d.columns = static_cast<uint32_t>(p.extent[0]) * static_cast<uint32_t>(p.extent[1]);
	d.voxels = d.columns * static_cast<uint32_t>(p.extent[2]);
	d.queue = d.columns * ((static_cast<uint32_t>(p.extent[2]) + 1u) >> 1);
	d.height = p.height;
	const bool toward = (p.flags & kFootToward) != 0;
	d.up = toward ? p.drop : p.climb;
	d.down = toward ? p.climb : p.drop;
	d.floor = (p.flags & kFootNoFloor) ? 0u : 1u;
	d.row_pitch = p.row_pitch ? p.row_pitch : p.extent[0];
	d.slice_pitch = p.slice_pitch ? p.slice_pitch : d.row_pitch * p.extent[1];
	return d;
}

// bytes from the byte volume's first byte to one past its last
inline uint64_t foot_span(const FootDims& d) {
	return static_cast<uint64_t>(d.extent[2] - 1) * static_cast<uint64_t>(d.slice_pitch) + static_cast<uint64_t>(d.extent[1] - 1) * static_cast<uint64_t>(d.row_pitch) +
		   static_cast<uint64_t>(d.extent[0]);
}

// The workspace: the queue, 4 bytes per entry (2 bytes per voxel at most), rounded up to 16, then the tail.
inline size_t foot_tail_offset(const FootDims& d) { return (static_cast<size_t>(d.queue) * 4 + 15) & ~static_cast<size_t>(15); }
inline size_t foot_workspace_bytes(const FootDims& d) { return foot_tail_offset(d) + kFootTailBytes; }

// the tail, zeroed by every call.  Level j -- the stands that hold j; the accepted seeds are level 0 -- is the queue's segment
// [begin[j % 3], begin[j % 3] + count[j % 3]).  Round k (1, 2, ...) reads begin and count of level k - 1, appends level k behind it under
// count[k % 3], writes begin[k % 3] for the next round and zeroes count[(k + 1) % 3], which round k - 1 read and round k + 1 appends
// under.  After `done` rounds the next front is level `done`, and begin + count of it is the number of stands reached.
struct FootTail {
	uint64_t key;
	uint32_t standable, rejected;
	uint32_t count[3], pad0;
	uint32_t begin[3], pad1;
	uint64_t pad2[2];
};
static_assert(sizeof(FootTail) == kFootTailBytes, "the tail's size");
constexpr uint32_t kFootTailStandableWord = 2, kFootTailRejectedWord = 3, kFootTailCountWord = 4, kFootTailBeginWord = 8; // the tail as 32-bit words

// ---- the room byte
// A column is walked downwards with the running count of free voxels, which starts at the cap: everything above the volume is free.
BM_VHD uint32_t foot_room_run(uint32_t run_above, bool blocked) { return blocked ? 0u : (run_above < kFootRoomCap ? run_above + 1u : kFootRoomCap); }
// the byte of a voxel whose count is `run`, given whether what lies below it supports (a blocked voxel; under z = 0 the floor, if any)
BM_VHD uint32_t foot_room_byte(uint32_t run, bool below_supports) { return run | (run != 0 && below_supports ? kFootSupported : 0u); }

// ---- stands and moves, from room bytes alone
BM_VHD bool foot_stand(uint32_t room, int32_t height) { return (room & kFootSupported) != 0 && (room & kFootRoomCap) >= static_cast<uint32_t>(height); }
// p -> q between neighbouring columns with dz = z(q) - z(p), whatever climb and drop allow: both are stands and the lower one has room
// for the agent and the difference.  Symmetric in p and q.
BM_VHD bool foot_move(uint32_t room_p, uint32_t room_q, int32_t dz, int32_t height) {
	const uint32_t lower = dz >= 0 ? room_p : room_q;
	return foot_stand(room_p, height) && foot_stand(room_q, height) && (lower & kFootRoomCap) >= static_cast<uint32_t>(height + (dz >= 0 ? dz : -dz));
}
// the four columns in the order of the paths: -x, +x, -y, +y
BM_VHD int32_t foot_dir_x(int dir) { return dir == 0 ? -1 : dir == 1 ? 1 : 0; }
BM_VHD int32_t foot_dir_y(int dir) { return dir == 2 ? -1 : dir == 3 ? 1 : 0; }

BM_VHD uint32_t foot_voxel_index(const FootDims& d, int32_t x, int32_t y, int32_t z) {
	return static_cast<uint32_t>(z) * d.columns + static_cast<uint32_t>(y) * static_cast<uint32_t>(d.extent[0]) + static_cast<uint32_t>(x);
}

// One pair (front node, direction) of a round: the node p = `index` holds level - 1; offer(q) is called for every legal target q in the
// column `dir`, in ascending z.  room(i) reads a room byte.  The loop is bounded by up + down + 1.
template <class Room, class Offer>
BM_VHD void foot_expand(const FootDims& d, uint32_t index, int dir, Room&& room, Offer&& offer) {
	const int32_t nx = d.extent[0], ny = d.extent[1], nz = d.extent[2];
	const int32_t z = static_cast<int32_t>(index / d.columns), c = static_cast<int32_t>(index - static_cast<uint32_t>(z) * d.columns), y = c / nx, x = c - y * nx;
	const int32_t qx = x + foot_dir_x(dir), qy = y + foot_dir_y(dir);
	if (qx < 0 || qy < 0 || qx >= nx || qy >= ny) return;
	const uint32_t rp = room(index);
	const int32_t z0 = z - d.down < 0 ? 0 : z - d.down, z1 = z + d.up >= nz ? nz - 1 : z + d.up;
	for (int32_t qz = z0; qz <= z1; ++qz) {
		const uint32_t q = foot_voxel_index(d, qx, qy, qz);
		if (foot_move(rp, room(q), qz - z, d.height)) offer(q);
	}
}

// ---- the record
// the key whose maximum names the largest finite value and, among its voxels, the lowest index (travel.h); 0 for none
BM_VHD uint64_t foot_max_key(uint32_t value, uint32_t index) {
	return value >= kFootNone ? 0u : (static_cast<uint64_t>(value) << 32 | (0xFFFFFFFFu - index));
}

// the 32 bytes of a bm_foot_result
struct FootRecord {
	uint64_t reached;
	uint32_t farthest, seeds_rejected;
	uint64_t farthest_at, standable;
};
BM_VHD FootRecord foot_record(uint64_t key, uint64_t reached, uint32_t rejected, uint64_t standable) {
	if (key == 0) return {reached, kFootNone, rejected, 0u, standable};
	return {reached, static_cast<uint32_t>(key >> 32), rejected, static_cast<uint64_t>(0xFFFFFFFFu - static_cast<uint32_t>(key)), standable};
}

// ---- paths
// The walk from start s over a field read through value(i) and the room bytes read through room(i) (linear indices inside the volume):
// emit(k, x, y, z) for the first min(length, capacity) voxels, the start first; from p the next voxel is the first q that holds W(p) - 1
// and whose move is legal, the columns in the order -x, +x, -y, +y and inside a column in ascending z.  The walk goes against the search:
// q lies at dz in -up ... down of p.  Returns W(s) + 1, 0 when the start is outside the volume or holds no finite value, -1 when no q
// qualifies (the field was not made by bm_foot_field from this room and these parameters).  Bounded by W(s), capacity and up + down + 1.
template <class Value, class Room, class Emit>
BM_VHD int32_t foot_walk(const FootDims& d, int32_t sx, int32_t sy, int32_t sz, int32_t capacity, Value&& value, Room&& room, Emit&& emit) {
	const int32_t nx = d.extent[0], ny = d.extent[1], nz = d.extent[2];
	if (sx < 0 || sy < 0 || sz < 0 || sx >= nx || sy >= ny || sz >= nz) return 0;
	uint32_t t = value(foot_voxel_index(d, sx, sy, sz));
	if (t >= kFootNone) return 0;
	const int32_t length = static_cast<int32_t>(t) + 1;
	int32_t x = sx, y = sy, z = sz;
	emit(0, x, y, z);
	for (int32_t k = 1; k < length && k < capacity; ++k) {
		const uint32_t rp = room(foot_voxel_index(d, x, y, z));
		bool found = false;
		int32_t fx = x, fy = y, fz = z;
		for (int dir = 0; dir < 4 && !found; ++dir) {
			const int32_t qx = x + foot_dir_x(dir), qy = y + foot_dir_y(dir);
			if (qx < 0 || qy < 0 || qx >= nx || qy >= ny) continue;
			const int32_t z0 = z - d.up < 0 ? 0 : z - d.up, z1 = z + d.down >= nz ? nz - 1 : z + d.down;
			for (int32_t qz = z0; qz <= z1 && !found; ++qz) {
				const uint32_t q = foot_voxel_index(d, qx, qy, qz);
				if (value(q) == t - 1u && foot_move(rp, room(q), qz - z, d.height)) {
					fx = qx;
					fy = qy;
					fz = qz;
					found = true;
				}
			}
		}
		if (!found) return -1;
		x = fx;
		y = fy;
		z = fz;
		--t;
		emit(k, x, y, z);
	}
	return length;
}

} // namespace bm
