// settle.h -- the rules of rigid settling (bm_settle, bm_host_settle, include/brickmap.h), written once for the kernels of settle.hip and
// the plain loops of settle_host.cpp.  Needs no HIP header: tests/settle_check.cpp builds it with a host compiler.
//
// All integers.  A label volume L[z][y][x] (0 = empty, equal non-zero values = one rigid piece), a table of n records in ascending label
// and one byte `chosen` per record.  A solid voxel MOVES when the search below finds its label at a slot whose byte is not 0; every other
// solid voxel, and the floor under z = 0, is static.  In a column, a moving voxel at z whose nearest solid voxel below, at z' (the floor:
// z' = -1), carries another label is a CONTACT (upper, lower, g = z - z' - 1).  The drops are the greatest values with
// drop(upper) <= drop(lower) + g over all contacts, static pieces and the floor at 0: the shortest-path distance from "ground" in the
// contact graph, whose weights are not negative -- it exists, it is unique, and no order of evaluation can change it.
//
// The device reaches it by relaxation, D(upper) = min(D(upper), D(lower) + g) over all contacts, in rounds, from D = kSettleUnknown for
// the chosen records.  Why late values do no harm: D only ever falls, and every value ever stored is the length of a real chain of
// contacts down to something static, so a value read late is merely larger than it will become, never wrong.  A value that fell in round
// k is seen by round k + 1, a later kernel.  After round r every piece whose shortest chain has at most r contacts is final; a chain
// visits no piece twice, so it has at most as many contacts as there are chosen records.
//
// Why no two voxels land on one.  Two solid voxels of a column, the upper at z and the nearest one below at z': with different labels
// they are a contact, or the upper one is static, and the new gap g + drop(lower) - drop(upper) is not negative either way (a static
// upper has drop 0); with the same label they move together.  So the order within a column is kept, the lowest voxel's chain bounds
// its drop by the empty voxels under it, and z - drop >= 0.
#pragma once
#include <cstddef>
#include <cstdint>

#include "device_types.h"

namespace bm {

constexpr uint32_t kSettleUnknown = 0x7FFFFFFFu;          // "not yet known": never added to
constexpr int kSettleMaxExtent = 16384;                    // the limits of bm_distance_params
constexpr int64_t kSettleMaxVoxels = (int64_t{1} << 31) - 2;
constexpr int kSettleSlices = 16;                          // slices whose loads a column walk keeps in flight per wait (measured: DESIGN.md 4.19)
constexpr uint32_t kSettleBatch = 8;                       // rounds enqueued between two looks of the host (measured: DESIGN.md 4.19)
constexpr size_t kSettleTailBytes = 64;                    // the workspace's last bytes, see SettleTail
constexpr size_t kSettleRecordBytes = 40;                  // a bm_component; its label is its first word

// null, or why these extents are refused
inline const char* settle_extent_problem(const int32_t extent[3]) {
	for (int k = 0; k < 3; ++k)
		if (extent[k] < 1 || extent[k] > kSettleMaxExtent) return "an extent below 1 or above 16384";
	if (static_cast<int64_t>(extent[0]) * extent[1] > kSettleMaxVoxels / extent[2]) return "more than 2^31 - 2 voxels";
	return nullptr;
}

// what the kernels and the loops need of the extents
struct SettleDims {
	int32_t nz;
	uint32_t columns; // nx * ny: the index of column (x, y) is y nx + x, and voxel (x, y, z) is word z * columns + column
	uint32_t groups;  // groups of 64 consecutive columns: what one wave walks
	uint32_t voxels;  // below 2^31 - 1
	uint32_t n;       // records
};
inline SettleDims settle_dims(const int32_t extent[3], int64_t n) {
	SettleDims d;
	d.nz = extent[2];
	d.columns = static_cast<uint32_t>(extent[0]) * static_cast<uint32_t>(extent[1]);
	d.groups = (d.columns + 63u) >> 6;
	d.voxels = d.columns * static_cast<uint32_t>(extent[2]);
	d.n = static_cast<uint32_t>(n);
	return d;
}

// The workspace: D, one word per record; one word per column group (round 1 notes whether the group holds a contact); the tail.  Every
// part is a multiple of 16 bytes.  Bytes per piece and per 64 columns, none per voxel.  The workspace need only be 4-byte aligned; the
// tail holds 64-bit sums, so it begins at the first 8-byte aligned address at or after its offset, and 8 bytes are there for that.
inline size_t settle_round16(size_t bytes) { return (bytes + 15) & ~static_cast<size_t>(15); }
inline size_t settle_groups_offset(const SettleDims& d) { return settle_round16(static_cast<size_t>(d.n) * 4); }
inline size_t settle_tail_offset(const SettleDims& d) { return settle_groups_offset(d) + settle_round16(static_cast<size_t>(d.groups) * 4); }
inline size_t settle_workspace_bytes(const SettleDims& d) { return settle_tail_offset(d) + kSettleTailBytes + 8; }
inline uint32_t* settle_tail_at(const SettleDims& d, void* workspace) {
	const uintptr_t p = reinterpret_cast<uintptr_t>(workspace) + settle_tail_offset(d);
	return reinterpret_cast<uint32_t*>((p + 7) & ~static_cast<uintptr_t>(7));
}

// the tail, zeroed by every call: the sums of the record, and the three rotating counts of changes -- round k adds under count[k % 3],
// reads count[(k - 1) % 3] (a round whose predecessor changed nothing returns at once) and zeroes count[(k + 1) % 3], which round k - 1
// read and round k + 1 adds under.  `chosen` lies beside the counts: the host reads those 16 bytes in one copy.
struct SettleTail {
	uint64_t moved_voxels, contacts;
	uint32_t moved_pieces, largest_drop, pad[2];
	uint32_t count[3], chosen;
	uint64_t pad1[2];
};
static_assert(sizeof(SettleTail) == kSettleTailBytes, "the tail's size");
constexpr uint32_t kSettleTailMovedWord = 4, kSettleTailLargestWord = 5, kSettleTailCountWord = 8, kSettleTailChosenWord = 11; // the tail as 32-bit words

// ---- who moves
// The slot of `label` in a table of n records whose labels label_at(slot) ascend, or -1: a lower bound and one comparison.  Every
// kernel and the host routine use this one search, so a table that does not ascend, or names a label twice, still gives every label one
// answer.  Bounded by log2 n + 1 steps; it reads slots below n only.
template <class LabelAt>
BM_VHD int32_t settle_find(LabelAt&& label_at, uint32_t n, int32_t label) {
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (label_at(mid) < label) lo = mid + 1; else hi = mid;
	}
	return lo < n && label_at(lo) == label ? static_cast<int32_t>(lo) : -1;
}
// the slot of a moving label, -1 for a static one
template <class LabelAt, class ChosenAt>
BM_VHD int32_t settle_moving_slot(LabelAt&& label_at, ChosenAt&& chosen_at, uint32_t n, int32_t label) {
	const int32_t slot = settle_find(label_at, n, label);
	return slot >= 0 && chosen_at(static_cast<uint32_t>(slot)) != 0 ? slot : -1;
}

// ---- a column, walked upwards
// what a walk keeps of the nearest solid voxel below: its label, its height and its moving slot (-1: static).  The floor is {0, -1, -1}:
// no solid voxel carries label 0.
struct SettleBelow {
	int32_t label, z, slot;
};
BM_VHD SettleBelow settle_floor() { return {0, -1, -1}; }

struct SettleContact {
	int32_t upper, lower; // slots; lower -1 = static or the floor
	int32_t gap;
};

// The step for the solid voxel (label != 0) at height z: `below` becomes this voxel; true when the pair is a contact, which `c` then
// holds.  moving_slot(label) is asked only where the label changes.
template <class MovingSlot>
BM_VHD bool settle_step(SettleBelow& below, int32_t label, int32_t z, MovingSlot&& moving_slot, SettleContact& c) {
	const bool same = label == below.label;
	const int32_t slot = same ? below.slot : moving_slot(label);
	const bool contact = !same && slot >= 0;
	c.upper = slot;
	c.lower = below.slot;
	c.gap = z - below.z - 1;
	below.label = label;
	below.z = z;
	below.slot = slot;
	return contact;
}

// the candidate drop(lower) + g; kSettleUnknown is never added to.  (A known drop is at most nz and a gap is below nz: no overflow.)
BM_VHD uint32_t settle_candidate(uint32_t lower_drop, int32_t gap) { return lower_drop == kSettleUnknown ? kSettleUnknown : lower_drop + static_cast<uint32_t>(gap); }

// the drop a record ends with: a chosen record that no voxel's search arrives at (a label without voxels, the second of two equal
// labels) has no contact and keeps kSettleUnknown to the end -- it falls nowhere
BM_VHD uint32_t settle_final_drop(uint32_t d) { return d == kSettleUnknown ? 0u : d; }

// the byte the move writes at z - drop
BM_VHD uint32_t settle_byte(uint32_t drop) { return drop == 0 ? 1u : 2u; }

// ---- the record: the 32 bytes of a bm_settle_result
struct SettleRecord {
	uint64_t moved_voxels;
	uint32_t chosen_pieces, moved_pieces, largest_drop, reserved;
	uint64_t contacts;
};

} // namespace bm
