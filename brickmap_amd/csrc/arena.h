// arena.h -- the brick arena: one device address range that every supercell's pool lives in (Scene.cpp:152-175,231-251 made one
// allocator).  Which region is whose is arithmetic without HIP, RegionLists (pool_book.h), held here as a member; this class keeps the
// address range and maps memory before the top of the regions moves.  The arena is a RESERVED VIRTUAL RANGE sized for the world's worst case into which
// physical chunks are mapped as residency grows (hipMemAddressReserve / hipMemCreate / hipMemMap): growing it
// neither copies a brick nor synchronises the device, and every pointer into it stays valid for frames in flight.
// (Devices without virtual memory management fall back to reallocate + copy behind a device synchronisation.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pool_book.h"

namespace bm {

class BrickArena {
public:
	BrickArena() = default;
	BrickArena(const BrickArena&) = delete;
	BrickArena& operator=(const BrickArena&) = delete;
	~BrickArena() { close(); }

	int open(int device, uint64_t max_bricks); // reserve the address range (once per world); base() may change
	void close();
	void reset() { regions_.reset(); }         // nothing handed out, nothing free-listed; what is mapped stays mapped
	// make the arena at least this large (contents kept); exact: (re)size an EMPTY arena to fit.  *left_unmapped: the emptied arena
	// was unmapped and could not be mapped again.  base() may change (reallocate + copy devices only).
	int reserve(uint64_t bricks, bool exact = false, bool* left_unmapped = nullptr);
	int region_alloc(uint32_t bricks, uint32_t* offset); // a region for one pool: a free one of that size, else the arena grows to hold it at the top
	uint32_t claim_top(uint64_t bricks) { return regions_.claim_top(bricks); } // an exact-fit pool from the top of a reserve()d arena: its offset
	RegionLists& regions() { return regions_; } // where vacated regions go back to (pool_book.h)

	uint32_t* base() const { return base_; }
	bool is_virtual() const { return virtual_; }
	uint64_t capacity() const { return capacity_; }       // bricks mapped
	uint64_t pool_bricks() const { return regions_.pool_bricks(); } // bricks of capacity currently handed to pools
	uint64_t growths() const { return growths_; }         // times the arena grew / grew by synchronise + copy
	uint64_t copy_growths() const { return copy_growths_; }

private:
	struct Chunk { hipMemGenericAllocationHandle_t handle; size_t offset, bytes; };
	int unmap_all();

	int device_ = 0;
	uint32_t* base_ = nullptr;
	bool virtual_ = false;
	size_t va_bytes_ = 0, granularity_ = 0;
	std::vector<Chunk> chunks_;
	uint64_t growths_ = 0, copy_growths_ = 0;
	uint64_t capacity_ = 0; // bricks mapped
	RegionLists regions_;
};

} // namespace bm
