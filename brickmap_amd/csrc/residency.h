// residency.h -- which brick is resident where, with one owner: the index grid and the pool bases, the brick arena, the two request rings with
// their pinned mirrors, the staging of an upload batch, and the book that takes every decision about them (pool_book.h, host only, scripted on
// the CPU by tests/pool_book_check.cpp).  This class holds the HIP objects and makes the calls.  A Scene holds one; it keeps the world, the walk
// fields and the ordering, and hands over the FrameOrder and the load stream where a batch is published.  The pointers of the device view that
// are residency's (index_grid, pool_base, brick_arena, load_queue, load_queue_count, queue_cap) are written here, into the view given to init.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/brickmap.h"
#include "arena.h"
#include "device_types.h"
#include "error.h"
#include "frame_order.h"
#include "hip_owned.h"
#include "pool_book.h"
#include "world.h"

namespace bm {

class Residency {
public:
	Residency(int device, World* world) : device_(device), world_(world), book_(&arena_.regions()) {}

	int init(DeviceScene* view); // the rings' counters and their pinned mirrors
	int alloc_queue();           // rings, mirrors and staging for the queue capacity; ring 0 is current
	int set_queue_capacity(int cap);
	int queue_capacity() const { return queue_cap_; }
	int set_streaming_mode(int overlapped, FrameOrder& order, hipStream_t load_stream);

	// ---- the device memory of a world
	int alloc_index_grid();                   // the flat index grid and one pool-base word per supercell
	int open_arena(uint64_t world_bricks);    // the arena's address range, for a world of so many bricks
	int arena_fit(uint64_t bricks);           // empty the arena and size it for a known residency
	void release();
	uint32_t* index_grid() const { return d_index_grid_; }
	uint32_t* pool_base() const { return d_pool_base_; }
	uint32_t* arena_base() const { return arena_.base(); }

	// ---- a new residency; each leaves the book rebuilt (the caller tells the fields and the ordering)
	int reset();                              // reference initial state: every non-empty brick is "unloaded | lod", nothing resident (Scene.cpp:157-175)
	int preload_all(hipStream_t load_stream); // every pool is its supercell's host brick vector
	// a world that the device has just built in the preloaded layout (load.hip): begin_adopt, adopt every supercell (from any thread) once its host
	// bricks are in place, adopted
	void begin_adopt() { book_.begin_rebuild(world_->dims.supercells); }
	void adopt(int sci, uint32_t base) { book_.adopt_exact(sci, base, world_->supercells[sci].bricks.size(), world_->supercells[sci].free_slots); }
	void adopted(uint64_t total_bricks); // the pools are the first total_bricks bricks of the arena
	int clear_ring_counts(hipStream_t stream);

	// ---- streaming: what bm_scene_process_load_queue does once the scene has passed its own checks
	int process_load_queue(FrameOrder& order, hipStream_t load_stream, uint32_t* serviced);

	// ---- the device half of a change of the host world (Scene stages and submits it): begin_batch, rebind every changed supercell, commit_batch
	// once the batch is queued -- or report why it was not
	void begin_batch() { book_.begin_batch(); }
	int rebind(int sci, const std::vector<uint32_t>& old_words, const uint8_t* touched);
	const std::vector<PoolMove>& moves() const { return book_.moves(); }
	void commit_batch() { book_.commit_batch(); }
	int report(int e) { return book_.report(e); } // what queueing a batch answered: an error leaves the host ahead of the device, the scene is failed
	const PoolBook& book() const { return book_; }

	// ---- readbacks, each the body of the C-ABI call of its name once the scene is on the device; info: the residency lines of bm_scene_info
	int device_indices(int supercell, uint32_t* out4096);
	int device_brick(int supercell, uint32_t device_slot, uint32_t* out16);
	int dump(const char* path);
	void info(bool on_device, bm_scene_info* out) const;

private:
	void rebuilt(bool preloaded); // the book's rebuilt, and what follows from it here: ring 0 in the view, no snapshot pending
	void use_ring(int ring); // the request ring that frames issued from now on append to
	int pool_region(uint32_t bricks, uint32_t* offset); // BrickArena::region_alloc, with the device view following the arena's base
	auto region_alloc() { return [this](uint32_t bricks, uint32_t* offset) { return pool_region(bricks, offset); }; }
	int said(int e); // the book's own message, where it has one, becomes the error string
	int service_ring(int ring, uint32_t count, FrameOrder& order, hipStream_t load_stream, uint32_t* serviced);

	int device_;
	World* world_;
	DeviceScene* view_ = nullptr;
	DeviceBuffer<uint32_t> d_index_grid_, d_pool_base_;
	BrickArena arena_; // every supercell's pool (arena.h); view_->brick_arena follows its base
	PoolBook book_;
	// two request rings (pool_book.h says which one does what), their counters, and the pinned mirrors they are copied out into
	DeviceBuffer<int> d_load_queue_[2];
	DeviceBuffer<uint32_t> d_load_count_[2];
	PinnedBuffer<int> h_positions_[2];
	PinnedBuffer<uint32_t> h_count_[2];
	Turn snapshot_; // pending: the book's snapshot ring is being copied out on the load stream
	// an upload batch: pinned staging (Scene.cpp:30-32) and its device copies; a ring's entries without the stale ones, when some were skipped;
	// the batch's pool moves
	PinnedBuffer<uint32_t> h_bricks_, h_indices_;
	DeviceBuffer<uint32_t> d_bricks_queue_, d_indices_queue_;
	DeviceBuffer<int> d_positions_;
	PinnedBuffer<PoolMove> h_moves_;
	DeviceBuffer<PoolMove> d_moves_;
	int queue_cap_ = 1024; // variables.h:35
};

} // namespace bm
