// pool_book.h -- which brick is resident where.  Host only, no HIP: the book holds no buffer, event or stream (residency.h owns those and keeps the
// book).  It holds what is pure bookkeeping -- every supercell's pool (region of the arena, capacity, high-water mark, host slot -> device slot,
// freed device slots), whether the scene is preloaded or has failed, the resident total, the statistics of the upload batches, and which of the
// two request rings does what -- and it takes every decision about them: the one slot rule, the one growth size, the one record of a batch's pool
// moves, the one device word of a cell, the one test that a brick is absent.  RegionLists is the arithmetic of the arena's regions, which
// BrickArena (arena.h) holds as a member.  tests/pool_book_check.cpp scripts both on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/brickmap.h"
#include "device_types.h"

namespace bm {

constexpr uint16_t kNoDeviceSlot = 0xFFFF; // a host slot whose brick is not resident

// The regions of the arena: powers of two of at least kStartingPool bricks, handed out from per-size free lists (take_free) or from the top
// (claim_top -- the owner makes sure the arena reaches that far first).  A vacated region becomes reusable once the batch that vacates it has been
// queued (commit_freed): its move kernel still reads it, and a pool growing in the SAME batch must not be given it (later batches are ordered behind
// this one on the load stream).
class RegionLists {
public:
	static constexpr uint32_t kStartingPool = 16; // supergrid_starting_size, variables.h:15

	void reset() { // nothing handed out, nothing free-listed
		top_ = pool_bricks_ = 0;
		for (auto& f : free_) f.clear();
		freed_this_batch_.clear();
	}
	uint64_t top() const { return top_; }                 // bricks below it have been handed out at some time
	uint64_t pool_bricks() const { return pool_bricks_; } // bricks currently handed to pools
	bool take_free(uint32_t bricks, uint32_t* offset) {   // a free region of `bricks` (a power of two >= kStartingPool); false: there is none, claim the top
		int cls = 0;
		while ((1u << cls) < bricks) ++cls;
		if (free_[cls].empty()) return false;
		*offset = free_[cls].back();
		free_[cls].pop_back();
		pool_bricks_ += bricks;
		return true;
	}
	uint32_t claim_top(uint64_t bricks) { // also an exact-fit pool (preloaded residency), of any size: its offset
		const uint32_t offset = static_cast<uint32_t>(top_);
		top_ += bricks;
		pool_bricks_ += bricks;
		return offset;
	}
	// The region is filed under the largest power of two it holds: a grown pool is one, and of a preloaded pool -- an exact fit -- only that much is
	// handed out again.
	void free_deferred(uint32_t bricks, uint32_t offset) {
		int cls = 0;
		while ((2u << cls) <= bricks) ++cls;
		freed_this_batch_.emplace_back(cls, offset);
		pool_bricks_ -= bricks;
	}
	void commit_freed() {
		for (const auto& f : freed_this_batch_) free_[f.first].push_back(f.second);
		freed_this_batch_.clear();
	}
	const std::vector<uint32_t>& free_regions(int cls) const { return free_[cls]; }

private:
	uint64_t top_ = 0, pool_bricks_ = 0;
	std::vector<uint32_t> free_[32];                         // [log2 size]: arena offsets of free regions
	std::vector<std::pair<int, uint32_t>> freed_this_batch_; // (log2 size, offset) of regions vacated by the batch being built
};

// The book.  A function that takes `alloc` may grow a pool: alloc(bricks, &offset) hands out a region of the arena or returns an error code (the
// library passes BrickArena::region_alloc, which maps memory first); vacated regions go back to `regions` by themselves.  A function that can fail
// returns 0 or an error code; why() is the message where the book itself refuses, null where `alloc` has reported its own.
class PoolBook {
public:
	static constexpr uint32_t kStartingPool = RegionLists::kStartingPool;
	struct Pool { // of one supercell (Scene::Supercell gpu_count / gpu_index_highest, Scene.h:24-27)
		uint32_t base = 0;               // first arena slot
		uint32_t capacity = 0;           // bricks it can hold (0 = no pool yet)
		uint32_t high = 0;               // high-water mark: the next device slot never handed out
		std::vector<uint16_t> dev_slot;  // host slot -> device slot (kNoDeviceSlot = not resident)
		std::vector<uint32_t> freed;     // device slots below `high` that edits emptied, handed out again last freed first
		uint32_t resident() const { return high - static_cast<uint32_t>(freed.size()); }

	private:
		friend class PoolBook; // the pool as the current batch found it, and the batch's move of it (-1: it has not grown)
		uint64_t batch = 0;
		uint32_t batch_base = 0, batch_high = 0;
		int batch_move = -1;
	};

	explicit PoolBook(RegionLists* regions) : regions_(regions) {}

	// ---- the rules that are plain functions
	// the device word of a cell whose host word is `host_word` (0, or a host slot | loaded | lod) and whose brick stands in `device_slot`
	static uint32_t device_word(uint32_t host_word, uint32_t device_slot) {
		if (!(host_word & BM_BRICK_LOADED_BIT)) return 0u;
		if (device_slot == kNoDeviceSlot) return BM_BRICK_UNLOADED_BIT | (host_word & BM_BRICK_LOD_BITS); // requested bit clear: asked for again
		return device_slot | BM_BRICK_LOADED_BIT | (host_word & BM_BRICK_LOD_BITS);
	}
	// the capacity a pool of `capacity` grows to so that it holds `need` bricks: it at least doubles (Scene.cpp:231-251: 2^ceil(log2(highest + 1)))
	static uint32_t grown_capacity(uint32_t capacity, uint32_t need) {
		uint32_t grown = kStartingPool;
		while (grown < need || grown < 2 * capacity) grown *= 2;
		return grown;
	}
	// the cell's brick exists and the device does not hold it
	bool absent(int sci, uint32_t host_word) const { return host_word != 0 && pools_[sci].dev_slot[host_word & BM_BRICK_INDEX_BITS] == kNoDeviceSlot; }

	// ---- the scene
	bool preloaded() const { return preloaded_; } // bm_scene_preload_all: an edit uploads new bricks at once (no requests are serviced)
	bool failed() const { return failed_; }       // a batch could not be completed: the residency is undefined until it is rebuilt
	static constexpr const char* kFailedWhy = "a streaming batch failed on this scene: call bm_scene_reset_residency / bm_scene_preload_all";
	// THE place the failed flag is set: whatever a growth, a remapping of the arena or the queueing of a batch answers passes through here
	int report(int e) {
		if (e) failed_ = true;
		return e;
	}
	const char* why() const { return why_; }
	uint64_t resident_bricks() const { return resident_; }
	uint64_t stream_batches() const { return batches_; } // upload batches since the residency was rebuilt / host time staging them
	uint64_t stream_host_ns() const { return host_ns_; }
	void batch_streamed(uint64_t host_ns) { batches_++; host_ns_ += host_ns; }
	const Pool& pool(int sci) const { return pools_[sci]; }
	int pools() const { return static_cast<int>(pools_.size()); }

	// ---- a new residency: begin_rebuild, every supercell's pool by start_pool or adopt_exact, rebuilt
	void begin_rebuild(int supercells) {
		pools_.assign(static_cast<size_t>(supercells), Pool{});
		resident_ = 0;
	}
	// reset: nothing resident, a starting pool for a supercell that holds bricks (Scene.cpp:157-175)
	template <class Alloc> int start_pool(int sci, size_t host_slots, Alloc&& alloc) {
		why_ = nullptr;
		Pool& p = pools_[sci];
		p = Pool{};
		p.dev_slot.assign(host_slots, kNoDeviceSlot);
		if (host_slots == 0) return 0;
		if (int e = alloc(kStartingPool, &p.base)) return report(e);
		p.capacity = kStartingPool;
		return 0;
	}
	// the pool IS its supercell's host brick vector at `base`: exact fit, identity slots; host slots that edits freed keep their place in the pool and
	// are its free slots.  (Pools of different supercells may be adopted from different threads.)
	void adopt_exact(int sci, uint32_t base, size_t host_slots, const std::vector<uint32_t>& free_host_slots) {
		Pool& p = pools_[sci];
		p = Pool{};
		p.base = base;
		p.capacity = p.high = static_cast<uint32_t>(host_slots);
		p.dev_slot.resize(host_slots);
		for (size_t s = 0; s < host_slots; ++s) p.dev_slot[s] = static_cast<uint16_t>(s);
		p.freed = free_host_slots;
	}
	// the host state that goes with a freshly written index grid: ring 0, nothing pending, nothing failed, statistics from zero
	void rebuilt(bool preloaded) {
		rings_reset();
		preloaded_ = preloaded;
		failed_ = false;
		batches_ = host_ns_ = 0;
		resident_ = 0;
		for (const Pool& p : pools_) resident_ += p.resident();
	}

	// ---- a batch: begin_batch, slots handed out (ring_slots / rebind), moves() queued ahead of its scatter, commit_batch once it is queued
	void begin_batch() {
		batch_++;
		moves_.clear();
	}
	// One record per pool that grew in the batch: `count` bricks from `src` to `dst`.  Only the bricks that were resident BEFORE the batch have to be
	// copied (the batch's own bricks are scattered to base + slot after the bases are published), and only once: a pool that grows twice in one batch
	// moves from the region it had when the batch began straight to the last one.  A pool that had no region yet has count 0 and src 0: move_pools
	// reads nothing for such a move, it only publishes dst.
	const std::vector<PoolMove>& moves() const { return moves_; }
	void commit_batch() { regions_->commit_freed(); }

	// THE slot rule, in two steps.  make_room: the pool of `sci` can take `slots` more bricks -- freed slots count first; for the rest it grows to
	// grown_capacity, into a new region.  take_slot: a freed slot, last freed first, else the high-water mark.
	template <class Alloc> int make_room(int sci, uint32_t slots, Alloc&& alloc) {
		Pool& p = in_batch(sci);
		const uint32_t appends = slots - std::min<uint32_t>(slots, static_cast<uint32_t>(p.freed.size()));
		if (p.high + appends <= p.capacity) return 0;
		const uint32_t grown = grown_capacity(p.capacity, p.high + appends);
		uint32_t fresh = 0;
		if (int e = alloc(grown, &fresh)) return report(e);
		if (p.batch_move < 0) {
			p.batch_move = static_cast<int>(moves_.size());
			moves_.push_back(PoolMove{p.batch_base, fresh, p.batch_high, static_cast<uint32_t>(sci)});
		} else {
			moves_[p.batch_move].dst = fresh;
		}
		if (p.capacity > 0) regions_->free_deferred(p.capacity, p.base);
		p.base = fresh;
		p.capacity = grown;
		return 0;
	}
	uint32_t take_slot(int sci) {
		Pool& p = pools_[sci];
		if (p.freed.empty()) return p.high++;
		const uint32_t slot = p.freed.back();
		p.freed.pop_back();
		return slot;
	}

	// ---- a request ring's entries: `count` positions (3 ints each, as the device wrote them).  lookup(px, py, pz, &sci, &host_word, &host_slots):
	// false for a position outside the world, else the cell's supercell, its host index word and the number of host slots of that supercell.
	// check_ring mutates nothing: an entry that cannot be a request marks the scene failed (the ring's counter is still set and the requested bits
	// still stand: every later call would fail the same way while frames went on as if nothing had happened; recovery is a residency reset).
	template <class Lookup> int check_ring(const int* pos, uint32_t count, Lookup&& lookup) {
		if (refuse()) return BM_ESTATE;
		for (uint32_t i = 0; i < count; ++i) {
			int sci = 0;
			uint32_t word = 0;
			size_t host_slots = 0;
			if (!lookup(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], &sci, &word, &host_slots)) {
				why_ = "brick request ring holds a position outside the world";
				return report(BM_ESTATE);
			}
			const uint32_t slot = word & BM_BRICK_INDEX_BITS;
			if (word != 0 && (!(word & BM_BRICK_LOADED_BIT) || slot >= host_slots || slot >= pools_[sci].dev_slot.size())) {
				why_ = "brick request ring names a brick that does not exist";
				return report(BM_ESTATE);
			}
		}
		return 0;
	}
	// ring_slots, on a ring that has passed check_ring: a slot per request, in request order (gpu_index_highest++, Scene.cpp:224), room made for one
	// at a time -- a pool may double twice in a batch.  An entry is stale when an edit has emptied its brick since it was requested, or when its
	// brick is resident already (a brick an edit changed is asked for again, and may then stand in the ring twice): it is skipped and not counted.
	// The kept positions are moved to the front of pos; staged(i, sci, host_word, device_word) hears of kept entry i.  From here on the book
	// changes entry by entry; the only thing that can still go wrong is `alloc`, and that leaves the scene marked as failed.
	template <class Lookup, class Alloc, class Staged> int ring_slots(int* pos, uint32_t count, Lookup&& lookup, Alloc&& alloc, Staged&& staged, uint32_t* kept_out) {
		if (refuse()) return BM_ESTATE;
		uint32_t kept = 0;
		for (uint32_t i = 0; i < count; ++i) {
			const int px = pos[3 * i], py = pos[3 * i + 1], pz = pos[3 * i + 2];
			int sci = 0;
			uint32_t word = 0;
			size_t host_slots = 0;
			lookup(px, py, pz, &sci, &word, &host_slots);
			if (!absent(sci, word)) continue; // stale
			const uint32_t i_out = kept++;
			if (i_out != i) { pos[3 * i_out] = px; pos[3 * i_out + 1] = py; pos[3 * i_out + 2] = pz; }
			if (int e = make_room(sci, 1, alloc)) return e;
			const uint32_t slot = take_slot(sci);
			pools_[sci].dev_slot[word & BM_BRICK_INDEX_BITS] = static_cast<uint16_t>(slot);
			resident_++;
			staged(i_out, sci, word, device_word(word, slot));
		}
		*kept_out = kept;
		return 0;
	}

	// ---- the rebinding after a change of the host world: the supercell's index words before and after (4096 each), which cells were touched, and
	// the number of its host slots now.  Untouched cells keep their device slots (their host slots did not move); a resident brick that is still
	// there keeps its slot; one that was emptied frees it; on a preloaded scene a new brick gets a slot at once, by the slot rule, with room made for
	// all of the supercell's new bricks together.  Afterwards pool(sci).dev_slot names the device slot of every host slot.
	template <class Alloc> int rebind(int sci, const uint32_t* old_words, const uint32_t* new_words, const uint8_t* touched, size_t host_slots, Alloc&& alloc) {
		if (refuse()) return BM_ESTATE;
		Pool& p = in_batch(sci);
		constexpr int kCells = 4096;
		rebound_.assign(host_slots, kNoDeviceSlot);
		fresh_.clear();
		for (int j = 0; j < kCells; ++j)
			if (new_words[j] && !touched[j]) rebound_[new_words[j] & BM_BRICK_INDEX_BITS] = p.dev_slot[new_words[j] & BM_BRICK_INDEX_BITS];
		for (int j = 0; j < kCells; ++j) {
			if (!touched[j]) continue;
			const uint32_t ow = old_words[j], nw = new_words[j];
			const uint16_t was = ow ? p.dev_slot[ow & BM_BRICK_INDEX_BITS] : kNoDeviceSlot;
			if (was != kNoDeviceSlot) {
				if (nw) rebound_[nw & BM_BRICK_INDEX_BITS] = was; // resident stays resident, rewritten in place
				else { p.freed.push_back(was); resident_--; }
			} else if (nw && preloaded_) {
				fresh_.push_back(nw & BM_BRICK_INDEX_BITS);
			}
		}
		if (!fresh_.empty()) {
			if (int e = make_room(sci, static_cast<uint32_t>(fresh_.size()), alloc)) return e;
			for (const uint32_t host_slot : fresh_) rebound_[host_slot] = static_cast<uint16_t>(take_slot(sci));
			resident_ += fresh_.size();
		}
		p.dev_slot.swap(rebound_);
		return 0;
	}

	// ---- the two request rings.  The blocking (reference-order) mode only uses ring 0; the overlapped mode alternates them, so that a frame can
	// raise requests while the previous frame's ring is being copied out and serviced.
	bool overlapped() const { return overlapped_; }
	int ring() const { return ring_; } // the ring that frames issued from now on append to
	void rings_reset() { ring_ = 0; snapshot_pending_ = false; }
	// What process_load_queue does next.  Blocking: wait for the frames, read ring 0 and service it (service = 0, snapshot = -1).  Overlapped: service
	// the ring that the call before copied out (service, -1: there is none), then copy out the ring the last frames wrote (snapshot) and hand the other
	// one to the next frames.
	struct QueueStep { int service, snapshot; };
	QueueStep queue_step() const {
		if (!overlapped_) return {0, -1};
		return {snapshot_pending_ ? ring_snapshot_ : -1, ring_};
	}
	void snapshot_read() { snapshot_pending_ = false; } // the pending copy has been waited for
	void snapshot_taken() {                             // the copy of ring() has been queued
		ring_snapshot_ = ring_;
		snapshot_pending_ = true;
		ring_ ^= 1;
	}
	// What a change of mode must do first (the device has been waited for): service the ring that was copied out (drain, -1: none is pending), so that
	// no request is lost; then, where the blocking mode takes over with ring 1 current, carry what the last frames queued there over to ring 0, which
	// is the only one that mode works on.
	struct ModeChange { int drain; bool carry; };
	ModeChange mode_change(bool overlapped) const { return {snapshot_pending_ ? ring_snapshot_ : -1, overlapped_ && !overlapped && ring_ != 0}; }
	void mode_changed(bool overlapped) {
		if (mode_change(overlapped).carry) ring_ = 0;
		overlapped_ = overlapped;
	}

private:
	bool refuse() {
		why_ = failed_ ? kFailedWhy : nullptr;
		return failed_;
	}
	Pool& in_batch(int sci) { // the first touch of a pool in a batch notes what the batch found
		Pool& p = pools_[sci];
		if (p.batch != batch_) {
			p.batch = batch_;
			p.batch_base = p.base;
			p.batch_high = p.high;
			p.batch_move = -1;
		}
		return p;
	}

	RegionLists* regions_;
	std::vector<Pool> pools_;
	bool preloaded_ = false, failed_ = false;
	const char* why_ = nullptr;
	uint64_t resident_ = 0; // resident non-empty bricks
	uint64_t batches_ = 0, host_ns_ = 0;
	uint64_t batch_ = 1;
	std::vector<PoolMove> moves_;
	std::vector<uint16_t> rebound_; // rebind's scratch
	std::vector<uint32_t> fresh_;
	bool overlapped_ = false, snapshot_pending_ = false;
	int ring_ = 0, ring_snapshot_ = 0;
};

} // namespace bm
