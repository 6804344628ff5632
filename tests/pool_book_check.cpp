// pool_book_check.cpp -- a program with its own main around csrc/pool_book.h alone (no HIP, no scene), built plain and with
// -fsanitize=address,undefined by tests/test_pool_book.py.  It scripts residency resets, request rings, changes of the host world, batches and
// the two request rings on the book, over a region allocator that can be told to fail, and after every step compares the book's answer -- which
// slot, which region, which move, which word, which ring -- with values written out here by hand from the rules of pool_book.h.  prints "steps N"
// and "failures N".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../brickmap_amd/csrc/pool_book.h"

namespace {

using bm::kNoDeviceSlot;
using bm::PoolBook;
using bm::PoolMove;
using bm::RegionLists;

long failures = 0, steps = 0;
#define CHECK(cond)                                                                  \
	do {                                                                             \
		++steps;                                                                     \
		if (!(cond)) {                                                               \
			if (++failures <= 20) std::printf("line %d: %s\n", __LINE__, #cond);     \
		}                                                                            \
	} while (0)

constexpr uint32_t kLoaded = BM_BRICK_LOADED_BIT, kUnloaded = BM_BRICK_UNLOADED_BIT;

// the arena of the program: the region lists, and a growth of the arena that fails when it is told to
struct Arena {
	RegionLists regions;
	int fail_at = 0; // the fail_at-th alloc from now returns 77 (0: none does)
	int alloc(uint32_t bricks, uint32_t* offset) {
		if (fail_at > 0 && --fail_at == 0) return 77;
		if (!regions.take_free(bricks, offset)) *offset = regions.claim_top(bricks);
		return 0;
	}
	auto fn() { return [this](uint32_t bricks, uint32_t* offset) { return alloc(bricks, offset); }; }
};

// a host world: supercells side by side along x, 16 cells high and deep; a supercell's host slots are handed out as World::edit_supercell does
struct Supercell {
	std::vector<uint32_t> words = std::vector<uint32_t>(4096, 0u);
	uint32_t host_slots = 0;
	std::vector<uint32_t> free_slots;
	void set(int j, uint32_t lod = 0) {
		uint32_t s;
		if (!free_slots.empty()) { s = free_slots.back(); free_slots.pop_back(); }
		else s = host_slots++;
		words[j] = s | kLoaded | (lod << 12);
	}
	void clear(int j) {
		free_slots.push_back(words[j] & BM_BRICK_INDEX_BITS);
		words[j] = 0;
	}
};
struct World {
	std::vector<Supercell> sc;
	explicit World(std::initializer_list<int> bricks) {
		for (const int n : bricks) {
			sc.emplace_back();
			for (int j = 0; j < n; ++j) sc.back().set(j, 0xAB);
		}
	}
	auto lookup() {
		return [this](int px, int py, int pz, int* sci, uint32_t* word, size_t* host_slots) {
			if (px < 0 || py < 0 || pz < 0 || px >= 16 * static_cast<int>(sc.size()) || py >= 16 || pz >= 16) return false;
			*sci = px / 16;
			*word = sc[*sci].words[(px & 15) + 16 * py + 256 * pz];
			*host_slots = sc[*sci].host_slots;
			return true;
		};
	}
};
void push(std::vector<int>& ring, int sci, int j) { ring.insert(ring.end(), {16 * sci + (j & 15), (j >> 4) & 15, j >> 8}); }

struct Staged { uint32_t i; int sci; uint32_t host_word, device_word; };

// reset: the arena emptied, a starting pool for every supercell that holds bricks
int reset(PoolBook& book, Arena& arena, const World& w) {
	arena.regions.reset();
	book.begin_rebuild(static_cast<int>(w.sc.size()));
	for (size_t i = 0; i < w.sc.size(); ++i)
		if (int e = book.start_pool(static_cast<int>(i), w.sc[i].host_slots, arena.fn())) return e;
	book.rebuilt(false);
	return 0;
}
// preload: every pool is its supercell's host brick vector, one behind the other from the top of the emptied arena
void preload(PoolBook& book, Arena& arena, const World& w) {
	arena.regions.reset();
	book.begin_rebuild(static_cast<int>(w.sc.size()));
	for (size_t i = 0; i < w.sc.size(); ++i) book.adopt_exact(static_cast<int>(i), arena.regions.claim_top(w.sc[i].host_slots), w.sc[i].host_slots, w.sc[i].free_slots);
	book.rebuilt(true);
}
// one ring as a batch: checked, slots handed out, committed.  what it staged goes to *out
int service(PoolBook& book, Arena& arena, World& w, std::vector<int>& ring, uint32_t* kept, std::vector<Staged>* out = nullptr, bool commit = true) {
	const uint32_t count = static_cast<uint32_t>(ring.size() / 3);
	if (int e = book.check_ring(ring.data(), count, w.lookup())) return e;
	book.begin_batch();
	auto staged = [&](uint32_t i, int sci, uint32_t hw, uint32_t dw) { if (out) out->push_back({i, sci, hw, dw}); };
	if (int e = book.ring_slots(ring.data(), count, w.lookup(), arena.fn(), staged, kept)) return e;
	if (commit) book.commit_batch();
	return 0;
}
// a change of one supercell of the host world as a batch of its own: cells cleared, then cells set
int edit(PoolBook& book, Arena& arena, World& w, int sci, const std::vector<int>& clear, const std::vector<int>& set, bool commit = true) {
	Supercell& c = w.sc[sci];
	const std::vector<uint32_t> old_words = c.words;
	std::vector<uint8_t> touched(4096, 0);
	for (const int j : clear) { c.clear(j); touched[j] = 1; }
	for (const int j : set) { c.set(j, 0x11); touched[j] = 1; }
	book.begin_batch();
	if (int e = book.rebind(sci, old_words.data(), c.words.data(), touched.data(), c.host_slots, arena.fn())) return e;
	if (commit) book.commit_batch();
	return 0;
}
bool is(const PoolMove& m, uint32_t src, uint32_t dst, uint32_t count, uint32_t supercell) { return m.src == src && m.dst == dst && m.count == count && m.supercell == supercell; }
bool pool_is(const PoolBook& book, int sci, uint32_t base, uint32_t capacity, uint32_t high) {
	const PoolBook::Pool& p = book.pool(sci);
	return p.base == base && p.capacity == capacity && p.high == high;
}

// (a) + (b): reset of a world with empty and non-empty supercells, then 40 requests for one supercell in one batch
void reset_and_forty_requests() {
	Arena arena;
	PoolBook book(&arena.regions);
	World w{20, 0, 42, 3};
	CHECK(reset(book, arena, w) == 0);
	CHECK(pool_is(book, 0, 0, 16, 0) && pool_is(book, 1, 0, 0, 0) && pool_is(book, 2, 16, 16, 0) && pool_is(book, 3, 32, 16, 0));
	CHECK(arena.regions.top() == 48 && arena.regions.pool_bricks() == 48);
	CHECK(book.pool(2).dev_slot.size() == 42 && book.pool(2).dev_slot[41] == kNoDeviceSlot && book.pool(1).dev_slot.empty());
	CHECK(!book.preloaded() && !book.failed() && book.resident_bricks() == 0 && book.stream_batches() == 0);
	// the words a reset writes, and the other two
	CHECK(PoolBook::device_word(w.sc[0].words[0], kNoDeviceSlot) == (kUnloaded | 0xAB000u));
	CHECK(PoolBook::device_word(0u, kNoDeviceSlot) == 0u && PoolBook::device_word(0u, 5) == 0u);
	CHECK(PoolBook::device_word(7u | kLoaded | 0xAB000u, 9) == (9u | kLoaded | 0xAB000u));
	CHECK(book.absent(0, w.sc[0].words[3]) && !book.absent(0, 0u));

	// ---- (b) cells 0 ... 39 of supercell 2: slots 0 ... 39, the pool 16 -> 32 -> 64, one move
	std::vector<int> ring;
	for (int j = 0; j < 40; ++j) push(ring, 2, j);
	std::vector<Staged> got;
	uint32_t kept = 0;
	CHECK(service(book, arena, w, ring, &kept, &got, false) == 0);
	CHECK(kept == 40 && got.size() == 40);
	bool in_order = true;
	for (uint32_t i = 0; i < got.size(); ++i)
		in_order = in_order && got[i].i == i && got[i].sci == 2 && got[i].host_word == w.sc[2].words[i] && got[i].device_word == (i | kLoaded | 0xAB000u) && book.pool(2).dev_slot[i] == i;
	CHECK(in_order);
	CHECK(pool_is(book, 2, 80, 64, 40)); // 32 bricks at 48, then 64 at 80
	CHECK(book.moves().size() == 1 && is(book.moves()[0], 16, 80, 0, 2)); // from where the batch found it to the last region, what was resident before: nothing
	CHECK(arena.regions.top() == 144 && arena.regions.pool_bricks() == 16 + 64 + 16);
	CHECK(arena.regions.free_regions(4).empty() && arena.regions.free_regions(5).empty()); // the vacated regions: not within the batch
	CHECK(book.resident_bricks() == 40 && book.pool(2).dev_slot[40] == kNoDeviceSlot);
	book.commit_batch();
	CHECK(arena.regions.free_regions(4) == std::vector<uint32_t>{16} && arena.regions.free_regions(5) == std::vector<uint32_t>{48});
	book.batch_streamed(1000);
	CHECK(book.stream_batches() == 1 && book.stream_host_ns() == 1000);

	// ---- the next batches are handed them: 10 bricks of supercell 0, then 10 more -- its pool grows to the vacated 32 at 48 and moves the 10
	ring.clear();
	for (int j = 0; j < 10; ++j) push(ring, 0, j);
	CHECK(service(book, arena, w, ring, &kept) == 0 && kept == 10 && book.moves().empty() && pool_is(book, 0, 0, 16, 10));
	ring.clear();
	for (int j = 10; j < 20; ++j) push(ring, 0, j);
	CHECK(service(book, arena, w, ring, &kept) == 0 && kept == 10);
	CHECK(pool_is(book, 0, 48, 32, 20) && arena.regions.top() == 144);
	CHECK(book.moves().size() == 1 && is(book.moves()[0], 0, 48, 10, 0));
	CHECK(arena.regions.free_regions(5).empty() && arena.regions.free_regions(4) == (std::vector<uint32_t>{16, 0}));
	// a supercell that had no brick at the reset gets one by an edit (not resident: the scene streams), and its first pool by the request: 16 at 0
	CHECK(edit(book, arena, w, 1, {}, {100}) == 0);
	CHECK(book.pool(1).dev_slot.size() == 1 && book.absent(1, w.sc[1].words[100]) && book.moves().empty() && book.resident_bricks() == 60);
	CHECK(PoolBook::device_word(w.sc[1].words[100], book.pool(1).dev_slot[0]) == (kUnloaded | 0x11000u));
	ring.clear();
	push(ring, 1, 100);
	got.clear();
	CHECK(service(book, arena, w, ring, &kept, &got) == 0 && kept == 1 && got[0].device_word == (0u | kLoaded | 0x11000u));
	CHECK(pool_is(book, 1, 0, 16, 1) && book.moves().size() == 1 && is(book.moves()[0], 0, 0, 0, 1)); // count 0: src means nothing
	CHECK(arena.regions.pool_bricks() == 32 + 16 + 64 + 16 && book.resident_bricks() == 61);
}

// (c) stale entries of all three kinds, and the kept count; (e) a freed slot reused by a request, last freed first
void stale_entries_and_freed_slots() {
	Arena arena;
	PoolBook book(&arena.regions);
	World w{12};
	uint32_t kept = 0;
	CHECK(reset(book, arena, w) == 0);
	std::vector<int> ring;
	for (int j = 0; j < 8; ++j) push(ring, 0, j);
	CHECK(service(book, arena, w, ring, &kept) == 0 && kept == 8);
	// cells 3 and 5 are emptied: their device slots are freed, in this order
	CHECK(edit(book, arena, w, 0, {3, 5}, {}) == 0);
	CHECK(book.pool(0).freed == (std::vector<uint32_t>{3, 5}) && book.resident_bricks() == 6 && book.pool(0).resident() == 6 && book.pool(0).high == 8);
	// the ring: 3 (emptied since), 8 (a request), 2 (resident already), 9 twice (a request, then its duplicate), 10 (a request)
	ring.clear();
	for (const int j : {3, 8, 2, 9, 9, 10}) push(ring, 0, j);
	std::vector<Staged> got;
	CHECK(service(book, arena, w, ring, &kept, &got) == 0);
	CHECK(kept == 3 && got.size() == 3);
	CHECK(ring[0] == 8 && ring[3] == 9 && ring[6] == 10); // the kept positions, moved to the front
	// 8 takes slot 5 (last freed first), 9 takes slot 3, 10 the high-water mark
	CHECK(got[0].device_word == (5u | kLoaded | 0xAB000u) && got[1].device_word == (3u | kLoaded | 0xAB000u) && got[2].device_word == (8u | kLoaded | 0xAB000u));
	CHECK(pool_is(book, 0, 0, 16, 9) && book.pool(0).freed.empty() && book.moves().empty() && book.resident_bricks() == 9);
	// a ring of stale entries only: nothing kept, nothing changed
	CHECK(service(book, arena, w, ring, &kept, &got) == 0 && kept == 0 && got.size() == 3 && pool_is(book, 0, 0, 16, 9));
	// a resident brick that an edit rewrites keeps its slot: cell 2 cleared and set again in one batch takes the host slot back, the device slot stays
	const uint16_t before = book.pool(0).dev_slot[w.sc[0].words[2] & BM_BRICK_INDEX_BITS];
	CHECK(edit(book, arena, w, 0, {2}, {2}) == 0);
	CHECK(book.pool(0).dev_slot[w.sc[0].words[2] & BM_BRICK_INDEX_BITS] == before && before == 2 && book.resident_bricks() == 9);
}

// (d) a ring with an entry that cannot be a request: nothing changed, failed set, later calls refused, cleared by a reset
void impossible_entries() {
	for (int kind = 0; kind < 4; ++kind) {
		Arena arena;
		PoolBook book(&arena.regions);
		World w{12, 4};
		uint32_t kept = 99;
		CHECK(reset(book, arena, w) == 0);
		std::vector<int> ring;
		push(ring, 0, 1);
		push(ring, 1, 2);
		if (kind == 0) ring.insert(ring.end(), {32, 0, 0});      // outside the world: x
		if (kind == 1) ring.insert(ring.end(), {3, -1, 0});      // outside the world: below
		if (kind == 2) { w.sc[1].words[7] = 4u | kLoaded; push(ring, 1, 7); } // names host slot 4 of 4
		if (kind == 3) { w.sc[1].words[7] = 2u | kUnloaded; push(ring, 1, 7); } // not a host word
		const std::vector<uint16_t> slots0 = book.pool(0).dev_slot, slots1 = book.pool(1).dev_slot;
		CHECK(service(book, arena, w, ring, &kept) == BM_ESTATE);
		CHECK(book.failed() && kept == 99);
		CHECK(std::strcmp(book.why(), kind < 2 ? "brick request ring holds a position outside the world" : "brick request ring names a brick that does not exist") == 0);
		CHECK(pool_is(book, 0, 0, 16, 0) && pool_is(book, 1, 16, 16, 0) && book.pool(0).dev_slot == slots0 && book.pool(1).dev_slot == slots1 && book.resident_bricks() == 0);
		// refused from here on, with the scene's message
		ring.resize(6);
		CHECK(service(book, arena, w, ring, &kept) == BM_ESTATE && std::strcmp(book.why(), PoolBook::kFailedWhy) == 0 && kept == 99);
		w.sc[1].words[7] = 0;
		CHECK(edit(book, arena, w, 0, {1}, {}) == BM_ESTATE && book.pool(0).freed.empty());
		w.sc[0].set(1, 0xAB); // (the host world as it was)
		CHECK(reset(book, arena, w) == 0 && !book.failed());
		CHECK(service(book, arena, w, ring, &kept) == 0 && kept == 2 && book.why() == nullptr);
	}
}

// (e) a freed slot reused by a preloaded edit; (f) a preloaded edit that needs k appends on an exact-fit pool of 100 bricks
void preloaded_edits() {
	Arena arena;
	PoolBook book(&arena.regions);
	World w{100, 7};
	preload(book, arena, w);
	CHECK(book.preloaded() && book.resident_bricks() == 107 && pool_is(book, 0, 0, 100, 100) && pool_is(book, 1, 100, 7, 7));
	CHECK(arena.regions.top() == 107 && arena.regions.pool_bricks() == 107 && book.pool(0).dev_slot[99] == 99);
	// ---- (e) cells 5 and 9 emptied, then one new brick: it takes host slot 9 and device slot 9, the pool stays
	CHECK(edit(book, arena, w, 0, {5, 9}, {}) == 0);
	CHECK(book.pool(0).freed == (std::vector<uint32_t>{5, 9}) && book.resident_bricks() == 105);
	CHECK(edit(book, arena, w, 0, {}, {200}) == 0);
	CHECK((w.sc[0].words[200] & BM_BRICK_INDEX_BITS) == 9 && book.pool(0).dev_slot[9] == 9 && book.pool(0).freed == std::vector<uint32_t>{5});
	CHECK(pool_is(book, 0, 0, 100, 100) && book.moves().empty() && book.resident_bricks() == 106);
	// ---- (f) 31 new bricks: one takes the freed slot 5, 30 are appended: 130 bricks need 256, the 100 move, the old region is filed under 64
	std::vector<int> cells;
	for (int j = 300; j < 331; ++j) cells.push_back(j);
	CHECK(edit(book, arena, w, 0, {}, cells, false) == 0);
	CHECK(pool_is(book, 0, 107, 256, 130) && book.pool(0).freed.empty() && book.resident_bricks() == 137);
	CHECK(book.moves().size() == 1 && is(book.moves()[0], 0, 107, 100, 0));
	CHECK(arena.regions.top() == 363 && arena.regions.pool_bricks() == 256 + 7);
	CHECK(book.pool(0).dev_slot[w.sc[0].words[300] & BM_BRICK_INDEX_BITS] == 5 && book.pool(0).dev_slot[w.sc[0].words[301] & BM_BRICK_INDEX_BITS] == 100 &&
		  book.pool(0).dev_slot[w.sc[0].words[330] & BM_BRICK_INDEX_BITS] == 129);
	CHECK(arena.regions.free_regions(6).empty());
	book.commit_batch();
	CHECK(arena.regions.free_regions(6) == std::vector<uint32_t>{0});
	for (int cls = 0; cls < 32; ++cls)
		if (cls != 6) CHECK(arena.regions.free_regions(cls).empty());
	// a preload again adopts the host's free slots as the pool's
	w.sc[0].clear(17);
	preload(book, arena, w);
	CHECK(pool_is(book, 0, 0, 130, 130) && book.pool(0).freed == std::vector<uint32_t>{17} && book.resident_bricks() == 136 && book.pool(0).resident() == 129);
}

// (g) the one growth size: max(16, 2c) for one more brick in a full pool of c
void growth_size() {
	CHECK(PoolBook::grown_capacity(0, 1) == 16);
	for (uint32_t c = 16; c <= 4096; c *= 2) CHECK(PoolBook::grown_capacity(c, c + 1) == std::max<uint32_t>(16, 2 * c));
	CHECK(PoolBook::grown_capacity(100, 130) == 256 && PoolBook::grown_capacity(100, 101) == 256 && PoolBook::grown_capacity(7, 8) == 16 && PoolBook::grown_capacity(16, 100) == 128);
}

// (h) the region allocator fails at the first, second and third growth of a batch
void failed_growth() {
	for (int nth = 1; nth <= 3; ++nth) {
		Arena arena;
		PoolBook book(&arena.regions);
		World w{100, 100};
		uint32_t kept = 0;
		CHECK(reset(book, arena, w) == 0);
		std::vector<int> ring;
		for (int j = 0; j < 100; ++j) push(ring, 0, j); // grows at the 17th, 33rd and 65th request
		arena.fail_at = nth;
		CHECK(service(book, arena, w, ring, &kept) == 77);
		CHECK(book.failed() && book.why() == nullptr); // (the allocator has said why)
		CHECK(book.pool(0).high == (nth == 1 ? 16u : nth == 2 ? 32u : 64u) && book.pool(0).high <= book.pool(0).capacity);
		CHECK(service(book, arena, w, ring, &kept) == BM_ESTATE && std::strcmp(book.why(), PoolBook::kFailedWhy) == 0);
		CHECK(edit(book, arena, w, 1, {}, {500}) == BM_ESTATE);
		CHECK(reset(book, arena, w) == 0 && !book.failed() && book.resident_bricks() == 0 && arena.regions.top() == 32);
		ring.clear();
		for (int j = 0; j < 100; ++j) push(ring, 0, j);
		CHECK(service(book, arena, w, ring, &kept) == 0 && kept == 100 && pool_is(book, 0, 128, 128, 100));
		// ... and under a preloaded edit, and at the starting pools of a reset
		preload(book, arena, w);
		arena.fail_at = 1;
		CHECK(edit(book, arena, w, 1, {}, {600, 601}) == 77 && book.failed() && pool_is(book, 1, 100, 101, 101));
		arena.fail_at = 2;
		CHECK(reset(book, arena, w) == 77 && book.failed());
		CHECK(reset(book, arena, w) == 0 && !book.failed());
	}
}

// (i) which ring does what: blocking, overlapped over four calls, and the switches of mode
void ring_state() {
	RegionLists regions;
	PoolBook book(&regions);
	auto step_is = [&](int service, int snapshot) { const PoolBook::QueueStep s = book.queue_step(); return s.service == service && s.snapshot == snapshot; };
	auto change_is = [&](bool to, int drain, bool carry) { const PoolBook::ModeChange m = book.mode_change(to); return m.drain == drain && m.carry == carry; };
	// blocking: ring 0, read and serviced by every call
	CHECK(!book.overlapped() && book.ring() == 0 && step_is(0, -1));
	CHECK(step_is(0, -1) && change_is(false, -1, false) && change_is(true, -1, false));
	// overlapped, four calls
	book.mode_changed(true);
	CHECK(book.overlapped() && book.ring() == 0 && step_is(-1, 0)); // 1: nothing copied out yet; ring 0 is copied out
	book.snapshot_taken();
	CHECK(book.ring() == 1 && step_is(0, 1));                       // 2: ring 0 is serviced, ring 1 copied out
	book.snapshot_read();
	CHECK(step_is(-1, 1));
	book.snapshot_taken();
	CHECK(book.ring() == 0 && step_is(1, 0));                       // 3
	book.snapshot_read();
	book.snapshot_taken();
	CHECK(book.ring() == 1 && step_is(0, 1));                       // 4
	// to blocking with ring 0 copied out and ring 1 current: drain 0, then carry ring 1 over
	CHECK(change_is(false, 0, true) && change_is(true, 0, false));
	book.snapshot_read();
	CHECK(change_is(false, -1, true));
	book.mode_changed(false);
	CHECK(!book.overlapped() && book.ring() == 0 && step_is(0, -1));
	// to blocking with ring 1 copied out and ring 0 current: drain 1, nothing to carry
	book.mode_changed(true);
	book.snapshot_taken();
	book.snapshot_read();
	book.snapshot_taken();
	CHECK(book.ring() == 0 && change_is(false, 1, false));
	book.snapshot_read();
	book.mode_changed(false);
	CHECK(book.ring() == 0 && !book.overlapped());
	// a rebuilt residency: ring 0, nothing pending, the mode stays
	book.mode_changed(true);
	book.snapshot_taken();
	book.begin_rebuild(0);
	book.rebuilt(false);
	CHECK(book.overlapped() && book.ring() == 0 && step_is(-1, 0));
	book.snapshot_taken();
	book.rings_reset();
	CHECK(book.ring() == 0 && step_is(-1, 0));
}

// (j) a few thousand mixed steps from a fixed seed, the invariants after every one
struct Rng {
	uint64_t s = 0x9E3779B97F4A7C15ull;
	uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>(s >> 33); }
	int below(int n) { return static_cast<int>(next() % static_cast<uint32_t>(n)); }
};
bool invariants(const PoolBook& book, const Arena& arena, const World& w) {
	uint64_t capacity = 0, resident = 0;
	std::vector<std::pair<uint32_t, uint32_t>> spans;
	for (size_t i = 0; i < w.sc.size(); ++i) {
		const PoolBook::Pool& p = book.pool(static_cast<int>(i));
		if (p.high > p.capacity || p.dev_slot.size() != w.sc[i].host_slots) return false;
		std::vector<int> seen(p.high, 0);
		for (const uint32_t s : p.freed) { if (s >= p.high || seen[s]++) return false; }
		uint32_t used = 0;
		for (const uint32_t word : w.sc[i].words) {
			if (!word) continue;
			const uint16_t s = p.dev_slot[word & BM_BRICK_INDEX_BITS];
			if (s == kNoDeviceSlot) { if (book.preloaded()) return false; continue; }
			if (s >= p.high || seen[s]++) return false; // unique, below the high-water mark, not a freed one
			used++;
		}
		if (used + p.freed.size() != p.high || used != p.resident()) return false; // freed plus used make [0, high)
		resident += used;
		capacity += p.capacity;
		if (p.capacity) spans.emplace_back(p.base, p.capacity);
	}
	std::sort(spans.begin(), spans.end());
	for (size_t k = 1; k < spans.size(); ++k) if (spans[k - 1].first + spans[k - 1].second > spans[k].first) return false; // pools do not overlap
	if (!spans.empty() && spans.back().first + static_cast<uint64_t>(spans.back().second) > arena.regions.top()) return false;
	return arena.regions.pool_bricks() == capacity && book.resident_bricks() == resident && !book.failed();
}
void random_script() {
	Arena arena;
	PoolBook book(&arena.regions);
	World w{30, 0, 200, 5, 90, 1};
	Rng rng;
	CHECK(reset(book, arena, w) == 0);
	constexpr int kCellsUsed = 700;
	uint64_t serviced = 0, growths = 0;
	for (int step = 0; step < 3000; ++step) {
		const int what = rng.below(100);
		if (what < 2) {
			if (rng.below(2)) preload(book, arena, w);
			else if (reset(book, arena, w)) { CHECK(false); return; }
		} else if (what < 50) { // a ring of up to 40 entries: whatever cells, empty, resident and repeated ones among them
			std::vector<int> ring;
			for (int n = rng.below(41); n > 0; --n) push(ring, rng.below(6), rng.below(kCellsUsed));
			uint32_t kept = 0;
			if (service(book, arena, w, ring, &kept)) { CHECK(false); return; }
			serviced += kept;
			growths += book.moves().size();
		} else { // an edit of one supercell: some cells emptied, some filled
			const int sci = rng.below(6);
			std::vector<int> clear, set;
			for (int n = rng.below(25); n > 0; --n) {
				const int j = rng.below(kCellsUsed);
				if (std::find(clear.begin(), clear.end(), j) != clear.end() || std::find(set.begin(), set.end(), j) != set.end()) continue;
				(w.sc[sci].words[j] ? clear : set).push_back(j);
			}
			if (what >= 90) { // a burst: a preloaded pool has to grow for it
				for (int j = kCellsUsed; j < kCellsUsed + 60; ++j) (w.sc[sci].words[j] ? clear : set).push_back(j);
			}
			if (edit(book, arena, w, sci, clear, set)) { CHECK(false); return; }
			growths += book.moves().size();
		}
		CHECK(invariants(book, arena, w));
	}
	CHECK(serviced > 1000 && growths > 20); // (the script does what it is for)
}

} // namespace

int main() {
	reset_and_forty_requests();
	stale_entries_and_freed_slots();
	impossible_entries();
	preloaded_edits();
	growth_size();
	failed_growth();
	ring_state();
	random_script();
	std::printf("steps %ld\nfailures %ld\n", steps, failures);
	return failures ? 1 : 0;
}
