// read_book_check.cpp -- a program with its own main around csrc/read_book.h (no HIP, no scene), linked with csrc/world.cpp and built plain and
// with -fsanitize=address,undefined by tests/test_read_book.py (-ffp-contract=off, as the library).  It asks the book what the calls that
// only read the world ask it -- the slabs of a box outside the world and where they lie in the caller's volume, what the label calls refuse
// about their box, which bricks of a box the device does not hold and how they are listed, what the two queries refuse, the LoD cell of an
// origin, the label clock -- and compares with answers computed here by brute force.  prints "steps N" and "failures N".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../brickmap_amd/csrc/read_book.h"

namespace {

using namespace bm;

long failures = 0, steps = 0;
#define CHECK(cond)                                                                  \
	do {                                                                             \
		++steps;                                                                     \
		if (!(cond)) {                                                               \
			if (++failures <= 20) std::printf("line %d: %s\n", __LINE__, #cond);     \
		}                                                                            \
	} while (0)

struct Rng {
	uint64_t s = 0x9E3779B97F4A7C15ull;
	uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>(s >> 33); }
	int below(int n) { return static_cast<int>(next() % static_cast<uint32_t>(n)); }
	int between(int a, int b) { return a + below(b - a + 1); }
};

struct Box {
	int64_t x0, x1, y0, y1, z0, z1;
	int64_t volume() const { return (x1 - x0) * (y1 - y0) * (z1 - z0); }
	bool empty() const { return x1 <= x0 || y1 <= y0 || z1 <= z0; }
	bool meets(const Box& o) const { return !empty() && !o.empty() && x0 < o.x1 && o.x0 < x1 && y0 < o.y1 && o.y0 < y1 && z0 < o.z1 && o.z0 < z1; }
	bool within(const Box& o) const { return x0 >= o.x0 && x1 <= o.x1 && y0 >= o.y0 && y1 <= o.y1 && z0 >= o.z0 && z1 <= o.z1; }
};

// ---------------------------------------------------------------- (a) outside slabs and offsets
// the slabs and the clipped box tile the box exactly once: by volumes and pairwise, and voxel by voxel where the box is small
void slabs_tile(const WorldDims& d, int x0, int y0, int z0, int x1, int y1, int z1, int want_slabs) {
	const int32_t blo[3] = {x0, y0, z0}, bhi[3] = {x1, y1, z1};
	bm_region r{};
	for (int k = 0; k < 3; ++k) { r.lo[k] = blo[k]; r.hi[k] = bhi[k]; }
	int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
	const bool inside = World::region_bounds(d, r, lo, hi);
	const Box box{x0, x1, y0, y1, z0, z1};
	const int dims[3] = {d.grid_size, d.grid_size, d.grid_height};
	Box clip{std::max(x0, 0), std::min(x1, dims[0]), std::max(y0, 0), std::min(y1, dims[1]), std::max(z0, 0), std::min(z1, dims[2])}; // by hand
	CHECK(inside == !clip.empty());
	if (inside) CHECK(lo[0] == clip.x0 && hi[0] == clip.x1 && lo[1] == clip.y0 && hi[1] == clip.y1 && lo[2] == clip.z0 && hi[2] == clip.z1);
	else clip = Box{0, 0, 0, 0, 0, 0};
	std::vector<Box> slabs;
	outside_slabs(blo, bhi, inside, lo, hi, [&](int64_t a0, int64_t a1, int64_t b0, int64_t b1, int64_t c0, int64_t c1) { slabs.push_back(Box{a0, a1, b0, b1, c0, c1}); });
	if (box.empty()) { // (the calls launch nothing for an empty box; the one slab of a box that is not inside is the box itself)
		CHECK(!inside && slabs.size() == 1 && slabs[0].volume() == 0);
		return;
	}
	CHECK(want_slabs < 0 || static_cast<int>(slabs.size()) == want_slabs);
	int64_t sum = clip.volume();
	bool ok = slabs.size() <= 6;
	for (size_t i = 0; i < slabs.size(); ++i) {
		ok = ok && !slabs[i].empty() && slabs[i].within(box) && !slabs[i].meets(clip);
		for (size_t j = 0; j < i; ++j) ok = ok && !slabs[i].meets(slabs[j]);
		sum += slabs[i].volume();
	}
	CHECK(ok && sum == box.volume());
	if (box.volume() > 64000) return;
	const int64_t nx = x1 - x0, ny = y1 - y0;
	std::vector<uint8_t> seen(static_cast<size_t>(box.volume()), 0);
	auto count = [&](const Box& b) {
		for (int64_t z = b.z0; z < b.z1; ++z)
			for (int64_t y = b.y0; y < b.y1; ++y)
				for (int64_t x = b.x0; x < b.x1; ++x) seen[static_cast<size_t>(((z - z0) * ny + (y - y0)) * nx + (x - x0))]++;
	};
	for (const Box& s : slabs) count(s);
	bool outside_world = true;
	for (int64_t z = z0; z < z1; ++z)
		for (int64_t y = y0; y < y1; ++y)
			for (int64_t x = x0; x < x1; ++x) {
				const bool in_world = x >= 0 && y >= 0 && z >= 0 && x < dims[0] && y < dims[1] && z < dims[2];
				outside_world = outside_world && seen[static_cast<size_t>(((z - z0) * ny + (y - y0)) * nx + (x - x0))] == (in_world ? 0 : 1);
			}
	CHECK(outside_world); // every voxel outside the world in exactly one slab, none inside it in any
	count(clip);
	bool once = true;
	for (const uint8_t c : seen) once = once && c == 1;
	CHECK(once);
}

void slabs() {
	WorldDims cube, flat;
	CHECK(cube.set(128, 128) && flat.set(256, 128));
	for (const WorldDims* d : {&cube, &flat}) {
		const int X = d->grid_size, Z = d->grid_height;
		slabs_tile(*d, 10, 20, 30, 40, 50, 60, 0);                  // inside the world
		slabs_tile(*d, 0, 0, 0, 8, 8, 8, 0);
		slabs_tile(*d, X - 8, X - 8, Z - 8, X, X, Z, 0);
		slabs_tile(*d, -5, 20, 30, 25, 50, 60, 1);                  // straddling each of the six faces
		slabs_tile(*d, X - 20, 20, 30, X + 7, 50, 60, 1);
		slabs_tile(*d, 10, -9, 30, 40, 21, 60, 1);
		slabs_tile(*d, 10, X - 1, 30, 40, X + 1, 60, 1);
		slabs_tile(*d, 10, 20, -30, 40, 50, 9, 1);
		slabs_tile(*d, 10, 20, Z - 3, 40, 50, Z + 30, 1);
		slabs_tile(*d, -5, -6, 30, 25, 24, 60, 2);                  // an edge
		slabs_tile(*d, X - 10, 20, Z - 10, X + 10, 50, Z + 10, 2);
		slabs_tile(*d, -5, -6, -7, 25, 24, 23, 3);                  // a corner
		slabs_tile(*d, X - 30, X - 20, Z - 10, X + 9, X + 19, Z + 29, 3);
		slabs_tile(*d, -1, -2, -3, X + 3, X + 2, Z + 1, 6);         // containing the world
		slabs_tile(*d, -1, 0, 0, X, X, Z, 1);
		slabs_tile(*d, X, 0, 0, X + 30, 30, 30, 1);                 // wholly outside: beside it, touching
		slabs_tile(*d, -40, -40, -40, -1, -1, -1, 1);
		slabs_tile(*d, 10, 20, Z + 100, 40, 50, Z + 130, 1);
		slabs_tile(*d, 10, 20, 30, 10, 50, 60, -1);                 // empty
		slabs_tile(*d, -10, -20, -30, 40, -20, 60, -1);
		slabs_tile(*d, 5, 5, 5, 5, 5, 5, -1);
	}
	Rng rng;
	for (int i = 0; i < 300; ++i) {
		const WorldDims& d = i & 1 ? flat : cube;
		const int x = rng.between(-30, d.grid_size + 10), y = rng.between(-30, d.grid_size + 10), z = rng.between(-30, d.grid_height + 10);
		slabs_tile(d, x, y, z, x + rng.between(0, 40), y + rng.between(0, 40), z + rng.between(0, 40), -1);
	}
}

void offsets() {
	// a region with pitches: the offset of every voxel against a walk of the volume, row by row and slice by slice
	bm_region r{};
	r.lo[0] = -7; r.lo[1] = 120; r.lo[2] = 3; r.hi[0] = 6; r.hi[1] = 131; r.hi[2] = 8;
	for (const int64_t row : {int64_t{13}, int64_t{16}, int64_t{100}})
		for (const int64_t slice : {row * 11, row * 11 + 5, row * 40}) {
			r.row_pitch = row; r.slice_pitch = slice;
			bool ok = true;
			int64_t at_z = 0;
			for (int z = r.lo[2]; z < r.hi[2]; ++z, at_z += slice) {
				int64_t at_y = at_z;
				for (int y = r.lo[1]; y < r.hi[1]; ++y, at_y += row) {
					int64_t at = at_y;
					for (int x = r.lo[0]; x < r.hi[0]; ++x, ++at) ok = ok && region_offset(r, x, y, z) == at;
				}
			}
			CHECK(ok);
		}
	// the label volume of a box: tight, four bytes a voxel, the voxel's word where label.h's index says
	const int32_t lo[3] = {-7, 120, 3}, hi[3] = {6, 131, 8};
	LabelDims d;
	bool empty = true;
	CHECK(check_label_box(lo, hi, 2, &d, &empty) == nullptr && !empty);
	const LabelPitch pitch(d);
	CHECK(pitch.row == 13 * 4 && pitch.slice == 13 * 11 * 4);
	std::vector<int32_t> volume(13 * 11 * 5);
	bool ok = true;
	for (int z = lo[2]; z < hi[2]; ++z)
		for (int y = lo[1]; y < hi[1]; ++y)
			for (int x = lo[0]; x < hi[0]; ++x) {
				const int32_t* word = &volume[label_index(static_cast<uint32_t>(x - lo[0]), static_cast<uint32_t>(y - lo[1]), static_cast<uint32_t>(z - lo[2]), d.nx, d.ny)];
				ok = ok && pitch.offset(d, x, y, z) == reinterpret_cast<const char*>(word) - reinterpret_cast<const char*>(volume.data());
			}
	CHECK(ok && pitch.offset(d, hi[0] - 1, hi[1] - 1, hi[2] - 1) + 4 == static_cast<int64_t>(volume.size() * sizeof(int32_t)));
}

// ---------------------------------------------------------------- (b) the label box
const char* const kNull = "null box";
const char* const kOrder = "hi < lo";
const char* const kTooMany = "the box holds more than 2^31 - 2 voxels";

void label_box_is(int32_t x0, int32_t y0, int32_t z0, int32_t x1, int32_t y1, int32_t z1, const char* want) {
	const int32_t lo[3] = {x0, y0, z0}, hi[3] = {x1, y1, z1};
	LabelDims d;
	std::memset(&d, 0x5A, sizeof d);
	bool empty = false;
	const char* why = check_label_box(lo, hi, 3, &d, &empty);
	// by 128-bit arithmetic
	const __int128 n[3] = {static_cast<__int128>(x1) - x0, static_cast<__int128>(y1) - y0, static_cast<__int128>(z1) - z0};
	const char* expect = n[0] < 0 || n[1] < 0 || n[2] < 0 ? kOrder : n[0] * n[1] * n[2] > ((static_cast<__int128>(1) << 31) - 2) ? kTooMany : nullptr;
	CHECK(expect == want || (expect && want && std::strcmp(expect, want) == 0));
	CHECK(why == want || (why && want && std::strcmp(why, want) == 0));
	if (why) return;
	CHECK(empty == (n[0] * n[1] * n[2] == 0));
	CHECK(d.org[0] == x0 && d.org[1] == y0 && d.org[2] == z0 && d.nx == static_cast<uint32_t>(n[0]) && d.ny == static_cast<uint32_t>(n[1]) && d.nz == static_cast<uint32_t>(n[2]) &&
		  d.sg_xy == 3 && d.sg_xy2 == 9);
}

void label_boxes() {
	const int32_t lo[3] = {0, 0, 0}, hi[3] = {8, 8, 8};
	LabelDims d;
	bool empty = false;
	CHECK(check_label_box(nullptr, hi, 1, &d, &empty) == std::string(kNull) && check_label_box(lo, nullptr, 1, &d, &empty) == std::string(kNull));
	CHECK(check_label_box(nullptr, nullptr, 1, &d, &empty) == std::string(kNull));
	const int32_t lowest = std::numeric_limits<int32_t>::min(), highest = std::numeric_limits<int32_t>::max();
	label_box_is(0, 0, 0, 8, 8, 8, nullptr);
	label_box_is(-3, -4, -5, 100, 200, 300, nullptr);
	label_box_is(1, 0, 0, 0, 8, 8, kOrder);
	label_box_is(0, 9, 0, 8, 8, 8, kOrder);
	label_box_is(0, 0, lowest + 1, 8, 8, lowest, kOrder);
	label_box_is(highest, 0, 0, lowest, 8, 8, kOrder);   // hi - lo would wrap in 32 bits
	label_box_is(0, 0, 0, lowest, highest, highest, kOrder); // (hi < lo wins over the count)
	// emptiness: an axis of no voxels, whatever the others span
	label_box_is(5, 0, 0, 5, 8, 8, nullptr);
	label_box_is(0, 0, 7, 8, 8, 7, nullptr);
	label_box_is(5, lowest, lowest, 5, highest, highest, nullptr);
	label_box_is(lowest, lowest, 0, highest, highest, 0, nullptr);
	label_box_is(lowest, 3, lowest, highest, 3, highest, nullptr);
	// the limit: 2^31 - 2 voxels pass, one more does not -- along one axis, as a product of two, of three
	label_box_is(0, 0, 0, highest - 1, 1, 1, nullptr);
	label_box_is(0, 0, 0, highest, 1, 1, kTooMany);
	label_box_is(0, 0, 0, 1, highest - 1, 1, nullptr);
	label_box_is(0, 0, 0, 1, 1, highest, kTooMany);
	label_box_is(-1, 0, 0, highest - 2, 1, 1, nullptr);
	label_box_is(-1, 0, 0, highest - 1, 1, 1, kTooMany);
	label_box_is(0, 0, 0, 65536, 32767, 1, nullptr);
	label_box_is(0, 0, 0, 65536, 32768, 1, kTooMany);
	label_box_is(0, 0, 0, 46340, 1, 46340, nullptr);     // 46340^2 = 2^31 - 88 047
	label_box_is(0, 0, 0, 46341, 1, 46341, kTooMany);
	label_box_is(0, 0, 0, 2, 1073741823, 1, nullptr);    // 2 x (2^30 - 1) = 2^31 - 2
	label_box_is(0, 0, 0, 2, 1073741824, 1, kTooMany);
	label_box_is(7, 7, 7, 1297, 1297, 1297, nullptr);    // 1290^3 = 2 146 689 000
	label_box_is(7, 7, 7, 1298, 1298, 1298, kTooMany);
	label_box_is(0, 0, 0, 2048, 1024, 1023, nullptr);
	label_box_is(0, 0, 0, 2048, 1024, 1024, kTooMany);
	// overflow: edges of up to 2^32 - 1 on one, two and three axes (the products are formed in 64 bits, each only once the one before has passed)
	label_box_is(lowest, 0, 0, highest, 1, 1, kTooMany);
	label_box_is(0, lowest, 0, 1, highest, 1, kTooMany);
	label_box_is(0, 0, lowest, 1, 1, highest, kTooMany);
	label_box_is(lowest, lowest, 0, highest, highest, 1, kTooMany);
	label_box_is(lowest, 0, lowest, highest, 1, highest, kTooMany);
	label_box_is(0, lowest, lowest, 1, highest, highest, kTooMany);
	label_box_is(lowest, lowest, lowest, highest, highest, highest, kTooMany);
	label_box_is(0, lowest, lowest, highest - 1, highest, highest, kTooMany); // the first factor passes alone, the product of two does not
	label_box_is(0, 0, lowest, 46340, 46340, highest, kTooMany);              // the product of two passes, of three does not
	label_box_is(-1, -1, -1, highest, highest, highest, kTooMany);            // 2^31 on every axis
	label_box_is(0, 0, 0, 65536, 65536, 65536, kTooMany);                     // 2^48

	// label_clip: the box clipped by hand, and the cells counted one by one
	WorldDims cube, flat;
	CHECK(cube.set(128, 128) && flat.set(256, 128));
	Rng rng;
	for (int i = 0; i < 200; ++i) {
		const WorldDims& w = i & 1 ? flat : cube;
		const int dims[3] = {w.grid_size, w.grid_size, w.grid_height};
		int32_t blo[3], bhi[3];
		for (int k = 0; k < 3; ++k) {
			blo[k] = rng.between(-40, dims[k] + 20);
			bhi[k] = blo[k] + (i % 7 == 0 && k == i % 3 ? 0 : rng.between(1, i < 20 ? 400 : 60));
		}
		LabelDims ld{};
		bool none = false;
		CHECK(check_label_box(blo, bhi, w.supergrid_xy, &ld, &none) == nullptr);
		const bool inside = label_clip(w, blo, bhi, &ld);
		bool want_inside = true;
		int clo[3], chi[3];
		for (int k = 0; k < 3; ++k) {
			clo[k] = std::max<int>(blo[k], 0);
			chi[k] = std::min<int>(bhi[k], dims[k]);
			want_inside = want_inside && clo[k] < chi[k];
		}
		bm_region r{};
		for (int k = 0; k < 3; ++k) { r.lo[k] = blo[k]; r.hi[k] = bhi[k]; }
		int rlo[3] = {0, 0, 0}, rhi[3] = {0, 0, 0};
		CHECK(inside == want_inside && inside == World::region_bounds(w, r, rlo, rhi));
		bool ok = true;
		for (int k = 0; k < 3; ++k) {
			if (!inside) { ok = ok && ld.lo[k] == 0 && ld.hi[k] == 0 && ld.c0[k] == 0 && ld.nc[k] == 0; continue; }
			int first = -1, cells = 0;
			for (int c = 0; c < dims[k] / 8; ++c)
				if (8 * c < chi[k] && 8 * c + 8 > clo[k]) { if (first < 0) first = c; ++cells; }
			ok = ok && ld.lo[k] == clo[k] && ld.hi[k] == chi[k] && ld.lo[k] == rlo[k] && ld.hi[k] == rhi[k] && ld.c0[k] == first && ld.nc[k] == cells;
		}
		CHECK(ok && ld.org[0] == blo[0] && ld.nz == static_cast<uint32_t>(bhi[2] - blo[2]) && ld.sg_xy == static_cast<uint32_t>(w.supergrid_xy)); // (what the box check filled in stays)
	}
}

// ---------------------------------------------------------------- (c) the patch list
struct Arena { // as in pool_book_check.cpp
	RegionLists regions;
	int alloc(uint32_t bricks, uint32_t* offset) {
		if (!regions.take_free(bricks, offset)) *offset = regions.claim_top(bricks);
		return 0;
	}
	auto fn() { return [this](uint32_t bricks, uint32_t* offset) { return alloc(bricks, offset); }; }
};

// a host world with its book (as in change_book_check.cpp)
struct Rig {
	World world;
	Arena arena;
	PoolBook book{&arena.regions};

	Rig(const std::vector<uint8_t>& volume, bool preloaded) {
		world.dims.set(128, 128);
		world.load_voxels(volume.data(), 2);
		const int n = world.dims.supercells;
		arena.regions.reset();
		book.begin_rebuild(n);
		for (int i = 0; i < n; ++i) {
			const HostSupercell& c = world.supercells[i];
			if (preloaded) book.adopt_exact(i, arena.regions.claim_top(c.bricks.size()), c.bricks.size(), c.free_slots);
			else CHECK(book.start_pool(i, c.bricks.size(), arena.fn()) == 0);
		}
		book.rebuilt(preloaded);
	}
	Rig(const Rig&) = delete;
	// a streaming scene's requests, serviced: the bricks become resident
	void request(std::vector<int> pos) {
		const WorldDims& d = world.dims;
		auto lookup = [&](int px, int py, int pz, int* sci, uint32_t* word, size_t* host_slots) {
			if (px < 0 || py < 0 || pz < 0 || px >= d.cells || py >= d.cells || pz >= d.cells_height) return false;
			*sci = d.supercell_id(px / kSupercell, py / kSupercell, pz / kSupercell);
			*word = world.supercells[*sci].indices[cell_local_index(px, py, pz)];
			*host_slots = world.supercells[*sci].bricks.size();
			return true;
		};
		const uint32_t count = static_cast<uint32_t>(pos.size() / 3);
		CHECK(book.check_ring(pos.data(), count, lookup) == 0);
		book.begin_batch();
		uint32_t kept = 0;
		CHECK(book.ring_slots(pos.data(), count, lookup, arena.fn(), [](uint32_t, int, uint32_t, uint32_t) {}, &kept) == 0);
		book.commit_batch();
	}
	// the list of the box against a scan of every cell of the world; returns the number of bricks listed
	size_t list_is_scan(int x0, int y0, int z0, int x1, int y1, int z1) {
		bm_region r{};
		r.lo[0] = x0; r.lo[1] = y0; r.lo[2] = z0; r.hi[0] = x1; r.hi[1] = y1; r.hi[2] = z1;
		int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
		const bool inside = World::region_bounds(world.dims, r, lo, hi);
		const PatchList list(world, book, inside, lo, hi);
		std::vector<int> cells;
		std::vector<Brick> bricks;
		for (int cz = 0; cz < 16; ++cz)
			for (int cy = 0; cy < 16; ++cy)
				for (int cx = 0; cx < 16; ++cx) {
					if (8 * cx >= x1 || 8 * cx + 8 <= x0 || 8 * cy >= y1 || 8 * cy + 8 <= y0 || 8 * cz >= z1 || 8 * cz + 8 <= z0 || x1 <= x0 || y1 <= y0 || z1 <= z0) continue; // no voxel of the box
					const HostSupercell& c = world.supercells[0];
					const uint32_t word = c.indices[static_cast<size_t>(cx + 16 * cy + 256 * cz)];
					if (word == 0) continue;                                          // no brick
					if (book.pool(0).dev_slot[word & 0xFFFu] != 0xFFFFu) continue;    // the device holds it
					cells.push_back(cx); cells.push_back(cy); cells.push_back(cz);
					bricks.push_back(c.bricks[word & 0xFFFu]);
				}
		CHECK(list.cells == cells && list.bricks.size() == bricks.size() && list.layout().n == bricks.size());
		CHECK(bricks.empty() || std::memcmp(list.bricks.data(), bricks.data(), bricks.size() * sizeof(Brick)) == 0);
		return bricks.size();
	}
};

// four solid layers of cells (1024 bricks, each with a voxel or two out of it, so that bricks next to each other in a list differ), a tower and one full brick in the air
std::vector<uint8_t> hand_made() {
	const int n = 128;
	std::vector<uint8_t> v(static_cast<size_t>(n) * n * n, 0);
	auto fill = [&](int x0, int y0, int z0, int x1, int y1, int z1, uint8_t to) {
		for (int z = z0; z < z1; ++z)
			for (int y = y0; y < y1; ++y)
				for (int x = x0; x < x1; ++x) v[(static_cast<size_t>(z) * n + y) * n + x] = to;
	};
	fill(0, 0, 0, n, n, 32, 1);
	for (int c = 0; c < 1024; ++c) { // cell c of the layers loses voxels (c % 8, (c / 8) % 8, (c / 64) % 8) and, for c >= 512, its last one
		const int cx = c % 16, cy = (c / 16) % 16, cz = c / 256;
		fill(8 * cx + c % 8, 8 * cy + (c / 8) % 8, 8 * cz + (c / 64) % 8, 8 * cx + c % 8 + 1, 8 * cy + (c / 8) % 8 + 1, 8 * cz + (c / 64) % 8 + 1, 0);
		if (c >= 512) fill(8 * cx + 7, 8 * cy + 7, 8 * cz + 7, 8 * cx + 8, 8 * cy + 8, 8 * cz + 8, 0);
	}
	fill(60, 60, 32, 70, 70, 90, 1);
	fill(96, 16, 96, 104, 24, 104, 1);
	return v;
}

void patch_lists() {
	const std::vector<uint8_t> volume = hand_made();
	{ // a preloaded scene holds every brick
		Rig rig(volume, true);
		CHECK(rig.list_is_scan(0, 0, 0, 128, 128, 128) == 0 && rig.list_is_scan(3, 3, 3, 70, 70, 70) == 0);
	}
	Rig rig(volume, false);
	const size_t towers = 2 * 2 * 8, air = 1; // cells 7 ... 8 of x and y, 4 ... 11 of z; one full brick
	CHECK(rig.world.total_bricks() == 1024 + towers + air);
	CHECK(rig.list_is_scan(0, 0, 0, 128, 128, 128) == 1024 + towers + air); // nothing resident
	CHECK(rig.list_is_scan(0, 0, 0, 8, 8, 8) == 1);
	CHECK(rig.list_is_scan(0, 0, 0, 128, 128, 32) == 1024);
	CHECK(rig.list_is_scan(7, 7, 7, 9, 9, 9) == 8);                 // one voxel of eight cells each
	CHECK(rig.list_is_scan(8, 8, 8, 16, 16, 16) == 1);
	CHECK(rig.list_is_scan(0, 0, 32, 128, 128, 128) == towers + air);
	CHECK(rig.list_is_scan(0, 0, 96, 50, 50, 128) == 0);           // air
	CHECK(rig.list_is_scan(-20, -20, -20, 12, 12, 12) == 8);       // clipped by the world
	CHECK(rig.list_is_scan(200, 0, 0, 300, 10, 10) == 0);          // outside: nothing is read
	CHECK(rig.list_is_scan(5, 5, 5, 5, 60, 60) == 0);              // empty
	std::vector<int> pos; // some bricks resident: a row of the floor, the lower half of the tower, the piece in the air
	for (int cx = 2; cx < 10; ++cx) pos.insert(pos.end(), {cx, 5, 0});
	for (int cz = 4; cz < 8; ++cz) pos.insert(pos.end(), {7, 7, cz, 8, 8, cz});
	pos.insert(pos.end(), {12, 2, 12});
	rig.request(pos);
	CHECK(rig.book.resident_bricks() == 17);
	CHECK(rig.list_is_scan(0, 0, 0, 128, 128, 128) == 1024 + towers + air - 17);
	CHECK(rig.list_is_scan(0, 40, 0, 128, 48, 8) == 8);            // the row of cells y = 5, z = 0: eight of sixteen left
	CHECK(rig.list_is_scan(16, 40, 0, 80, 48, 8) == 0);
	CHECK(rig.list_is_scan(56, 56, 32, 72, 72, 96) == towers - 8);
	CHECK(rig.list_is_scan(96, 16, 96, 112, 32, 112) == 0);
	Rng rng;
	size_t listed = 0;
	for (int i = 0; i < 40; ++i) {
		const int x = rng.between(-20, 120), y = rng.between(-20, 120), z = rng.between(-20, 100);
		listed += rig.list_is_scan(x, y, z, x + rng.between(0, 90), y + rng.between(0, 90), z + rng.between(0, 60));
	}
	CHECK(listed > 1000);

	// the layout: [cells: 3 ints each][bricks], the bricks on a 64-byte line, no line wasted
	for (const size_t n : {0u, 1u, 5u, 6u, 860u, 861u, 862u, 863u, 1024u}) {
		const PatchList::Layout at(n);
		CHECK(at.n == n && at.o_bricks % 64 == 0 && at.o_bricks >= 12 * n && at.o_bricks < 12 * n + 64 && at.bytes == at.o_bricks + 64 * n);
		CHECK((at.bytes <= kScratchStart) == (n <= 862)); // what the list starts with holds it
		CHECK(scratch_grown(at.bytes) == (n <= 862 ? size_t{65536} : at.bytes));
	}
	CHECK(PatchList::Layout(0).bytes == 0 && PatchList::Layout(1).o_bricks == 64 && PatchList::Layout(1).bytes == 128);
	CHECK(PatchList::Layout(5).o_bricks == 64 && PatchList::Layout(5).bytes == 384 && PatchList::Layout(6).o_bricks == 128 && PatchList::Layout(6).bytes == 512); // 60 bytes of cells fit a line, 72 do not
	CHECK(PatchList::Layout(860).bytes == 65408 && PatchList::Layout(861).bytes == 65472 && PatchList::Layout(862).bytes == 65536 && PatchList::Layout(863).bytes == 65600);
	CHECK(PatchList::Layout(1024).o_bricks == 12288 && PatchList::Layout(1024).bytes == 77824);
	CHECK(kScratchStart == 65536 && scratch_grown(0) == 65536 && scratch_grown(1) == 65536 && scratch_grown(65537) == 65537 && scratch_grown(72296) == 72296);

	// fill, out of a poisoned buffer: both sections where the layout says, nothing else written
	for (const int layers : {0, 1, 4}) {
		Rig fresh(volume, false);
		int lo[3] = {0, 0, 0}, hi[3] = {layers == 1 ? 40 : 128, layers == 1 ? 8 : 128, 8 * std::max(layers, 1)};
		const PatchList list(fresh.world, fresh.book, layers > 0, lo, hi);
		const PatchList::Layout at = list.layout();
		CHECK(at.n == (layers == 0 ? 0u : layers == 1 ? 5u : 1024u));
		std::vector<char> buf(at.bytes + 64, static_cast<char>(0xA5));
		list.fill(buf.data());
		bool back = at.n == 0 || (std::memcmp(buf.data(), list.cells.data(), 12 * at.n) == 0 && std::memcmp(buf.data() + at.o_bricks, list.bricks.data(), 64 * at.n) == 0);
		bool poison = true;
		for (size_t i = 0; i < buf.size(); ++i)
			if (!(i < 12 * at.n || (i >= at.o_bricks && i < at.bytes))) poison = poison && buf[i] == static_cast<char>(0xA5);
		CHECK(back && poison);
		for (size_t i = 1; i < at.n; ++i) back = back && std::memcmp(&list.bricks[i], &list.bricks[i - 1], sizeof(Brick)) != 0; // (neighbours differ: an order mistake shows)
		CHECK(back);
	}
}

// ---------------------------------------------------------------- (d) query arguments
bool says(const char* got, const char* want) { return want ? got && std::strcmp(got, want) == 0 : got == nullptr; }

void queries() {
	const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
	char rays[64] = {}, hits[64] = {};
	float origin[3] = {10.f, 20.f, 30.f};
	int campos[3] = {-1, -1, -1};
	bool nothing = true;
	// cast_rays, in the order of the refusals: flags, n, (n == 0), nulls, lod_origin
	CHECK(says(check_cast_rays(1, rays, hits, 4u, origin, campos, &nothing), "bm_scene_cast_rays: unknown flag") && !nothing);
	CHECK(says(check_cast_rays(-1, nullptr, nullptr, 0x80000000u, nullptr, campos, &nothing), "bm_scene_cast_rays: unknown flag"));
	CHECK(says(check_cast_rays(-1, rays, hits, 0, nullptr, campos, &nothing), "bm_scene_cast_rays: n must be 0 ... 2^28"));
	CHECK(says(check_cast_rays((int64_t{1} << 28) + 1, nullptr, nullptr, BM_QUERY_LOD, nullptr, campos, &nothing), "bm_scene_cast_rays: n must be 0 ... 2^28") && !nothing);
	CHECK(says(check_cast_rays(0, nullptr, nullptr, BM_QUERY_LOD, nullptr, campos, &nothing), nullptr) && nothing); // nothing to do: the rest is not looked at
	CHECK(says(check_cast_rays(1, nullptr, hits, BM_QUERY_LOD, nullptr, campos, &nothing), "bm_scene_cast_rays: null ray or hit buffer") && !nothing);
	CHECK(says(check_cast_rays(1, rays, nullptr, 0, nullptr, campos, &nothing), "bm_scene_cast_rays: null ray or hit buffer"));
	CHECK(says(check_cast_rays(1, rays, hits, BM_QUERY_LOD, nullptr, campos, &nothing), "bm_scene_cast_rays: BM_QUERY_LOD needs lod_origin"));
	CHECK(says(check_cast_rays(int64_t{1} << 28, rays, hits, BM_QUERY_NO_REQUESTS, nullptr, campos, &nothing), nullptr) && !nothing && campos[0] == 0 && campos[1] == 0 && campos[2] == 0);
	campos[0] = campos[1] = campos[2] = -1;
	CHECK(says(check_cast_rays(5, rays, hits, 0, origin, campos, &nothing), nullptr) && campos[0] == 0 && campos[1] == 0 && campos[2] == 0); // without BM_QUERY_LOD the origin is not read
	CHECK(says(check_cast_rays(5, rays, hits, BM_QUERY_LOD | BM_QUERY_NO_REQUESTS, origin, campos, &nothing), nullptr) && campos[0] == 1 && campos[1] == 2 && campos[2] == 3);
	for (int axis = 0; axis < 3; ++axis)
		for (const float bad : {16777216.f, -16777216.f, 3e38f, nan, inf, -inf}) {
			float o[3] = {1.f, 2.f, 3.f};
			o[axis] = bad;
			CHECK(says(check_cast_rays(5, rays, hits, BM_QUERY_LOD, o, campos, &nothing), "bm_scene_cast_rays: lod_origin must be finite and below 2^24"));
			CHECK(!lod_origin_ok(bad));
		}
	// the LoD cell: the origin over 8, towards zero
	const struct { float v; int cell; } cells[] = {
		{0.f, 0}, {-0.f, 0}, {7.999f, 0}, {8.f, 1}, {-1.f, 0}, {-7.5f, 0}, {-8.f, -1}, {-9.f, -1}, {-16.f, -2}, {1023.9f, 127}, {1e-30f, 0},
		{16777215.f, 2097151}, {-16777215.f, -2097151}, {16777208.f, 2097151}, {16777207.f, 2097150}, {-16777208.f, -2097151},
	};
	for (const auto& c : cells) CHECK(lod_origin_ok(c.v) && lod_cell(c.v) == c.cell && lod_cell(c.v) == static_cast<int>(std::trunc(static_cast<double>(c.v) / 8.0)));
	Rng rng;
	bool ok = true;
	for (int i = 0; i < 2000; ++i) {
		uint32_t bits = rng.next() << 1 ^ rng.next();
		float v;
		std::memcpy(&v, &bits, sizeof v);
		const bool fits = std::isfinite(v) && std::fabs(static_cast<double>(v)) < 16777216.0;
		ok = ok && lod_origin_ok(v) == fits && (!fits || lod_cell(v) == static_cast<int>(std::trunc(static_cast<double>(v) / 8.0)));
	}
	CHECK(ok);
	float o[3] = {-16777215.f, 16777215.f, -8.f};
	CHECK(says(check_cast_rays(1, rays, hits, BM_QUERY_LOD, o, campos, &nothing), nullptr) && campos[0] == -2097151 && campos[1] == 2097151 && campos[2] == -1);

	// query_volumes: flags, n, (n == 0), nulls, alignment
	alignas(8) char volumes[64] = {}, results[64] = {};
	CHECK(says(check_query_volumes(-1, nullptr, nullptr, 2u, &nothing), "bm_scene_query_volumes: unknown flag") && !nothing);
	CHECK(says(check_query_volumes(-1, nullptr, nullptr, BM_VOLUME_ANY, &nothing), "bm_scene_query_volumes: n must be 0 ... 2^24"));
	CHECK(says(check_query_volumes((int64_t{1} << 24) + 1, volumes, results, 0, &nothing), "bm_scene_query_volumes: n must be 0 ... 2^24") && !nothing);
	CHECK(says(check_query_volumes(0, nullptr, volumes + 1, BM_VOLUME_ANY, &nothing), nullptr) && nothing);
	CHECK(says(check_query_volumes(1, nullptr, results + 1, 0, &nothing), "bm_scene_query_volumes: null volume or result buffer") && !nothing);
	CHECK(says(check_query_volumes(1, volumes, nullptr, 0, &nothing), "bm_scene_query_volumes: null volume or result buffer"));
	CHECK(says(check_query_volumes(1, volumes + 2, results, 0, &nothing), "bm_scene_query_volumes: volumes must be 4-byte aligned, results 8-byte aligned"));
	CHECK(says(check_query_volumes(1, volumes, results + 4, 0, &nothing), "bm_scene_query_volumes: volumes must be 4-byte aligned, results 8-byte aligned"));
	CHECK(says(check_query_volumes(int64_t{1} << 24, volumes + 4, results + 8, BM_VOLUME_ANY, &nothing), nullptr) && !nothing);
}

// ---------------------------------------------------------------- (e) the label clock
void label_clock() {
	WorldDims w;
	CHECK(w.set(128, 128));
	LabelClock clock;
	auto call = [&](int x0, int y0, int z0, int x1, int y1, int z1) { // what label_region does with the clock
		const int32_t lo[3] = {x0, y0, z0}, hi[3] = {x1, y1, z1};
		LabelDims d;
		bool empty = false;
		CHECK(check_label_box(lo, hi, w.supergrid_xy, &d, &empty) == nullptr);
		const bool inside = !empty && label_clip(w, lo, hi, &d);
		clock.begun();
		if (inside) clock.launched();
	};
	const char* const none = "the last bm_scene_label_region launched nothing, or there was none";
	CHECK(says(clock.refused(), none) && clock.clocked == 0);      // before any call
	call(10, 10, 10, 10, 50, 50);                                  // an empty box
	CHECK(says(clock.refused(), none));
	call(200, 0, 0, 230, 30, 30);                                  // wholly outside
	CHECK(says(clock.refused(), none));
	call(-10, -10, -10, 20, 20, 20);                               // part of it inside: the kernels ran
	CHECK(clock.refused() == nullptr && clock.clocked == kClockedCall);
	call(0, 0, 0, 128, 128, 128);
	CHECK(clock.refused() == nullptr);
	call(0, 0, 128, 128, 128, 160);                                // outside again: the times of the call before are not this call's
	CHECK(says(clock.refused(), none) && clock.clocked == 0);
	call(5, 5, 5, 6, 6, 6);
	CHECK(clock.refused() == nullptr);
	call(5, 5, 5, 6, 6, 5);
	CHECK(says(clock.refused(), none));
}

} // namespace

int main() {
	slabs();
	offsets();
	label_boxes();
	patch_lists();
	queries();
	label_clock();
	std::printf("steps %ld\nfailures %ld\n", steps, failures);
	return failures ? 1 : 0;
}
