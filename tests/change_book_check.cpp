// change_book_check.cpp -- a program with its own main around csrc/change_book.h (no HIP, no scene), linked with csrc/world.cpp and built plain
// and with -fsanitize=address,undefined by tests/test_change_book.py.  It changes real host worlds by World::edit_supercell and
// World::write_region_supercell over a PoolBook with a region allocator of its own, as WorldChanges does without the device calls, and compares
// what the book decides -- which supercells a box reaches, which word, arena slot and brick a touched cell sends, the two boxes of the
// FieldChange, the staging layout, the stage clocks -- with answers computed here independently.  prints "steps N" and "failures N".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../brickmap_amd/csrc/change_book.h"

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

// ---------------------------------------------------------------- (a) reach, (b) supercell_coords
// the supercells of the voxels of [lo, hi), by a scan of every voxel of the world
std::vector<int> reach_by_scan(const WorldDims& d, const int lo[3], const int hi[3]) {
	std::vector<uint8_t> hit(static_cast<size_t>(d.supercells), 0);
	for (int z = 0; z < d.grid_height; ++z)
		for (int y = 0; y < d.grid_size; ++y)
			for (int x = 0; x < d.grid_size; ++x) {
				if (x < lo[0] || x >= hi[0] || y < lo[1] || y >= hi[1] || z < lo[2] || z >= hi[2]) continue;
				hit[(x / 128) + (y / 128) * (d.grid_size / 128) + (z / 128) * (d.grid_size / 128) * (d.grid_size / 128)] = 1;
			}
	std::vector<int> out;
	for (int i = 0; i < d.supercells; ++i) if (hit[i]) out.push_back(i);
	return out;
}
void reach_is_scan(const WorldDims& d, int x0, int y0, int z0, int x1, int y1, int z1, size_t count) {
	bm_edit e{};
	e.op = BM_EDIT_SET; e.shape = BM_EDIT_BOX;
	e.lo[0] = x0; e.lo[1] = y0; e.lo[2] = z0; e.hi[0] = x1; e.hi[1] = y1; e.hi[2] = z1;
	int lo[3], hi[3];
	if (!World::edit_bounds(d, e, lo, hi)) { CHECK(count == 0); return; }
	std::vector<int> got;
	supercells_reached(d, lo, hi, &got);
	CHECK(got == reach_by_scan(d, lo, hi) && got.size() == count);
}
void reach() {
	WorldDims flat, cube, tall;
	CHECK(flat.set(256, 128) && cube.set(128, 128) && tall.set(256, 384));
	reach_is_scan(flat, 0, 0, 0, 128, 128, 128, 1);     // ends on the supercell's faces
	reach_is_scan(flat, 0, 0, 0, 127, 127, 127, 1);     // one voxel short
	reach_is_scan(flat, 0, 0, 0, 129, 129, 129, 4);     // one voxel beyond (z: clipped by the world)
	reach_is_scan(flat, 128, 0, 0, 256, 128, 128, 1);   // begins on a face
	reach_is_scan(flat, 127, 127, 5, 128, 128, 6, 1);   // the last voxel of supercell 0
	reach_is_scan(flat, 127, 127, 5, 129, 128, 6, 2);
	reach_is_scan(flat, 128, 128, 127, 129, 129, 128, 1);
	reach_is_scan(flat, -50, 100, -50, 1000, 130, 1000, 4); // clipped by the world on four sides
	reach_is_scan(flat, 256, 0, 0, 300, 10, 10, 0);     // outside
	reach_is_scan(cube, -5, -5, -5, 200, 200, 200, 1);
	reach_is_scan(cube, 127, 127, 127, 128, 128, 128, 1);
	reach_is_scan(tall, 100, 100, 0, 128, 128, 128, 1);
	reach_is_scan(tall, 100, 100, 0, 128, 128, 129, 2); // one voxel beyond, along z
	reach_is_scan(tall, 127, 127, 127, 129, 129, 257, 12);
	reach_is_scan(tall, 0, 0, 255, 256, 256, 256, 4);
	int seen = 0;
	for (int sz = 0; sz < tall.supergrid_z; ++sz)
		for (int sy = 0; sy < tall.supergrid_xy; ++sy)
			for (int sx = 0; sx < tall.supergrid_xy; ++sx, ++seen) {
				int x = -1, y = -1, z = -1;
				tall.supercell_coords(seen, &x, &y, &z);
				CHECK(x == sx && y == sy && z == sz && tall.supercell_id(x, y, z) == seen);
			}
	CHECK(seen == tall.supercells && seen == 12);
}

// ---------------------------------------------------------------- a host world with its book and a model of the device's index grid
struct Arena { // as in pool_book_check.cpp
	RegionLists regions;
	int alloc(uint32_t bricks, uint32_t* offset) {
		if (!regions.take_free(bricks, offset)) *offset = regions.claim_top(bricks);
		return 0;
	}
	auto fn() { return [this](uint32_t bricks, uint32_t* offset) { return alloc(bricks, offset); }; }
};

// what one change did: the batch, and what the test needs to judge it
struct Applied {
	CellBatch batch;
	std::vector<int> reached;
	std::vector<std::vector<uint32_t>> old_words;
	std::vector<std::vector<uint8_t>> touched;
};
struct Tally { long gained = 0, lost = 0, kept = 0, same_word = 0, batches = 0, crossing = 0, cells = 0, moves = 0; };

struct Rig {
	World world;
	Arena arena;
	PoolBook book{&arena.regions};
	std::vector<uint32_t> grid; // the device's index words, as the batches' (cell, word) pairs leave them

	Rig(int size, int height, const std::vector<uint8_t>& volume, bool preloaded) {
		world.dims.set(size, height);
		world.load_voxels(volume.data(), 2);
		const int n = world.dims.supercells;
		arena.regions.reset();
		book.begin_rebuild(n);
		grid.assign(static_cast<size_t>(n) * kCellsPerSupercell, 0u);
		for (int i = 0; i < n; ++i) {
			const HostSupercell& c = world.supercells[i];
			if (preloaded) book.adopt_exact(i, arena.regions.claim_top(c.bricks.size()), c.bricks.size(), c.free_slots);
			else CHECK(book.start_pool(i, c.bricks.size(), arena.fn()) == 0);
			for (int j = 0; j < kCellsPerSupercell; ++j) {
				const uint32_t w = c.indices[j];
				grid[static_cast<size_t>(i) * kCellsPerSupercell + j] = preloaded ? w : (w ? BM_BRICK_UNLOADED_BIT | (w & BM_BRICK_LOD_BITS) : 0u);
			}
		}
		book.rebuilt(preloaded);
	}
	Rig(const Rig&) = delete;

	// a streaming scene's requests, serviced (Residency::service_ring without the device): the bricks become resident, the words say so
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
		auto staged = [&](uint32_t i, int sci, uint32_t, uint32_t device_word) {
			grid[static_cast<size_t>(sci) * kCellsPerSupercell + cell_local_index(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2])] = device_word;
		};
		CHECK(book.ring_slots(pos.data(), count, lookup, arena.fn(), staged, &kept) == 0);
		book.commit_batch();
	}

	void stage(Applied& a, size_t i) { // WorldChanges::stage
		const int sci = a.reached[i];
		const HostSupercell& c = world.supercells[sci];
		CHECK(book.rebind(sci, a.old_words[i].data(), c.indices.data(), a.touched[i].data(), c.bricks.size(), arena.fn()) == 0);
		a.batch.add_supercell(world.dims, sci, c, a.old_words[i], a.touched[i].data(), book.pool(sci));
	}
	// WorldChanges::edit and ::write_region (a host volume) up to the submission
	void edit(const std::vector<bm_edit>& edits, Applied* out) {
		const WorldDims& d = world.dims;
		Applied& a = *out;
		std::string why;
		CHECK(World::validate_edits(edits.data(), static_cast<int>(edits.size()), &why));
		for (const bm_edit& e : edits) {
			int lo[3], hi[3];
			if (World::edit_bounds(d, e, lo, hi)) supercells_reached(d, lo, hi, &a.reached);
		}
		std::sort(a.reached.begin(), a.reached.end());
		a.reached.erase(std::unique(a.reached.begin(), a.reached.end()), a.reached.end());
		a.old_words.resize(a.reached.size());
		a.touched.resize(a.reached.size());
		book.begin_batch();
		for (size_t i = 0; i < a.reached.size(); ++i) {
			HostSupercell& c = world.supercells[a.reached[i]];
			int sx, sy, sz;
			d.supercell_coords(a.reached[i], &sx, &sy, &sz);
			a.old_words[i] = c.indices;
			a.touched[i].assign(kCellsPerSupercell, 0);
			World::edit_supercell(d, c, sx, sy, sz, edits.data(), static_cast<int>(edits.size()), a.touched[i].data());
			stage(a, i);
		}
	}
	void write(bm_region r, int op, const std::vector<uint8_t>& volume, Applied* out) {
		const WorldDims& d = world.dims;
		Applied& a = *out;
		std::string why;
		uint64_t span = 0;
		CHECK(World::validate_region(&r, &why, &span) && span <= volume.size());
		int lo[3], hi[3];
		book.begin_batch();
		if (!World::region_bounds(d, r, lo, hi)) return;
		const RegionDims rd = region_dims(d, r, lo, hi);
		World::RegionSource src;
		for (int k = 0; k < 3; ++k) { src.c0[k] = rd.c0[k]; src.nc[k] = rd.nc[k]; src.origin[k] = r.lo[k]; }
		src.voxels = volume.data();
		src.row_pitch = r.row_pitch;
		src.slice_pitch = r.slice_pitch;
		supercells_reached(d, lo, hi, &a.reached);
		a.old_words.resize(a.reached.size());
		a.touched.resize(a.reached.size());
		for (size_t i = 0; i < a.reached.size(); ++i) {
			HostSupercell& c = world.supercells[a.reached[i]];
			int sx, sy, sz;
			d.supercell_coords(a.reached[i], &sx, &sy, &sz);
			a.old_words[i] = c.indices;
			a.touched[i].assign(kCellsPerSupercell, 0);
			World::write_region_supercell(d, c, sx, sy, sz, lo, hi, op, src, a.touched[i].data());
		}
		for (size_t i = 0; i < a.reached.size(); ++i) stage(a, i);
	}

	// the batch against answers computed here; then it is "submitted": replayed into the grid, committed, and the grid is the host world's
	bool judge(const Applied& a, Tally* t) {
		const WorldDims& d = world.dims;
		const CellBatch& b = a.batch;
		bool ok = b.cells.size() == b.words.size() && b.cells.size() == b.slots.size() && b.cells.size() == b.bricks.size();
		size_t k = 0;
		int box_lo[3] = {1 << 30, 1 << 30, 1 << 30}, box_hi[3] = {-1, -1, -1}, touch_lo[2] = {1 << 30, 1 << 30}, touch_hi[2] = {-1, -1};
		for (size_t i = 0; i < a.reached.size(); ++i) {
			const int sci = a.reached[i];
			ok = ok && (i == 0 || a.reached[i - 1] < sci);
			const HostSupercell& c = world.supercells[sci];
			const PoolBook::Pool& pool = book.pool(sci);
			const int cx0 = 16 * (sci % (d.grid_size / 128)), cy0 = 16 * ((sci / (d.grid_size / 128)) % (d.grid_size / 128)), cz0 = 16 * (sci / ((d.grid_size / 128) * (d.grid_size / 128)));
			for (int j = 0; j < kCellsPerSupercell; ++j) {
				const uint32_t ow = a.old_words[i][j], nw = c.indices[j];
				const int g[3] = {cx0 + j % 16, cy0 + (j / 16) % 16, cz0 + j / 256};
				if ((ow != 0) != (nw != 0))
					for (int q = 0; q < 3; ++q) { box_lo[q] = std::min(box_lo[q], g[q]); box_hi[q] = std::max(box_hi[q], g[q]); }
				if (!a.touched[i][j]) { ok = ok && ow == nw; continue; } // (and absent from the batch: the entries are counted)
				for (int q = 0; q < 2; ++q) { touch_lo[q] = std::min(touch_lo[q], g[q]); touch_hi[q] = std::max(touch_hi[q], g[q]); }
				if (k >= b.cells.size()) { ok = false; continue; }
				// the three-case rule: no brick / a brick the device does not hold / a brick in a pool slot
				const uint32_t slot = nw ? pool.dev_slot[nw & 0xFFFu] : 0xFFFFu;
				const uint32_t word = nw == 0 ? 0u : slot == 0xFFFFu ? 0x40000000u | (nw & 0x000FF000u) : slot | 0x80000000u | (nw & 0x000FF000u);
				Brick brick{};
				if (nw) brick = c.bricks[nw & 0xFFFu];
				ok = ok && b.cells[k] == static_cast<uint32_t>(sci) * 4096u + static_cast<uint32_t>(j) && b.words[k] == word &&
					 b.slots[k] == (nw != 0 && slot != 0xFFFFu ? pool.base + slot : 0xFFFFFFFFu) && std::memcmp(&b.bricks[k], &brick, sizeof brick) == 0;
				ok = ok && (nw == 0 || slot == 0xFFFFu || slot < pool.high) && (!book.preloaded() || nw == 0 || slot != 0xFFFFu);
				++k;
				if (!ow && nw) t->gained++;
				else if (ow && !nw) t->lost++;
				else if (ow == nw) t->same_word++;
				else t->kept++;
			}
		}
		ok = ok && k == b.cells.size();
		const FieldChange& ch = b.change;
		for (int q = 0; q < 3; ++q) ok = ok && ch.box_lo[q] == box_lo[q] && ch.box_hi[q] == box_hi[q];
		for (int q = 0; q < 2; ++q) ok = ok && ch.touch_lo[q] == touch_lo[q] && ch.touch_hi[q] == touch_hi[q];
		ok = ok && ch.occupancy() == (box_hi[0] >= 0);
		ok = ok && b.clocked() == (k == 0 ? 0u : box_hi[0] >= 0 ? 12u : 4u);
		t->batches++;
		t->cells += static_cast<long>(k);
		t->moves += static_cast<long>(book.moves().size());
		if (a.reached.size() > 1 && k > 0 && b.cells.front() / 4096u != b.cells.back() / 4096u) t->crossing++;
		// ---- submitted
		for (size_t n = 0; n < b.cells.size(); ++n) grid[b.cells[n]] = b.words[n];
		book.commit_batch();
		for (int sci = 0; sci < d.supercells; ++sci) {
			const HostSupercell& c = world.supercells[sci];
			for (int j = 0; j < kCellsPerSupercell; ++j) {
				const uint32_t w = c.indices[j];
				ok = ok && grid[static_cast<size_t>(sci) * kCellsPerSupercell + j] == PoolBook::device_word(w, w ? book.pool(sci).dev_slot[w & BM_BRICK_INDEX_BITS] : kNoDeviceSlot);
			}
		}
		return ok;
	}
};

bm_edit box(int op, int x0, int y0, int z0, int x1, int y1, int z1) {
	bm_edit e{};
	e.op = op; e.shape = BM_EDIT_BOX;
	e.lo[0] = x0; e.lo[1] = y0; e.lo[2] = z0; e.hi[0] = x1; e.hi[1] = y1; e.hi[2] = z1;
	return e;
}
bm_edit sphere(int op, int x, int y, int z, int radius) {
	bm_edit e{};
	e.op = op; e.shape = BM_EDIT_SPHERE;
	e.center[0] = x; e.center[1] = y; e.center[2] = z; e.radius = radius;
	return e;
}
bm_region region(int x0, int y0, int z0, int x1, int y1, int z1) {
	bm_region r{};
	r.lo[0] = x0; r.lo[1] = y0; r.lo[2] = z0; r.hi[0] = x1; r.hi[1] = y1; r.hi[2] = z1;
	return r;
}

// a floor two cells thick, a tower across the face between supercells 0 and 1 (x = 128), a slab in the air and one full brick
std::vector<uint8_t> hand_made(int size, int height) {
	std::vector<uint8_t> v(static_cast<size_t>(size) * size * height, 0);
	auto fill = [&](int x0, int y0, int z0, int x1, int y1, int z1) {
		for (int z = z0; z < z1; ++z)
			for (int y = y0; y < y1; ++y)
				for (int x = x0; x < std::min(x1, size); ++x) v[(static_cast<size_t>(z) * size + y) * size + x] = 1;
	};
	fill(0, 0, 0, size, size, 16);
	fill(size / 2 - 12, 40, 16, size / 2 + 12, 56, 60);
	fill(20, 90, 80, 60, 120, 83);
	fill(96, 96, 96, 104, 104, 104);
	return v;
}

// ---------------------------------------------------------------- (c) add_supercell on a preloaded and on a streaming book
void hand_made_changes(int size, int height, bool preloaded) {
	Rig rig(size, height, hand_made(size, height), preloaded);
	const int mid = size / 2; // a supercell face where the world is 256 wide, the middle of the only supercell where it is 128
	Tally t;
	if (!preloaded) { // some bricks resident: of the floor (cells (2 ... 9, 5, 0)), of the tower on both sides of the face, and the full brick
		std::vector<int> pos;
		for (int cx = 2; cx < 10; ++cx) pos.insert(pos.end(), {cx, 5, 0});
		pos.insert(pos.end(), {mid / 8 - 1, 5, 3, mid / 8, 5, 3, mid / 8 - 1, 6, 4, 12, 12, 12});
		rig.request(pos);
		CHECK(rig.book.resident_bricks() == 12);
	}
	{ // an empty batch: edits outside the world, and a clear of empty space
		Applied a;
		rig.edit({box(BM_EDIT_SET, size, 0, 0, size + 8, 8, 8), box(BM_EDIT_CLEAR, 8, 8, 112, 16, 16, 120)}, &a);
		CHECK(a.batch.cells.empty() && a.batch.clocked() == 0u && !a.batch.change.occupancy());
		CHECK(rig.judge(a, &t));
	}
	{ // bits only: a SET of voxels that are solid already (touched, the words stay), and an octant out of one of those full bricks (its LoD mask changes)
		Applied a;
		rig.edit({box(BM_EDIT_SET, 16, 40, 0, 40, 48, 8), box(BM_EDIT_CLEAR, 16, 40, 0, 20, 44, 4)}, &a);
		CHECK(a.batch.cells.size() == 3 && a.batch.clocked() == kClockedScatter && !a.batch.change.occupancy());
		CHECK(a.batch.change.touch_lo[0] == 2 && a.batch.change.touch_hi[0] == 4 && a.batch.change.touch_lo[1] == 5 && a.batch.change.touch_hi[1] == 5);
		CHECK(rig.judge(a, &t));
		CHECK(t.same_word == 2 && t.kept == 1);
	}
	{ // one batch across the face: the tower loses a slice of whole bricks, the air next to it gains a box, the full brick loses a corner
		Applied a;
		rig.edit({box(BM_EDIT_CLEAR, mid - 12, 40, 32, mid + 12, 56, 40), box(BM_EDIT_SET, mid - 20, 60, 20, mid + 20, 70, 30), sphere(BM_EDIT_CLEAR, 96, 96, 96, 6)}, &a);
		CHECK(a.batch.clocked() == (kClockedScatter | kClockedField) && a.reached.size() == (size == 256 ? 2u : 1u));
		CHECK(a.batch.change.box_lo[2] == 2 && a.batch.change.box_hi[2] == 4 && a.batch.change.box_lo[0] == mid / 8 - 3 && a.batch.change.box_hi[0] == mid / 8 + 2);
		CHECK(rig.judge(a, &t));
		CHECK(t.gained > 0 && t.lost > 0 && t.kept > 1);
	}
	// region writes, all three ops, from a volume with a checkerboard of 4-voxel blocks: over the slab and the air around it ...
	const int n = 48;
	std::vector<uint8_t> checker(static_cast<size_t>(n) * n * n);
	for (int z = 0; z < n; ++z)
		for (int y = 0; y < n; ++y)
			for (int x = 0; x < n; ++x) checker[(static_cast<size_t>(z) * n + y) * n + x] = ((x / 4 + y / 4 + z / 4) & 1) ? 7 : 0;
	for (const int op : {BM_EDIT_SET, BM_EDIT_CLEAR, BM_REGION_REPLACE}) {
		Applied a;
		rig.write(region(30, 85, 70, 30 + n, 85 + n, 70 + n), op, checker, &a);
		CHECK(rig.judge(a, &t));
		Applied again; // the same write once more changes nothing: no cell is touched
		rig.write(region(30, 85, 70, 30 + n, 85 + n, 70 + n), op, checker, &again);
		CHECK(again.batch.cells.empty() && rig.judge(again, &t));
	}
	{ // ... and across the face and out of the world's bottom, with pitches: zeros empty what is left of the tower, and the floor under it
		std::vector<uint8_t> zeros(static_cast<size_t>(70) * 50 * 64, 0);
		bm_region r = region(mid - 30, 30, -10, mid + 30, 70, 60);
		r.row_pitch = 64;
		r.slice_pitch = 64 * 50;
		int lo[3], hi[3];
		CHECK(World::region_bounds(rig.world.dims, r, lo, hi) && lo[2] == 0 && hi[2] == 60);
		const RegionDims rd = region_dims(rig.world.dims, r, lo, hi);
		CHECK(rd.c0[0] == (mid - 30) / 8 && rd.nc[0] == 8 && rd.c0[2] == 0 && rd.nc[2] == 8 && rd.g0 == rd.c0[0] / 16 && rd.org[2] == -10 && rd.lo[2] == 0 && rd.hi[0] == mid + 30 && rd.sg_xy == static_cast<uint32_t>(size / 128) && rd.sg_xy2 == rd.sg_xy * rd.sg_xy && rd.row_pitch == 64 && rd.slice_pitch == 3200);
		Applied a;
		rig.write(r, BM_REGION_REPLACE, zeros, &a);
		CHECK(a.batch.change.occupancy() && rig.judge(a, &t));
	}
	CHECK(t.gained > 20 && t.lost > 20 && t.kept > 5 && t.same_word >= 2);
	CHECK(size == 256 ? t.crossing >= 2 : t.crossing == 0);
	CHECK(preloaded ? rig.book.resident_bricks() == rig.world.total_bricks() : rig.book.resident_bricks() < 12);
}

// ---------------------------------------------------------------- (d) the staging layout
void staging() {
	for (const size_t moves : {0u, 3u})
		for (const size_t n : {0u, 1u, 16u, 17u, 860u, 861u, 862u, 863u}) {
			CellBatch b;
			std::vector<PoolMove> mv;
			for (size_t i = 0; i < moves; ++i) mv.push_back(PoolMove{static_cast<uint32_t>(100 + i), static_cast<uint32_t>(200 + i), static_cast<uint32_t>(300 + i), static_cast<uint32_t>(i)});
			for (size_t i = 0; i < n; ++i) {
				b.cells.push_back(static_cast<uint32_t>(7 * i + 1));
				b.words.push_back(static_cast<uint32_t>(0x80000000u + i));
				b.slots.push_back(static_cast<uint32_t>(i % 5 ? 3 * i : 0xFFFFFFFFu));
				Brick k;
				for (int w = 0; w < kBrickWords; ++w) k.data[w] = static_cast<uint32_t>(i * 16 + w) * 2654435761u;
				b.bricks.push_back(k);
			}
			const StagingLayout at(moves, n);
			// in order, not overlapping, each section on a 64-byte line, nothing behind the bricks
			CHECK(at.o_cells % 64 == 0 && at.o_words % 64 == 0 && at.o_slots % 64 == 0 && at.o_bricks % 64 == 0);
			CHECK(moves * 16 <= at.o_cells && at.o_cells + 4 * n <= at.o_words && at.o_words + 4 * n <= at.o_slots && at.o_slots + 4 * n <= at.o_bricks && at.o_bricks + 64 * n == at.bytes);
			CHECK(at.o_cells < moves * 16 + 64 && at.o_words < at.o_cells + 4 * n + 64 && at.o_slots < at.o_words + 4 * n + 64 && at.o_bricks < at.o_slots + 4 * n + 64); // no line wasted
			std::vector<char> buf(at.bytes + 64, static_cast<char>(0xA5));
			at.fill(buf.data(), mv, b);
			bool back = true, poison = true;
			std::vector<uint8_t> written(buf.size(), 0);
			auto section = [&](size_t at_byte, const void* want, size_t bytes) {
				if (bytes == 0) return;
				back = back && std::memcmp(buf.data() + at_byte, want, bytes) == 0;
				std::fill(written.begin() + static_cast<ptrdiff_t>(at_byte), written.begin() + static_cast<ptrdiff_t>(at_byte + bytes), 1);
			};
			section(0, mv.data(), moves * sizeof(PoolMove));
			section(at.o_cells, b.cells.data(), n * 4);
			section(at.o_words, b.words.data(), n * 4);
			section(at.o_slots, b.slots.data(), n * 4);
			section(at.o_bricks, b.bricks.data(), n * sizeof(Brick));
			for (size_t i = 0; i < buf.size(); ++i) poison = poison && (written[i] || buf[i] == static_cast<char>(0xA5));
			CHECK(back && poison);
		}
	// written out by hand: 16 cells fill their 64-byte lines, the 17th takes a second one; three moves take one line
	const StagingLayout a(0, 16), b(3, 17), c(0, 1), z(0, 0);
	CHECK(a.o_cells == 0 && a.o_words == 64 && a.o_slots == 128 && a.o_bricks == 192 && a.bytes == 1216);
	CHECK(b.o_cells == 64 && b.o_words == 192 && b.o_slots == 320 && b.o_bricks == 448 && b.bytes == 1536);
	CHECK(c.o_words == 64 && c.o_bricks == 192 && c.bytes == 256 && z.bytes == 0 && StagingLayout(3, 0).bytes == 64);
	// 76 bytes a cell: 860 and 861 cells stay below the 64 KiB the staging starts with, 862 fill it exactly, 863 -- or 862 and a move -- do not fit
	CHECK(StagingLayout(0, 860).bytes == 65408 && StagingLayout(0, 861).bytes == 65472 && StagingLayout(3, 860).bytes == 65472 && StagingLayout(3, 861).bytes == 65536);
	CHECK(StagingLayout(0, 862).bytes == 65536 && StagingLayout(0, 863).bytes == 65600 && StagingLayout(3, 862).bytes == 65600);
	CHECK(StagingLayout::grown(1) == 65536 && StagingLayout::grown(32768) == 65536 && StagingLayout::grown(32769) == 65538 && StagingLayout::grown(65600) == 131200);
}

// ---------------------------------------------------------------- (e) the clocks
void clocks() {
	const unsigned S = kClockedScatter, F = kClockedField, C = kClockedCall, P = kClockedPack;
	CHECK(C == 1 && P == 2 && S == 4 && F == 8);
	// an edit: the batch's own stages, or -- a batch that scatters nothing -- what the last one left
	CHECK(edit_clocked(0, 0) == 0 && edit_clocked(0, S) == S && edit_clocked(0, S | F) == (S | F));
	CHECK(edit_clocked(S, 0) == S && edit_clocked(S | F, 0) == (S | F) && edit_clocked(S | F, S) == S && edit_clocked(S, S | F) == (S | F));
	const float raw[4] = {1.5f, 2.5f, 3.5f, 4.5f};
	float a = -1, b = -1, c = -1, d = -1;
	edit_ms(S, raw, &a, &b);
	CHECK(a == 1.5f && b == 0.0f);
	edit_ms(S | F, raw, &a, &b);
	CHECK(a == 1.5f && b == 2.5f);
	// a region write: the call, the pack of a device volume, and the batch's stages
	CHECK(region_clocked(false, 0) == 1 && region_clocked(false, S) == 5 && region_clocked(false, S | F) == 13);
	CHECK(region_clocked(true, 0) == 3 && region_clocked(true, S) == 7 && region_clocked(true, S | F) == 15);
	const struct { unsigned flags; float want[4]; } cases[] = {
		{1, {0.f, 0.f, 0.f, 0.f}},  {5, {0.f, 0.f, 3.5f, 0.f}},  {13, {0.f, 0.f, 3.5f, 4.5f}},
		{3, {1.5f, 2.5f, 0.f, 0.f}}, {7, {1.5f, 2.5f, 3.5f, 0.f}}, {15, {1.5f, 2.5f, 3.5f, 4.5f}},
	};
	for (const auto& k : cases) {
		a = b = c = d = -1;
		region_ms(k.flags, raw, &a, &b, &c, &d);
		CHECK(a == k.want[0] && b == k.want[1] && c == k.want[2] && d == k.want[3]);
	}
}

// ---------------------------------------------------------------- (f) a seeded script of random edits and region writes
void random_script(bool preloaded, int rounds) {
	Rig rig(256, 128, hand_made(256, 128), preloaded);
	const WorldDims& d = rig.world.dims;
	Rng rng;
	rng.s += preloaded;
	Tally t;
	for (int step = 0; step < rounds; ++step) {
		if (!preloaded && step % 8 == 0) { // frames ask for bricks, and get them
			std::vector<int> pos;
			for (int i = rng.between(1, 30); i > 0; --i) pos.insert(pos.end(), {rng.below(d.cells), rng.below(d.cells), rng.below(12)});
			rig.request(pos);
		}
		Applied a;
		if (rng.below(2)) {
			std::vector<bm_edit> edits;
			for (int i = rng.between(1, 3); i > 0; --i) {
				const int op = rng.below(2) ? BM_EDIT_SET : BM_EDIT_CLEAR;
				const int x = rng.between(-20, 270), y = rng.between(-20, 270), z = rng.between(-20, 140);
				if (rng.below(2)) edits.push_back(box(op, x, y, z, x + rng.below(50), y + rng.below(50), z + rng.below(50)));
				else edits.push_back(sphere(op, x, y, z, rng.below(24)));
			}
			rig.edit(edits, &a);
		} else {
			const int nx = rng.between(0, 40), ny = rng.between(0, 40), nz = rng.between(0, 40);
			const int x = rng.between(-20, 250), y = rng.between(-20, 250), z = rng.between(-20, 120);
			const int density = rng.below(4); // none, some, most, all of the volume solid
			std::vector<uint8_t> volume(static_cast<size_t>(nx) * ny * nz + 1);
			for (uint8_t& v : volume) v = density == 0 ? 0 : density == 3 ? 1 : (rng.below(8) < (density == 1 ? 1 : 7));
			const int ops[3] = {BM_REGION_REPLACE, BM_EDIT_SET, BM_EDIT_CLEAR};
			rig.write(region(x, y, z, x + nx, y + ny, z + nz), ops[rng.below(3)], volume, &a);
		}
		CHECK(rig.judge(a, &t));
	}
	CHECK(t.batches == rounds && t.gained > 1000 && t.lost > 100 && t.kept > 300 && t.same_word > 100 && t.crossing > 20); // (the script does what it is for)
	CHECK(preloaded ? t.moves > 3 && rig.book.resident_bricks() == rig.world.total_bricks() : rig.book.resident_bricks() > 0 && rig.book.resident_bricks() < rig.world.total_bricks());
}

} // namespace

int main() {
	reach();
	for (const bool preloaded : {true, false}) {
		hand_made_changes(256, 128, preloaded);
		hand_made_changes(128, 128, preloaded);
	}
	staging();
	clocks();
	random_script(true, 200);
	random_script(false, 200);
	std::printf("steps %ld\nfailures %ld\n", steps, failures);
	return failures ? 1 : 0;
}
