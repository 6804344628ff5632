// world.h -- host-side brickmap world: simplex-noise terrain -> supercells of 64-byte bricks.
// Product code (not the oracle).  Mirrors the host half of the reference's Scene
// (src/Scene.h:3-44, src/Scene.cpp:44-147), with the world dimensions made runtime.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "../../include/brickmap.h"
#include "device_types.h" // the index word and a cell's place: kIndexBits, kLoadedBit, cell_local_index

namespace bm {

constexpr int kBrickSize = 8;        // variables.h:9
constexpr int kSupercell = 16;       // variables.h:11
constexpr int kBrickWords = 16;      // variables.h:20  (512 bits)
constexpr int kCellsPerSupercell = kSupercell * kSupercell * kSupercell;
constexpr int kColumnSpan = kSupercell * kBrickSize; // 128 voxels

struct Brick {
	uint32_t data[kBrickWords];
};
static_assert(sizeof(Brick) == 64, "a brick is one 64-byte record");

struct HostSupercell {               // Scene::Supercell, Scene.h:21-29 (host part)
	std::vector<uint32_t> indices;   // 4096 words: slot | loaded | lod<<12, 0 = empty brick
	std::vector<Brick> bricks;       // bricks in generation order; slots in free_slots are empty and unused
	std::vector<uint32_t> free_slots; // host slots emptied by edits, reused (last first) before bricks grows
};

struct WorldDims {
	int grid_size = 0, grid_height = 0;         // voxels
	int cells = 0, cells_height = 0;            // bricks
	int supergrid_xy = 0, supergrid_z = 0;      // supercells
	int supercells = 0;
	bool set(int grid_size_, int grid_height_);
	int supercell_id(int sx, int sy, int sz) const { return sx + sy * supergrid_xy + sz * supergrid_xy * supergrid_xy; }
	void supercell_coords(int sci, int* sx, int* sy, int* sz) const { // the inverse
		*sx = sci % supergrid_xy;
		*sy = (sci / supergrid_xy) % supergrid_xy;
		*sz = sci / (supergrid_xy * supergrid_xy);
	}
};
static_assert(kIndexBits == BM_BRICK_INDEX_BITS && kLoadedBit == BM_BRICK_LOADED_BIT, "device_types.h and brickmap.h name one index word");

// run work(i) for i in [0, n) on up to `threads` threads, the caller's among them: THE worker pool of the host code
template <class F> void parallel_for(int n, int threads, F work) {
	threads = std::max(1, std::min(threads, n));
	std::atomic<int> next{0};
	auto loop = [&]() {
		for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) work(i);
	};
	std::vector<std::thread> pool;
	for (int i = 1; i < threads; ++i) pool.emplace_back(loop);
	loop();
	for (auto& t : pool) t.join();
}

// 2-D simplex noise + fBm exactly as the reference's terrain uses it (SimplexNoise.cpp:216-292,
// 435-450 with SimplexNoise(1,1,2,0.5), Scene.cpp:45,53).  Pure fp32, no contraction.
float simplex2(float x, float y);
float fbm2(int octaves, float x, float y);

class World {
public:
	WorldDims dims;
	std::vector<HostSupercell> supercells;
	bool generated = false;

	// terrain heights of one supercell column, 128x128, heights[x + 128*y] (Scene.cpp:47-58)
	void column_heights(int sx, int sy, float* heights) const;
	// Scene::generate_supercell (Scene.cpp:44-116)
	void generate_supercell(int sx, int sy, int sz);
	// CPU half of Scene::generate (Scene.cpp:118-147)
	void generate(int threads);
	uint64_t total_bricks() const; // non-empty bricks (host slots minus freed ones)

	// ---- dense voxels (bm_scene_load_voxels): V[z][y][x], x fastest, (grid_height, grid_size, grid_size), one byte per voxel, non-zero =
	// solid.  The canonical build of V: what build_supercell would store if the terrain were V -- a brick per cell that holds a solid
	// voxel, host slots 0, 1, 2 ... in ascending local cell index, word = slot | loaded | lod << 12, no free slots.
	static void load_supercell(const WorldDims& dims, HostSupercell& c, int sx, int sy, int sz, const uint8_t* voxels);
	void load_voxels(const uint8_t* voxels, int threads); // every supercell, one per work item; the world counts as generated afterwards
	void store_voxels(uint8_t* voxels, int threads) const; // the inverse: the host world as a dense volume of 0 / 1
	// Octant cube field for the GPU walk (device_types.h DeviceScene::cube_field): 8 planes of
	// (cells + 2)^2 * (cells_height + 2) bytes.  Plane o, cell c: edge (capped at 254) of the largest cube of empty
	// cells inside the grid that has c as its near corner and extends towards -x / -y / -z where bit 0 / 1 / 2 of o is
	// set, +x / +y / +z otherwise; 0 for a cell whose index word is non-zero, 255 for the border cells.
	void build_cube_field(std::vector<uint8_t>& field, int threads) const;

	// ---- voxel edits (bm_scene_edit): the host world stays authoritative; Scene carries the result to the device
	// 2x2x2 LoD mask of a brick's bits (Scene.cpp:95)
	static uint32_t brick_lod(const Brick& b);
	// Check a whole batch before anything changes: known op and shape, hi >= lo, radius >= 0.  false + *why on the first bad edit.
	static bool validate_edits(const bm_edit* edits, int count, std::string* why);
	// Voxel bounds [lo, hi) of one (valid) edit clipped to a world of these dimensions; false = nothing of it inside the world.
	static bool edit_bounds(const WorldDims& dims, const bm_edit& e, int lo[3], int hi[3]);
	// Apply a batch, in order, to the supercell at supercell coordinates (sx, sy, sz): set / clear the voxels, recompute the LoD masks,
	// give a cell that gains voxels a brick (a freed slot first) and a brick that becomes empty word 0 (its slot goes on free_slots).
	// touched (4096 entries, may be null) is set to 1 for every cell whose word or brick the batch may have changed.
	static void edit_supercell(const WorldDims& dims, HostSupercell& c, int sx, int sy, int sz, const bm_edit* edits, int count, uint8_t* touched);

	// ---- dense regions (bm_scene_write_region / bm_scene_read_region): a box of voxels as a volume V[z][y][x] with pitches
	// Check a region, an op and the pointers' presence before anything changes: hi >= lo, pitches that cover their extents (0 = tight,
	// filled in), a span that fits 64 bits.  *span = bytes from the first to behind the last voxel of the volume (0 for an empty box).
	static bool validate_region(bm_region* r, std::string* why, uint64_t* span);
	// The region's box clipped to the world; false = nothing of it inside (or the box is empty).
	static bool region_bounds(const WorldDims& dims, const bm_region& r, int lo[3], int hi[3]);
	// Where the merge below takes the volume's bits of a brick cell from: the volume itself (host memory; origin = the world voxel of
	// V[0][0][0]) or the bricks region.hip packed from it (one per cell of the clipped box's cells c0 ... c0 + nc, x fastest).
	struct RegionSource {
		const uint8_t* voxels = nullptr;
		int64_t row_pitch = 0, slice_pitch = 0;
		int origin[3] = {0, 0, 0};
		const Brick* packed = nullptr;
		int c0[3] = {0, 0, 0}, nc[3] = {0, 0, 0};
	};
	// THE RULE of a region write, per brick cell of one supercell, in ascending local cell index: cover = the box's voxels in the cell,
	// new = (old & ~cover) | (vol & cover) for BM_REGION_REPLACE, old | (vol & cover) for BM_EDIT_SET, old & ~(vol & cover) for
	// BM_EDIT_CLEAR.  new == old: the cell is not touched at all.  An empty cell that gains voxels takes a freed slot (last freed first),
	// else a new one; a brick that becomes empty gets word 0 and its slot goes on free_slots; otherwise the cell keeps its slot and its
	// bits and LoD mask are rewritten.  [lo, hi): the clipped box in world voxels.  touched as for edit_supercell, but only cells that changed.
	static void write_region_supercell(const WorldDims& dims, HostSupercell& c, int sx, int sy, int sz, const int lo[3], const int hi[3], int op,
									   const RegionSource& src, uint8_t* touched);
	// The box [lo, hi) (world voxels, inside the world) of the host world as bytes 0 / 1 into V, whose V[0][0][0] is world voxel `origin`.
	void store_region(const int lo[3], const int hi[3], const int origin[3], uint8_t* voxels, int64_t row_pitch, int64_t slice_pitch, int threads) const;

private:
	void build_supercell(int sx, int sy, int sz, const float* heights);
};

} // namespace bm
