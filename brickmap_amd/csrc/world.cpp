// world.cpp -- CPU world build (the reference keeps this on the CPU too: BASELINE config 1
// "SimplexNoise world built by Scene.cpp on CPU (plumbing, no GPU)").
//
// Same results as the reference generator (src/Scene.cpp:44-147 + src/SimplexNoise.cpp), but
// organised for large worlds: the heightfield of a supercell column is computed once and
// reused for every z layer, and bricks that lie wholly below / above the terrain are
// emitted without touching their 512 voxels.
#include "world.h"
#include "voxel_bits.h"

#include <algorithm>
#include <climits>
#include <cstring>

namespace bm {

bool WorldDims::set(int grid_size_, int grid_height_) {
	if (grid_size_ <= 0 || grid_height_ <= 0 || grid_size_ % kColumnSpan || grid_height_ % kColumnSpan) return false;
	grid_size = grid_size_;
	grid_height = grid_height_;
	cells = grid_size / kBrickSize;
	cells_height = grid_height / kBrickSize;
	supergrid_xy = cells / kSupercell;
	supergrid_z = cells_height / kSupercell;
	supercells = supergrid_xy * supergrid_xy * supergrid_z;
	return true;
}

// ---------------------------------------------------------------- simplex noise
namespace {

// Ken Perlin's permutation (SimplexNoise.cpp:73-87); must be these exact 256 values.
const uint8_t kPerm[256] = {
	151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225, 140, 36, 103, 30, 69, 142, 8, 99, 37, 240,
	21, 10, 23, 190, 6, 148, 247, 120, 234, 75, 0, 26, 197, 62, 94, 252, 219, 203, 117, 35, 11, 32, 57, 177, 33, 88,
	237, 149, 56, 87, 174, 20, 125, 136, 171, 168, 68, 175, 74, 165, 71, 134, 139, 48, 27, 166, 77, 146, 158, 231, 83,
	111, 229, 122, 60, 211, 133, 230, 220, 105, 92, 41, 55, 46, 245, 40, 244, 102, 143, 54, 65, 25, 63, 161, 1, 216,
	80, 73, 209, 76, 132, 187, 208, 89, 18, 169, 200, 196, 135, 130, 116, 188, 159, 86, 164, 100, 109, 198, 173, 186,
	3, 64, 52, 217, 226, 250, 124, 123, 5, 202, 38, 147, 118, 126, 255, 82, 85, 212, 207, 206, 59, 227, 47, 16, 58,
	17, 182, 189, 28, 42, 223, 183, 170, 213, 119, 248, 152, 2, 44, 154, 163, 70, 221, 153, 101, 155, 167, 43, 172, 9,
	129, 22, 39, 253, 19, 98, 108, 110, 79, 113, 224, 232, 178, 185, 112, 104, 218, 246, 97, 228, 251, 34, 242, 193,
	238, 210, 144, 12, 191, 179, 162, 241, 81, 51, 145, 235, 249, 14, 239, 107, 49, 192, 214, 31, 181, 199, 106, 157,
	184, 84, 204, 176, 115, 121, 50, 45, 127, 4, 150, 254, 138, 236, 205, 93, 222, 114, 67, 29, 24, 72, 243, 141, 128,
	195, 78, 66, 215, 61, 156, 180
};

inline int perm_at(int i) { return kPerm[static_cast<uint8_t>(i)]; }

inline int floor_to_int(float v) { // SimplexNoise.cpp:47-50
	const int t = static_cast<int>(v);
	return v < t ? t - 1 : t;
}

// one simplex corner: falloff^4 * gradient . offset.  The gradient pick keeps the upstream
// quirk (hash masked with 0x3F but compared against 4, SimplexNoise.cpp:144-149).
inline float corner(int hash, float dx, float dy) {
	float falloff = 0.5f - dx * dx - dy * dy;
	if (falloff < 0.0f) return 0.0f;
	const int h = hash & 0x3F;
	const float u = h < 4 ? dx : dy;
	const float v = h < 4 ? dy : dx;
	const float g = ((h & 1) ? -u : u) + ((h & 2) ? -2.0f * v : 2.0f * v);
	falloff *= falloff;
	return falloff * falloff * g;
}

} // namespace

float simplex2(float x, float y) { // SimplexNoise.cpp:216-292
	const float kSkew = 0.366025403f;   // (sqrt(3)-1)/2
	const float kUnskew = 0.211324865f; // (3-sqrt(3))/6
	const float skew = (x + y) * kSkew;
	const int ci = floor_to_int(x + skew);
	const int cj = floor_to_int(y + skew);
	const float unskew = static_cast<float>(ci + cj) * kUnskew;
	const float dx0 = x - (ci - unskew);
	const float dy0 = y - (cj - unskew);
	const int oi = dx0 > dy0 ? 1 : 0; // which of the two triangles of the cell
	const int oj = 1 - oi;
	const float dx1 = dx0 - oi + kUnskew;
	const float dy1 = dy0 - oj + kUnskew;
	const float dx2 = dx0 - 1.0f + 2.0f * kUnskew;
	const float dy2 = dy0 - 1.0f + 2.0f * kUnskew;
	const float n0 = corner(perm_at(ci + perm_at(cj)), dx0, dy0);
	const float n1 = corner(perm_at(ci + oi + perm_at(cj + oj)), dx1, dy1);
	const float n2 = corner(perm_at(ci + 1 + perm_at(cj + 1)), dx2, dy2);
	return 45.23065f * (n0 + n1 + n2);
}

float fbm2(int octaves, float x, float y) { // SimplexNoise.cpp:435-450, lacunarity 2, persistence 0.5
	float sum = 0.f, norm = 0.f, freq = 1.0f, amp = 1.0f;
	for (int o = 0; o < octaves; ++o) {
		sum += amp * simplex2(x * freq, y * freq);
		norm += amp;
		freq *= 2.0f;
		amp *= 0.5f;
	}
	return sum / norm;
}

// ---------------------------------------------------------------- terrain -> bricks
void World::column_heights(int sx, int sy, float* heights) const {
	const float half = dims.grid_height / 2.f;
	for (int y = 0; y < kColumnSpan; ++y) {
		const float fy = (sy * kColumnSpan + y) / 2048.f;
		for (int x = 0; x < kColumnSpan; ++x) {
			float h = fbm2(8, (sx * kColumnSpan + x) / 2048.f, fy);
			h *= half;
			h += half;
			heights[x + y * kColumnSpan] = h;
		}
	}
}

void World::build_supercell(int sx, int sy, int sz, const float* heights) {
	HostSupercell& cell = supercells[dims.supercell_id(sx, sy, sz)];
	cell.indices.assign(kCellsPerSupercell, 0u);
	cell.bricks.clear();
	cell.free_slots.clear();

	// per brick column: lowest / highest terrain height under its 8x8 footprint
	float lo[kSupercell * kSupercell], hi[kSupercell * kSupercell];
	for (int by = 0; by < kSupercell; ++by)
		for (int bx = 0; bx < kSupercell; ++bx) {
			float mn = heights[bx * kBrickSize + by * kBrickSize * kColumnSpan], mx = mn;
			for (int cy = 0; cy < kBrickSize; ++cy)
				for (int cx = 0; cx < kBrickSize; ++cx) {
					const float h = heights[bx * kBrickSize + cx + (by * kBrickSize + cy) * kColumnSpan];
					mn = std::min(mn, h);
					mx = std::max(mx, h);
				}
			lo[bx + by * kSupercell] = mn;
			hi[bx + by * kSupercell] = mx;
		}

	for (int bz = 0; bz < kSupercell; ++bz) {
		const int z0 = (sz * kSupercell + bz) * kBrickSize; // global z of the brick's lowest voxel layer
		for (int by = 0; by < kSupercell; ++by)
			for (int bx = 0; bx < kSupercell; ++bx) {
				const int col = bx + by * kSupercell;
				// voxel is solid iff z < height (int compared as float, Scene.cpp:90)
				if (!(static_cast<float>(z0) < hi[col])) continue; // every voxel at or above the terrain: empty brick
				Brick brick;
				uint32_t lod = 0;
				if (static_cast<float>(z0 + kBrickSize - 1) < lo[col]) {
					std::memset(brick.data, 0xFF, sizeof brick.data); // wholly under the terrain
					lod = 0xFFu;
				} else {
					std::memset(brick.data, 0, sizeof brick.data);
					for (int cy = 0; cy < kBrickSize; ++cy)
						for (int cx = 0; cx < kBrickSize; ++cx) {
							const float h = heights[bx * kBrickSize + cx + (by * kBrickSize + cy) * kColumnSpan];
							for (int cz = 0; cz < kBrickSize; ++cz) {
								if (!(static_cast<float>(z0 + cz) < h)) break; // z ascending: the rest is air
								const int bit = cx + cy * kBrickSize + cz * kBrickSize * kBrickSize; // Scene.cpp:91-93
								brick.data[bit >> 5] |= 1u << (bit & 31);
								lod |= 1u << (((cx & 4) >> 2) + ((cy & 4) >> 1) + (cz & 4)); // Scene.cpp:95
							}
						}
				}
				cell.bricks.push_back(brick);
				cell.indices[bx + by * kSupercell + bz * kSupercell * kSupercell] =
					static_cast<uint32_t>(cell.bricks.size() - 1) | BM_BRICK_LOADED_BIT | (lod << 12); // Scene.cpp:104
			}
	}
}

void World::generate_supercell(int sx, int sy, int sz) {
	if (supercells.size() != static_cast<size_t>(dims.supercells)) supercells.resize(dims.supercells);
	std::vector<float> heights(kColumnSpan * kColumnSpan);
	column_heights(sx, sy, heights.data());
	build_supercell(sx, sy, sz, heights.data());
}

void World::generate(int threads) {
	supercells.clear();
	supercells.resize(dims.supercells);
	const int columns = dims.supergrid_xy * dims.supergrid_xy;
	parallel_for(columns, threads, [&](int c) {
		std::vector<float> heights(kColumnSpan * kColumnSpan);
		const int sx = c % dims.supergrid_xy, sy = c / dims.supergrid_xy;
		column_heights(sx, sy, heights.data());
		for (int sz = 0; sz < dims.supergrid_z; ++sz) build_supercell(sx, sy, sz, heights.data());
	});
	generated = true;
}

uint64_t World::total_bricks() const {
	uint64_t n = 0;
	for (const auto& c : supercells) n += c.bricks.size() - c.free_slots.size();
	return n;
}

// ---------------------------------------------------------------- dense voxels -> bricks
void World::load_supercell(const WorldDims& dims, HostSupercell& cell, int sx, int sy, int sz, const uint8_t* voxels) {
	cell = HostSupercell{};
	cell.indices.assign(kCellsPerSupercell, 0u);
	const size_t g = static_cast<size_t>(dims.grid_size);
	for (int bz = 0; bz < kSupercell; ++bz)
		for (int by = 0; by < kSupercell; ++by)
			for (int bx = 0; bx < kSupercell; ++bx) { // ascending local cell index: the generator's loop order
				const uint8_t* origin = voxels + (static_cast<size_t>(sz * kColumnSpan + bz * kBrickSize) * g + (sy * kColumnSpan + by * kBrickSize)) * g +
										sx * kColumnSpan + bx * kBrickSize;
				Brick brick;
				uint32_t any = 0;
				for (int w = 0; w < kBrickWords; ++w) { // word w = the x-rows (y = 4 (w & 1) ... + 3, z = w >> 1): byte (y + 8 z) of the brick
					uint32_t word = 0;
					for (int k = 0; k < 4; ++k) {
						uint32_t lo, hi;
						const uint8_t* row = origin + (static_cast<size_t>(w >> 1) * g + (4 * (w & 1) + k)) * g;
						std::memcpy(&lo, row, 4);
						std::memcpy(&hi, row + 4, 4);
						word |= brick_row_bits(lo, hi) << (8 * k);
					}
					brick.data[w] = word;
					any |= word;
				}
				if (!any) continue;
				cell.bricks.push_back(brick);
				cell.indices[bx + by * kSupercell + bz * kSupercell * kSupercell] =
					static_cast<uint32_t>(cell.bricks.size() - 1) | BM_BRICK_LOADED_BIT | (brick_lod(brick) << 12); // Scene.cpp:104
			}
}

void World::load_voxels(const uint8_t* voxels, int threads) {
	supercells.clear();
	supercells.resize(dims.supercells);
	parallel_for(dims.supercells, threads, [&](int sc) {
		int sx, sy, sz;
		dims.supercell_coords(sc, &sx, &sy, &sz);
		load_supercell(dims, supercells[sc], sx, sy, sz, voxels);
	});
	generated = true;
}

void World::store_voxels(uint8_t* voxels, int threads) const {
	const size_t g = static_cast<size_t>(dims.grid_size);
	parallel_for(dims.supercells, threads, [&](int sc) {
		const HostSupercell& c = supercells[sc];
		int sx, sy, sz;
		dims.supercell_coords(sc, &sx, &sy, &sz);
		for (int cell = 0; cell < kCellsPerSupercell; ++cell) {
			const uint32_t word = c.indices.empty() ? 0u : c.indices[cell];
			const uint8_t* bits = word ? reinterpret_cast<const uint8_t*>(c.bricks[word & BM_BRICK_INDEX_BITS].data) : nullptr;
			uint8_t* origin = voxels + (static_cast<size_t>(sz * kColumnSpan + (cell >> 8) * kBrickSize) * g + (sy * kColumnSpan + ((cell >> 4) & 15) * kBrickSize)) * g +
							  sx * kColumnSpan + (cell & 15) * kBrickSize;
			for (int r = 0; r < 64; ++r) { // x-row (y = r & 7, z = r >> 3) is byte r of the brick
				uint8_t* row = origin + (static_cast<size_t>(r >> 3) * g + (r & 7)) * g;
				for (int x = 0; x < kBrickSize; ++x) row[x] = bits ? (bits[r] >> x) & 1 : 0;
			}
		}
	});
}

// ---------------------------------------------------------------- voxel edits
namespace {
// bit positions of the 2x2x2 LoD octant q (bit 0: x >= 4, bit 1: y >= 4, bit 2: z >= 4) in a brick's 16 words (bit = x + 8y + 64z)
struct LodMasks {
	uint32_t m[8][kBrickWords] = {};
	LodMasks() {
		for (int bit = 0; bit < 512; ++bit) {
			const int x = bit & 7, y = (bit >> 3) & 7, z = bit >> 6;
			m[((x & 4) >> 2) + ((y & 4) >> 1) + (z & 4)][bit >> 5] |= 1u << (bit & 31);
		}
	}
};
const LodMasks kLodMasks;

inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
} // namespace

uint32_t World::brick_lod(const Brick& b) {
	uint32_t lod = 0;
	for (int q = 0; q < 8; ++q) {
		uint32_t any = 0;
		for (int w = 0; w < kBrickWords; ++w) any |= b.data[w] & kLodMasks.m[q][w];
		if (any) lod |= 1u << q;
	}
	return lod;
}

bool World::validate_edits(const bm_edit* edits, int count, std::string* why) {
	if (count < 0 || (count > 0 && !edits)) { *why = "bad edit count or null edit list"; return false; }
	for (int i = 0; i < count; ++i) {
		const bm_edit& e = edits[i];
		const std::string at = "edit " + std::to_string(i) + ": ";
		if (e.op != BM_EDIT_SET && e.op != BM_EDIT_CLEAR) { *why = at + "unknown op"; return false; }
		if (e.shape == BM_EDIT_BOX) {
			for (int k = 0; k < 3; ++k)
				if (e.hi[k] < e.lo[k]) { *why = at + "box with hi < lo"; return false; }
		} else if (e.shape == BM_EDIT_SPHERE) {
			if (e.radius < 0) { *why = at + "sphere with a negative radius"; return false; }
		} else {
			*why = at + "unknown shape";
			return false;
		}
	}
	return true;
}

bool World::edit_bounds(const WorldDims& dims, const bm_edit& e, int lo[3], int hi[3]) {
	const int64_t size[3] = {dims.grid_size, dims.grid_size, dims.grid_height};
	for (int k = 0; k < 3; ++k) {
		int64_t a, b; // half-open, 64-bit: centre +- radius may leave the int32 range
		if (e.shape == BM_EDIT_BOX) { a = e.lo[k]; b = e.hi[k]; }
		else { a = static_cast<int64_t>(e.center[k]) - e.radius; b = static_cast<int64_t>(e.center[k]) + e.radius + 1; }
		a = clamp64(a, 0, size[k]);
		b = clamp64(b, 0, size[k]);
		if (a >= b) return false;
		lo[k] = static_cast<int>(a);
		hi[k] = static_cast<int>(b);
	}
	return true;
}

void World::edit_supercell(const WorldDims& dims, HostSupercell& c, int sx, int sy, int sz, const bm_edit* edits, int count, uint8_t* touched) {
	const int org[3] = {sx * kColumnSpan, sy * kColumnSpan, sz * kColumnSpan}; // voxel origin of the supercell
	for (int i = 0; i < count; ++i) {
		const bm_edit& e = edits[i];
		int lo[3], hi[3];
		if (!edit_bounds(dims, e, lo, hi)) continue;
		bool inside = true;
		for (int k = 0; k < 3; ++k) {
			lo[k] = std::max(lo[k], org[k]) - org[k];
			hi[k] = std::min(hi[k], org[k] + kColumnSpan) - org[k];
			inside = inside && lo[k] < hi[k];
		}
		if (!inside) continue;
		const bool sphere = e.shape == BM_EDIT_SPHERE;
		const __int128 r2 = static_cast<__int128>(e.radius) * e.radius;
		for (int bz = lo[2] >> 3; bz <= (hi[2] - 1) >> 3; ++bz)
			for (int by = lo[1] >> 3; by <= (hi[1] - 1) >> 3; ++by)
				for (int bx = lo[0] >> 3; bx <= (hi[0] - 1) >> 3; ++bx) {
					const int local = bx + by * kSupercell + bz * kSupercell * kSupercell;
					uint32_t& word = c.indices[local];
					if (e.op == BM_EDIT_CLEAR && word == 0) continue; // nothing to clear
					// the edit's voxels in this brick (bit = x + 8y + 64z, Scene.cpp:91-93)
					uint32_t mask[kBrickWords] = {};
					bool any = false;
					const int x0 = std::max(lo[0], bx * 8), x1 = std::min(hi[0], bx * 8 + 8);
					const int y0 = std::max(lo[1], by * 8), y1 = std::min(hi[1], by * 8 + 8);
					const int z0 = std::max(lo[2], bz * 8), z1 = std::min(hi[2], bz * 8 + 8);
					for (int z = z0; z < z1; ++z)
						for (int y = y0; y < y1; ++y)
							for (int x = x0; x < x1; ++x) {
								if (sphere) { // sum of squares in 64-bit integers (wider where a far-away centre would overflow them)
									const __int128 dx = static_cast<int64_t>(org[0] + x) - e.center[0], dy = static_cast<int64_t>(org[1] + y) - e.center[1],
												   dz = static_cast<int64_t>(org[2] + z) - e.center[2];
									if (dx * dx + dy * dy + dz * dz > r2) continue;
								}
								const int bit = (x & 7) + (y & 7) * 8 + (z & 7) * 64;
								mask[bit >> 5] |= 1u << (bit & 31);
								any = true;
							}
					if (!any) continue;
					if (touched) touched[local] = 1;
					if (e.op == BM_EDIT_SET) {
						if (word == 0) { // the cell gains a brick: a freed slot first, else a new one
							uint32_t slot;
							if (!c.free_slots.empty()) {
								slot = c.free_slots.back();
								c.free_slots.pop_back();
							} else {
								slot = static_cast<uint32_t>(c.bricks.size());
								c.bricks.emplace_back();
							}
							std::memset(c.bricks[slot].data, 0, sizeof(Brick));
							word = slot | BM_BRICK_LOADED_BIT;
						}
						Brick& b = c.bricks[word & BM_BRICK_INDEX_BITS];
						for (int w = 0; w < kBrickWords; ++w) b.data[w] |= mask[w];
						word = (word & BM_BRICK_INDEX_BITS) | BM_BRICK_LOADED_BIT | (brick_lod(b) << 12); // Scene.cpp:104
					} else {
						const uint32_t slot = word & BM_BRICK_INDEX_BITS;
						Brick& b = c.bricks[slot];
						uint32_t left = 0;
						for (int w = 0; w < kBrickWords; ++w) left |= (b.data[w] &= ~mask[w]);
						if (left == 0) { // empty brick: word 0, slot free
							c.free_slots.push_back(slot);
							word = 0;
						} else {
							word = slot | BM_BRICK_LOADED_BIT | (brick_lod(b) << 12);
						}
					}
				}
	}
}

// ---------------------------------------------------------------- dense regions
bool World::validate_region(bm_region* r, std::string* why, uint64_t* span) {
	int64_t n[3];
	for (int k = 0; k < 3; ++k) {
		if (r->hi[k] < r->lo[k]) { *why = "region with hi < lo"; return false; }
		n[k] = static_cast<int64_t>(r->hi[k]) - r->lo[k];
	}
	if (r->row_pitch == 0) r->row_pitch = n[0];
	if (r->row_pitch < n[0]) { *why = "row_pitch is smaller than the row it spans (hi.x - lo.x bytes)"; return false; }
	const __int128 slice = static_cast<__int128>(r->row_pitch) * n[1];
	if (slice > INT64_MAX) { *why = "region too large"; return false; }
	if (r->slice_pitch == 0) r->slice_pitch = static_cast<int64_t>(slice);
	if (r->slice_pitch < static_cast<int64_t>(slice)) { *why = "slice_pitch is smaller than the slice it spans (row_pitch * (hi.y - lo.y) bytes)"; return false; }
	*span = 0;
	if (n[0] == 0 || n[1] == 0 || n[2] == 0) return true;
	const __int128 bytes = static_cast<__int128>(n[2] - 1) * r->slice_pitch + static_cast<__int128>(n[1] - 1) * r->row_pitch + n[0];
	if (bytes > INT64_MAX) { *why = "region too large"; return false; }
	*span = static_cast<uint64_t>(bytes);
	return true;
}

bool World::region_bounds(const WorldDims& dims, const bm_region& r, int lo[3], int hi[3]) {
	bm_edit e{};
	e.shape = BM_EDIT_BOX;
	for (int k = 0; k < 3; ++k) { e.lo[k] = r.lo[k]; e.hi[k] = r.hi[k]; }
	return edit_bounds(dims, e, lo, hi);
}

namespace {
// (vol & cover) of the brick cell whose first voxel is world voxel cell0, for the box [lo, hi) (world voxels); cover = the box's voxels in the cell
void region_cell_bits(const World::RegionSource& src, const int cell0[3], const int lo[3], const int hi[3], Brick* vol, Brick* cover) {
	const int x0 = std::max(lo[0] - cell0[0], 0), x1 = std::min(hi[0] - cell0[0], kBrickSize);
	const uint32_t xmask = ((1u << (x1 - x0)) - 1u) << x0;
	uint8_t* vb = reinterpret_cast<uint8_t*>(vol->data);
	uint8_t* cb = reinterpret_cast<uint8_t*>(cover->data);
	const uint8_t* packed = nullptr;
	if (src.packed) {
		const size_t at = (static_cast<size_t>((cell0[2] >> 3) - src.c0[2]) * src.nc[1] + ((cell0[1] >> 3) - src.c0[1])) * src.nc[0] + ((cell0[0] >> 3) - src.c0[0]);
		packed = reinterpret_cast<const uint8_t*>(src.packed[at].data);
	}
	for (int r = 0; r < 64; ++r) { // x-row (y = r & 7, z = r >> 3) is byte r of the brick
		const int y = cell0[1] + (r & 7), z = cell0[2] + (r >> 3);
		const bool in = y >= lo[1] && y < hi[1] && z >= lo[2] && z < hi[2];
		cb[r] = in ? static_cast<uint8_t>(xmask) : 0;
		if (!in) { vb[r] = 0; continue; }
		if (packed) { vb[r] = packed[r] & static_cast<uint8_t>(xmask); continue; }
		uint8_t row[8] = {};
		const uint8_t* from = src.voxels + (static_cast<int64_t>(z) - src.origin[2]) * src.slice_pitch + (static_cast<int64_t>(y) - src.origin[1]) * src.row_pitch +
							  (static_cast<int64_t>(cell0[0]) - src.origin[0]);
		std::memcpy(row + x0, from + x0, static_cast<size_t>(x1 - x0));
		uint32_t a, b;
		std::memcpy(&a, row, 4);
		std::memcpy(&b, row + 4, 4);
		vb[r] = static_cast<uint8_t>(brick_row_bits(a, b));
	}
}
} // namespace

void World::write_region_supercell(const WorldDims&, HostSupercell& c, int sx, int sy, int sz, const int lo_w[3], const int hi_w[3], int op, const RegionSource& src,
								   uint8_t* touched) {
	const int org[3] = {sx * kColumnSpan, sy * kColumnSpan, sz * kColumnSpan};
	int lo[3], hi[3]; // the box inside this supercell, world voxels
	for (int k = 0; k < 3; ++k) {
		lo[k] = std::max(lo_w[k], org[k]);
		hi[k] = std::min(hi_w[k], org[k] + kColumnSpan);
		if (lo[k] >= hi[k]) return;
	}
	for (int bz = (lo[2] - org[2]) >> 3; bz <= (hi[2] - 1 - org[2]) >> 3; ++bz)
		for (int by = (lo[1] - org[1]) >> 3; by <= (hi[1] - 1 - org[1]) >> 3; ++by)
			for (int bx = (lo[0] - org[0]) >> 3; bx <= (hi[0] - 1 - org[0]) >> 3; ++bx) { // ascending local cell index
				const int local = bx + by * kSupercell + bz * kSupercell * kSupercell;
				uint32_t& word = c.indices[local];
				const int cell0[3] = {org[0] + bx * 8, org[1] + by * 8, org[2] + bz * 8};
				Brick vol, cover, fresh;
				region_cell_bits(src, cell0, lo, hi, &vol, &cover);
				const Brick* old = word ? &c.bricks[word & BM_BRICK_INDEX_BITS] : nullptr;
				uint32_t differs = 0, any = 0;
				for (int w = 0; w < kBrickWords; ++w) {
					const uint32_t o = old ? old->data[w] : 0u;
					const uint32_t n = op == BM_REGION_REPLACE ? (o & ~cover.data[w]) | vol.data[w] : op == BM_EDIT_SET ? o | vol.data[w] : o & ~vol.data[w];
					fresh.data[w] = n;
					differs |= n ^ o;
					any |= n;
				}
				if (!differs) continue; // not touched: word, brick, slot and device state stay as they are
				if (touched) touched[local] = 1;
				if (!any) { // the brick became empty: word 0, slot free
					c.free_slots.push_back(word & BM_BRICK_INDEX_BITS);
					word = 0;
					continue;
				}
				uint32_t slot = word & BM_BRICK_INDEX_BITS;
				if (word == 0) { // the cell gains a brick: a freed slot first, else a new one
					if (!c.free_slots.empty()) {
						slot = c.free_slots.back();
						c.free_slots.pop_back();
					} else {
						slot = static_cast<uint32_t>(c.bricks.size());
						c.bricks.emplace_back();
					}
				}
				c.bricks[slot] = fresh;
				word = slot | BM_BRICK_LOADED_BIT | (brick_lod(fresh) << 12); // Scene.cpp:104
			}
}

void World::store_region(const int lo[3], const int hi[3], const int origin[3], uint8_t* voxels, int64_t row_pitch, int64_t slice_pitch, int threads) const {
	const int nz = hi[2] - lo[2];
	parallel_for(nz, threads, [&](int iz) {
		const int z = lo[2] + iz;
		for (int y = lo[1]; y < hi[1]; ++y) {
			uint8_t* row = voxels + (static_cast<int64_t>(z) - origin[2]) * slice_pitch + (static_cast<int64_t>(y) - origin[1]) * row_pitch - origin[0]; // row[x] = world voxel x
			for (int cx = lo[0] >> 3; cx <= (hi[0] - 1) >> 3; ++cx) {
				const HostSupercell& c = supercells[dims.supercell_id(cx / kSupercell, (y >> 3) / kSupercell, (z >> 3) / kSupercell)];
				const uint32_t word = c.indices.empty() ? 0u : c.indices[cell_local_index(cx, y >> 3, z >> 3)];
				const uint32_t bits = word ? reinterpret_cast<const uint8_t*>(c.bricks[word & BM_BRICK_INDEX_BITS].data)[(y & 7) + 8 * (z & 7)] : 0u;
				uint32_t a, b;
				brick_row_bytes(bits, &a, &b);
				uint8_t bytes[8];
				std::memcpy(bytes, &a, 4);
				std::memcpy(bytes + 4, &b, 4);
				const int x0 = std::max(lo[0], cx * 8), x1 = std::min(hi[0], cx * 8 + 8);
				std::memcpy(row + x0, bytes + (x0 - cx * 8), static_cast<size_t>(x1 - x0));
			}
		}
	});
}

// Largest empty cube per cell and octant: the classic "maximal square" recurrence in 3-D.  A cube of edge n anchored at
// c exists iff c is empty and cubes of edge n - 1 are anchored at the 7 neighbours c + {0,1}^3 * dir, so
// E(c) = 1 + min over those neighbours, swept from the far end of the octant's direction.  The border reads as 0
// during the sweep (a cube never leaves the grid) and is stamped 255 afterwards.
void World::build_cube_field(std::vector<uint8_t>& field, int threads) const {
	const int X = dims.cells + 2, Z = dims.cells_height + 2;
	const size_t plane = static_cast<size_t>(X) * X * Z;
	field.assign(plane * 8, 0);
	std::vector<uint8_t> occupied(plane, 1); // border counts as occupied
	for (int sc = 0; sc < dims.supercells; ++sc) {
		const HostSupercell& c = supercells[sc];
		int sx, sy, sz;
		dims.supercell_coords(sc, &sx, &sy, &sz);
		for (int lz = 0; lz < kSupercell; ++lz)
			for (int ly = 0; ly < kSupercell; ++ly) {
				uint8_t* row = &occupied[(static_cast<size_t>(sz * kSupercell + lz + 1) * X + (sy * kSupercell + ly + 1)) * X + sx * kSupercell + 1];
				const uint32_t* words = c.indices.empty() ? nullptr : &c.indices[ly * kSupercell + lz * kSupercell * kSupercell];
				for (int lx = 0; lx < kSupercell; ++lx) row[lx] = words && words[lx] ? 1 : 0;
			}
	}
	auto sweep = [&](int oct) {
		uint8_t* f = field.data() + plane * oct;
		const int dx = (oct & 1) ? -1 : 1, dy = (oct & 2) ? -1 : 1, dz = (oct & 4) ? -1 : 1;
		const ptrdiff_t ox = dx, oy = static_cast<ptrdiff_t>(dy) * X, oz = static_cast<ptrdiff_t>(dz) * X * X;
		for (int iz = 0; iz < dims.cells_height; ++iz) {
			const int z = dz > 0 ? dims.cells_height - iz : iz + 1; // bordered coordinate, far end first
			for (int iy = 0; iy < dims.cells; ++iy) {
				const int y = dy > 0 ? dims.cells - iy : iy + 1;
				const size_t row = (static_cast<size_t>(z) * X + y) * X;
				for (int ix = 0; ix < dims.cells; ++ix) {
					const int x = dx > 0 ? dims.cells - ix : ix + 1;
					const size_t i = row + x;
					if (occupied[i]) continue; // stays 0
					const uint8_t* n = f + i;
					uint8_t m = n[ox];
					m = std::min(m, n[oy]); m = std::min(m, n[ox + oy]);
					m = std::min(m, n[oz]); m = std::min(m, n[oz + ox]); m = std::min(m, n[oz + oy]); m = std::min(m, n[oz + oy + ox]);
					f[i] = static_cast<uint8_t>(std::min<int>(m, 253) + 1);
				}
			}
		}
		for (int z = 0; z < Z; ++z) // stamp the border
			for (int y = 0; y < X; ++y) {
				uint8_t* row = f + (static_cast<size_t>(z) * X + y) * X;
				if (z == 0 || z == Z - 1 || y == 0 || y == X - 1) std::memset(row, 255, X);
				else row[0] = row[X - 1] = 255;
			}
	};
	parallel_for(8, std::min(threads, 8), sweep);
}

} // namespace bm
