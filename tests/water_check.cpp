// water_check.cpp -- a program with its own main that links csrc/water_host.cpp alone and runs what the kernels of csrc/water.hip do to a
// tile, lane by lane on the host, through the same functions of csrc/water.h (water_row_sweep, water_step, water_start, water_faces_of),
// against the plain priority flood of bm_host_water_field:
//   rows    : all 2^12 solid patterns of a 12-voxel row (two tiles) with a drain moving along it, open ends and a sea, by the round scheme;
//             and the row sweep alone over the pattern's low byte at several heights and halo values, against a voxel-by-voxel fixed point
//   snake   : the longest corridor that fits a tile -- rows joined at alternating ends, planes joined by one voxel -- along each of the
//             three axes, alone in an 8^3 volume, drained at its start; the sweeps it needs must stay below the bound
//   tiles   : 10^4 random tiles at random heights with random values of their own and random halos already taken, against a relaxation to
//             the fixed point voxel by voxel
//   volumes : the round scheme over the tiles of 40 random volumes, every tile reading each neighbour at random as it stood when the round
//             began or as already rewritten in it, against the flood; the rounds never exceed the cap
//   refused : the parameter refusals of the host routines
// Prints "name count" pairs; "failures 0" at the end says that everything agreed.  Built plain and with -fsanitize=address,undefined by
// tests/test_water_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <random>
#include <vector>

#include "../brickmap_amd/csrc/water.h"
#include "../include/brickmap.h"

using namespace bm;

namespace {

int failures = 0;
int most_sweeps = 0;
#define EXPECT(cond)                                                          \
	do {                                                                      \
		if (!(cond)) {                                                        \
			if (++failures <= 10) std::printf("line %d: %s\n", __LINE__, #cond); \
		}                                                                     \
	} while (0)

struct Volume {
	int32_t nx, ny, nz;
	std::vector<uint8_t> bytes;
	uint8_t& at(int x, int y, int z) { return bytes[(static_cast<size_t>(z) * ny + y) * nx + x]; }
};

Volume make_volume(int nx, int ny, int nz, uint8_t fill) { return {nx, ny, nz, std::vector<uint8_t>(static_cast<size_t>(nx) * ny * nz, fill)}; }

bm_water_params params_of(const Volume& v, uint32_t faces, uint32_t sea) {
	bm_water_params p{};
	p.extent[0] = v.nx;
	p.extent[1] = v.ny;
	p.extent[2] = v.nz;
	p.sea_level = sea;
	p.flags = faces;
	return p;
}

// the tile's rows as the 64 lanes of a wave hold them; lane r's row lies at height z0 + (r >> 3)
struct Tile {
	uint32_t t[64][8];
	uint32_t open[64];
	uint32_t z0;
};

// what water_relax does between its loads and its stores: the sweeps, synchronous over the lanes.  Returns the sweeps that ran.
int settle(Tile& tile) {
	int sweeps = 0;
	for (int sweep = 0; sweep < kTravelTileSweeps; ++sweep) {
		++sweeps;
		uint32_t near[64][8];
		for (int r = 0; r < 64; ++r) {
			const int src[4] = {r - 1, r + 1, r - 8, r + 8};
			const bool have[4] = {(r & 7) != 0, (r & 7) != 7, (r >> 3) != 0, (r >> 3) != 7};
			for (int i = 0; i < 8; ++i) {
				near[r][i] = kWaterNone;
				for (int k = 0; k < 4; ++k)
					if (have[k]) near[r][i] = std::min(near[r][i], tile.t[src[k]][i]);
			}
		}
		bool any = false;
		for (int r = 0; r < 64; ++r) any = water_row_sweep(tile.t[r], tile.open[r], near[r], tile.z0 + (r >> 3)) || any;
		if (!any) break;
	}
	most_sweeps = std::max(most_sweeps, sweeps);
	return sweeps;
}

// ---- the round scheme, as launch_water_setup / water_drain / water_relax run it, over host memory
struct Rounds {
	std::vector<uint32_t> field;
	uint32_t rounds = 0, refalls = 0; // refalls: visits of a tile in which a value fell, after an earlier visit in which one fell
};

Rounds run_rounds(Volume& v, const std::vector<int32_t>& drains, uint32_t faces, uint32_t sea, std::mt19937& rng, bool stale) {
	const TravelDims d = water_dims(water_params_view(params_of(v, faces, sea)));
	Rounds out;
	out.field.assign(d.voxels, kWaterNone);
	std::vector<uint32_t>& field = out.field;
	std::vector<uint32_t> stamps(d.tile_count, 0u), fallen(d.tile_count, 0u), list, next;
	auto solid = [&](uint32_t x, uint32_t y, uint32_t z) {
		return x >= static_cast<uint32_t>(v.nx) || y >= static_cast<uint32_t>(v.ny) || z >= static_cast<uint32_t>(v.nz) || v.at(x, y, z) != 0;
	};
	auto list_tile = [&](std::vector<uint32_t>& l, uint32_t tile, uint32_t round) {
		const uint32_t old = stamps[tile];
		stamps[tile] = std::max(old, round);
		if (old < round) l.push_back(tile);
	};
	// setup: the outlets on the open faces
	for (int32_t z = 0; z < v.nz; ++z)
		for (int32_t y = 0; y < v.ny; ++y)
			for (int32_t x = 0; x < v.nx; ++x)
				if (v.at(x, y, z) == 0 && (water_faces_of(d.extent, x, y, z) & faces) != 0) {
					field[travel_voxel_index(d, x, y, z)] = water_start(z, sea);
					list_tile(list, travel_tile_index(d, x >> 3, y >> 3, z >> 3), 1u);
				}
	for (size_t s = 0; s + 2 < drains.size(); s += 3) {
		const int32_t x = drains[s], y = drains[s + 1], z = drains[s + 2];
		if (x < 0 || y < 0 || z < 0 || x >= v.nx || y >= v.ny || z >= v.nz || v.at(x, y, z) != 0) continue;
		field[travel_voxel_index(d, x, y, z)] = water_start(z, sea);
		list_tile(list, travel_tile_index(d, x >> 3, y >> 3, z >> 3), 1u);
	}
	const uint64_t cap = static_cast<uint64_t>(d.voxels) + 2;
	for (uint32_t round = 1; !list.empty(); ++round) {
		if (round > cap) {
			EXPECT(!"the rounds end");
			break;
		}
		out.rounds = round;
		next.clear();
		std::shuffle(list.begin(), list.end(), rng);
		const std::vector<uint32_t> before = field; // the field as the round found it
		for (const uint32_t id : list) {
			const uint32_t q = id / d.tiles[0], tx = id - q * d.tiles[0], ty = q % d.tiles[1], tz = q / d.tiles[1];
			// a halo value: as the round found it or as it stands now, at random per voxel
			auto halo = [&](uint32_t index) { return stale && (rng() & 1u) ? before[index] : field[index]; };
			Tile tile;
			tile.z0 = tz * 8;
			uint32_t was[64][8];
			const uint32_t nx = v.nx, ny = v.ny, nz = v.nz, slice = nx * ny;
			for (uint32_t r = 0; r < 64; ++r) {
				const uint32_t x0 = tx * 8, y = ty * 8 + (r & 7), z = tz * 8 + (r >> 3);
				uint32_t open = 0;
				for (uint32_t i = 0; i < 8; ++i)
					if (!solid(x0 + i, y, z)) open |= 1u << i;
				tile.open[r] = open;
				const uint32_t base = open ? travel_voxel_index(d, x0, y, z) : 0u;
				uint32_t* t = tile.t[r];
				for (uint32_t i = 0; i < 8; ++i) {
					t[i] = ((open >> i) & 1u) ? field[base + i] : kWaterNone;
					was[r][i] = round == 1u ? kWaterNone : t[i];
				}
				if ((open & 1u) && x0 > 0) t[0] = water_step(t[0], halo(base - 1), z, true);
				if ((open & 0x80u) && x0 + 8u < nx) t[7] = water_step(t[7], halo(base + 8), z, true);
				for (uint32_t i = 0; i < 8; ++i) {
					if (!((open >> i) & 1u)) continue;
					if ((r & 7) == 0 && y > 0) t[i] = water_step(t[i], halo(base - nx + i), z, true);
					if ((r & 7) == 7 && y + 1 < ny) t[i] = water_step(t[i], halo(base + nx + i), z, true);
					if ((r >> 3) == 0 && z > 0) t[i] = water_step(t[i], halo(base - slice + i), z, true);
					if ((r >> 3) == 7 && z + 1 < nz) t[i] = water_step(t[i], halo(base + slice + i), z, true);
				}
			}
			EXPECT(settle(tile) < kTravelTileSweeps);
			bool faces_fell[6] = {false, false, false, false, false, false}, any_fell = false;
			for (uint32_t r = 0; r < 64; ++r) {
				const uint32_t base = tile.open[r] ? travel_voxel_index(d, tx * 8, ty * 8 + (r & 7), tz * 8 + (r >> 3)) : 0u;
				bool fell = false;
				for (uint32_t i = 0; i < 8; ++i)
					if (tile.t[r][i] < was[r][i]) {
						EXPECT(tile.t[r][i] <= field[base + i] && (round == 1 || tile.t[r][i] < field[base + i])); // a value only ever falls
						EXPECT(tile.t[r][i] >= tz * 8 + (r >> 3));                                                  // and never below its voxel
						field[base + i] = tile.t[r][i];
						fell = true;
					}
				any_fell = any_fell || fell;
				faces_fell[0] = faces_fell[0] || (tile.t[r][0] < was[r][0] && tx > 0);
				faces_fell[1] = faces_fell[1] || (tile.t[r][7] < was[r][7] && tx + 1 < d.tiles[0]);
				faces_fell[2] = faces_fell[2] || (fell && (r & 7) == 0 && ty > 0);
				faces_fell[3] = faces_fell[3] || (fell && (r & 7) == 7 && ty + 1 < d.tiles[1]);
				faces_fell[4] = faces_fell[4] || (fell && (r >> 3) == 0 && tz > 0);
				faces_fell[5] = faces_fell[5] || (fell && (r >> 3) == 7 && tz + 1 < d.tiles[2]);
			}
			if (any_fell && fallen[id]++ != 0) ++out.refalls;
			const uint32_t step[3] = {1u, d.tiles[0], d.tiles[0] * d.tiles[1]};
			for (int f = 0; f < 6; ++f)
				if (faces_fell[f]) list_tile(next, (f & 1) ? id + step[f >> 1] : id - step[f >> 1], round + 1);
		}
		EXPECT(next.size() <= d.tile_count);
		list.swap(next);
	}
	return out;
}

// the rounds against the host routine; returns the host's record
bm_water_result compare(Volume& v, const std::vector<int32_t>& drains, uint32_t faces, uint32_t sea, std::mt19937& rng, bool stale, Rounds* rounds = nullptr) {
	const bm_water_params p = params_of(v, faces, sea);
	std::vector<uint32_t> want(v.bytes.size());
	bm_water_result rec{};
	EXPECT(bm_host_water_field(&p, v.bytes.data(), drains.empty() ? nullptr : drains.data(), static_cast<int64_t>(drains.size() / 3), want.data(), &rec) == 0);
	Rounds got = run_rounds(v, drains, faces, sea, rng, stale);
	EXPECT(got.field == want);
	// the mask against the field, plainly
	std::vector<uint8_t> mask(v.bytes.size(), 9);
	EXPECT(bm_host_water_mask(p.extent, want.data(), 2, mask.data()) == 0);
	uint64_t wet = 0;
	for (size_t i = 0; i < want.size(); ++i) {
		const uint32_t z = static_cast<uint32_t>(i / (static_cast<size_t>(v.nx) * v.ny));
		EXPECT(mask[i] == (want[i] != kWaterNone && want[i] >= z + 2 ? 1 : 0));
		wet += want[i] != kWaterNone && want[i] > z ? 1 : 0;
	}
	EXPECT(wet == rec.wet);
	if (rounds) *rounds = std::move(got);
	return rec;
}

// A corridor without a branch that winds through a whole tile.  Rows along axis a; in the planes 0, 2, 4, 6 of axis c the rows 0, 2, 4, 6
// of axis b are free and joined at alternating ends by one voxel of the rows 1, 3, 5; the planes are joined by one voxel, by turns at row 6
// and at row 0, where the walk of a plane ends.  35 voxels a plane and three joints: 143 voxels, the start at the origin.
Volume snake(int a, int b, int c) {
	Volume v = make_volume(8, 8, 8, 1);
	auto open = [&](int ia, int ib, int ic) {
		int p[3];
		p[a] = ia;
		p[b] = ib;
		p[c] = ic;
		v.at(p[0], p[1], p[2]) = 0;
	};
	for (int w = 0; w < 8; w += 2) {
		for (int row = 0; row < 8; row += 2)
			for (int i = 0; i < 8; ++i) open(i, row, w);
		open(7, 1, w);
		open(0, 3, w);
		open(7, 5, w);
		if (w + 2 < 8) open(0, (w / 2) % 2 == 0 ? 6 : 0, w + 1);
	}
	return v;
}

} // namespace

int main() {
	std::mt19937 rng(12345);
	// ---- rows
	int rows = 0;
	const uint32_t heights[4] = {0u, 5u, 100u, 16383u}, halos[6] = {kWaterNone, 0u, 4u, 5u, 7u, 16383u};
	for (uint32_t pattern = 0; pattern < 4096; ++pattern) {
		Volume v = make_volume(12, 1, 1, 0);
		for (int i = 0; i < 12; ++i) v.bytes[i] = (pattern >> i) & 1u ? 200 : 0;
		compare(v, {static_cast<int32_t>(pattern % 12), 0, 0}, (pattern / 12) % 4, pattern % 5 == 0 ? 1 : 0, rng, true);
		// the sweep of one row alone: own values and the rows beside it at random, against a fixed point voxel by voxel
		const uint32_t open = ~pattern & 0xFFu, z = heights[(pattern >> 8) % 4];
		uint32_t t[8], near[8], want[8];
		for (int i = 0; i < 8; ++i) {
			near[i] = halos[rng() % 6];
			t[i] = ((open >> i) & 1u) && rng() % 4 == 0 ? std::max(z, halos[1 + rng() % 5]) : kWaterNone;
			want[i] = ((open >> i) & 1u) ? water_step(t[i], near[i], z, true) : t[i];
			EXPECT(water_step(t[i], near[i], z, false) == t[i]);
		}
		for (bool again = true; again;) {
			again = false;
			for (int i = 0; i < 8; ++i)
				for (const int k : {i - 1, i + 1})
					if (k >= 0 && k < 8 && ((open >> i) & 1u) && std::max(want[k], z) < want[i]) {
						want[i] = std::max(want[k], z);
						again = true;
					}
		}
		water_row_sweep(t, open, near, z);
		EXPECT(std::memcmp(t, want, sizeof t) == 0);
		EXPECT(!water_row_sweep(t, open, near, z)); // one sweep settles a row against constant neighbours
		++rows;
	}
	std::printf("rows %d\n", rows);
	// ---- the snake
	int snakes = 0, snake_sweeps = 0;
	const int axes[3][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}};
	for (const auto& ax : axes) {
		Volume v = snake(ax[0], ax[1], ax[2]);
		const int before = most_sweeps;
		most_sweeps = 0;
		const bm_water_result rec = compare(v, {0, 0, 0}, 0, 0, rng, false);
		snake_sweeps = std::max(snake_sweeps, most_sweeps);
		most_sweeps = std::max(most_sweeps, before);
		EXPECT(rec.closed == 0 && rec.drains_rejected == 0); // one corridor: the drain reaches all of it
		++snakes;
	}
	std::printf("snake %d snake_sweeps %d\n", snakes, snake_sweeps);
	// ---- random tiles with random halos: the sweeps against a relaxation to the fixed point
	int tiles = 0;
	for (int n = 0; n < 10000; ++n) {
		const uint32_t density = rng() % 5, z0 = 8 * (rng() % 4);
		Tile tile;
		tile.z0 = z0;
		std::vector<uint32_t> want(512);
		std::vector<bool> open(512);
		for (int r = 0; r < 64; ++r) {
			tile.open[r] = 0;
			for (int i = 0; i < 8; ++i) {
				const bool o = rng() % 10 >= density * 2;
				if (o) tile.open[r] |= 1u << i;
				// a value of its own, or a halo value already taken: either way a start of the relaxation, and never below the voxel
				const uint32_t roll = rng() % 16, value = roll == 0 ? std::max<uint32_t>(z0 + (r >> 3), rng() % 40) : kWaterNone;
				tile.t[r][i] = o ? value : kWaterNone;
				open[r * 8 + i] = o;
				want[r * 8 + i] = tile.t[r][i];
			}
		}
		for (bool again = true; again;) {
			again = false;
			for (int j = 0; j < 512; ++j) {
				if (!open[j]) continue;
				const int x = j & 7, y = (j >> 3) & 7, z = j >> 6;
				const int nb[6] = {x > 0 ? j - 1 : -1, x < 7 ? j + 1 : -1, y > 0 ? j - 8 : -1, y < 7 ? j + 8 : -1, z > 0 ? j - 64 : -1, z < 7 ? j + 64 : -1};
				for (const int k : nb)
					if (k >= 0 && want[k] != kWaterNone && std::max<uint32_t>(want[k], z0 + z) < want[j]) {
						want[j] = std::max<uint32_t>(want[k], z0 + z);
						again = true;
					}
			}
		}
		EXPECT(settle(tile) < kTravelTileSweeps);
		bool same = true;
		for (int r = 0; r < 64; ++r)
			for (int i = 0; i < 8; ++i) same = same && tile.t[r][i] == want[r * 8 + i];
		EXPECT(same);
		++tiles;
	}
	std::printf("tiles %d\n", tiles);
	// ---- the round scheme with stale halos
	int volumes = 0, rounds_over = 0;
	uint32_t refalls = 0;
	const uint32_t densities[4] = {35, 50, 60, 70};
	for (int n = 0; n < 40; ++n) {
		Volume v = make_volume(1 + rng() % 29, 1 + rng() % 29, 1 + rng() % 29, 0);
		for (auto& b : v.bytes) b = rng() % 100 < densities[n % 4] ? 1 + rng() % 255 : 0;
		std::vector<int32_t> drains;
		for (uint32_t s = 0, count = rng() % 4; s < count; ++s) {
			drains.push_back(static_cast<int32_t>(rng() % (v.nx + 2)) - 1);
			drains.push_back(static_cast<int32_t>(rng() % (v.ny + 2)) - 1);
			drains.push_back(static_cast<int32_t>(rng() % (v.nz + 2)) - 1);
		}
		const uint32_t faces = n % 5 == 0 ? 0u : n % 5 == 1 ? 1u << (rng() % 6) : n % 5 == 2 ? 63u : 15u;
		const uint32_t sea = n % 3 == 0 ? rng() % (v.nz + 1) : 0u;
		Rounds got;
		compare(v, drains, faces, sea, rng, true, &got);
		if (got.rounds > static_cast<uint64_t>(v.bytes.size()) + 2) ++rounds_over;
		refalls += got.refalls;
		++volumes;
	}
	std::printf("volumes %d rounds_over %d refalls %u\n", volumes, rounds_over, refalls);
	// ---- refusals
	int refused = 0;
	{
		uint8_t vol[8] = {0}, mask[8];
		uint32_t field[8];
		int32_t drains[3] = {0, 0, 0};
		bm_water_result rec{};
		auto bad = [&](bm_water_params p, const uint8_t* v, const int32_t* s, int64_t n, uint32_t* f, bm_water_result* r) {
			if (bm_host_water_field(&p, v, s, n, f, r) == BM_EINVAL) ++refused;
		};
		bm_water_params ok{};
		ok.extent[0] = 2;
		ok.extent[1] = 2;
		ok.extent[2] = 2;
		ok.flags = 15;
		bm_water_params p = ok;
		p.extent[0] = 0; bad(p, vol, drains, 1, field, &rec);
		p = ok; p.extent[2] = 16385; bad(p, vol, drains, 1, field, &rec);
		p = ok; p.row_pitch = 1; bad(p, vol, drains, 1, field, &rec);
		p = ok; p.slice_pitch = 3; bad(p, vol, drains, 1, field, &rec);
		p = ok; p.flags = 64; bad(p, vol, drains, 1, field, &rec);
		p = ok; p.reserved = 1; bad(p, vol, drains, 1, field, &rec);
		p = ok; p.sea_level = 3; bad(p, vol, drains, 1, field, &rec);
		bad(ok, nullptr, drains, 1, field, &rec);
		bad(ok, vol, nullptr, 1, field, &rec);
		bad(ok, vol, drains, -1, field, &rec);
		bad(ok, vol, drains, 1, nullptr, &rec);
		bad(ok, vol, drains, 1, field, nullptr);
		p = ok; p.sea_level = 2;
		EXPECT(bm_host_water_field(&p, vol, drains, 1, field, &rec) == 0 && rec.wet == 8 && rec.deepest == 2 && rec.deepest_at == 0 && rec.closed == 0);
		if (bm_host_water_mask(ok.extent, field, 0, mask) == BM_EINVAL) ++refused;
		if (bm_host_water_mask(ok.extent, nullptr, 1, mask) == BM_EINVAL) ++refused;
		EXPECT(bm_host_water_mask(ok.extent, field, 2, mask) == 0 && mask[0] == 1 && mask[7] == 0);
	}
	std::printf("refused %d\n", refused);
	std::printf("most_sweeps %d\n", most_sweeps);
	std::printf("failures %d\n", failures);
	return failures == 0 ? 0 : 1;
}
