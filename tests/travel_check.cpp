// travel_check.cpp -- a program with its own main that links csrc/travel_host.cpp alone and runs what the kernels of csrc/travel.hip do
// to a tile, lane by lane on the host, through the same functions of csrc/travel.h (travel_row_sweep, travel_take), against the plain
// breadth-first search of bm_host_travel_field:
//   rows    : all 2^12 blocked patterns of a 12-voxel row (two tiles), the seed moving along it, by the round scheme
//   snake   : the longest corridor that fits a tile -- rows joined at alternating ends, slices joined by one voxel -- along each of the
//             three axes, alone in an 8^3 volume; the sweeps it needs are the most a tile can ask for and must stay below the bound
//   tiles   : 10^4 random tiles with random values of their own and random halos, against a relaxation to the fixed point voxel by voxel
//   volumes : the round scheme over the tiles of 40 random volumes, every tile reading each neighbour at random as it stood when the round
//             began or as already rewritten in it, against the plain search; the rounds never exceed farthest + 2
//   refused : the parameter refusals of the host routines
// Prints "name count" pairs; "failures 0" at the end says that everything agreed.  Built plain and with -fsanitize=address,undefined by
// tests/test_travel_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../brickmap_amd/csrc/travel.h"
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

bm_travel_params params_of(const Volume& v, uint32_t max_steps) {
	bm_travel_params p{};
	p.extent[0] = v.nx;
	p.extent[1] = v.ny;
	p.extent[2] = v.nz;
	p.max_steps = max_steps;
	return p;
}

// the tile's rows as the 64 lanes of a wave hold them
struct Tile {
	uint32_t t[64][8];
	uint32_t open[64];
};

// what travel_relax does between its loads and its stores: the sweeps, synchronous over the lanes.  Returns the sweeps that ran.
int settle(Tile& tile, uint32_t limit) {
	int sweeps = 0;
	for (int sweep = 0; sweep < kTravelTileSweeps; ++sweep) {
		++sweeps;
		uint32_t near[64][8];
		for (int r = 0; r < 64; ++r) {
			const int src[4] = {r - 1, r + 1, r - 8, r + 8};
			const bool have[4] = {(r & 7) != 0, (r & 7) != 7, (r >> 3) != 0, (r >> 3) != 7};
			for (int i = 0; i < 8; ++i) {
				near[r][i] = kTravelNone;
				for (int k = 0; k < 4; ++k)
					if (have[k]) near[r][i] = std::min(near[r][i], tile.t[src[k]][i]);
			}
		}
		bool any = false;
		for (int r = 0; r < 64; ++r) any = travel_row_sweep(tile.t[r], tile.open[r], near[r], limit) || any;
		if (!any) break;
	}
	most_sweeps = std::max(most_sweeps, sweeps);
	return sweeps;
}

// ---- the round scheme, as launch_travel_setup / travel_seed / travel_relax run it, over host memory
struct Rounds {
	std::vector<uint32_t> field;
	uint32_t rounds = 0;
};

Rounds run_rounds(Volume& v, const std::vector<int32_t>& seeds, uint32_t max_steps, std::mt19937& rng, bool stale) {
	const TravelDims d = travel_dims(travel_params_view(params_of(v, max_steps)));
	Rounds out;
	out.field.assign(d.voxels, kTravelNone);
	std::vector<uint32_t>& field = out.field;
	std::vector<uint32_t> stamps(d.tile_count, 0u), list, next;
	auto blocked = [&](uint32_t x, uint32_t y, uint32_t z) {
		return x >= static_cast<uint32_t>(v.nx) || y >= static_cast<uint32_t>(v.ny) || z >= static_cast<uint32_t>(v.nz) || v.at(x, y, z) != 0;
	};
	auto list_tile = [&](std::vector<uint32_t>& l, uint32_t tile, uint32_t round) {
		const uint32_t old = stamps[tile];
		stamps[tile] = std::max(old, round);
		if (old < round) l.push_back(tile);
	};
	for (size_t s = 0; s + 2 < seeds.size(); s += 3) {
		const int32_t x = seeds[s], y = seeds[s + 1], z = seeds[s + 2];
		if (x < 0 || y < 0 || z < 0 || x >= v.nx || y >= v.ny || z >= v.nz || v.at(x, y, z) != 0) continue;
		field[travel_voxel_index(d, x, y, z)] = 0;
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
			uint32_t was[64][8];
			const uint32_t nx = v.nx, ny = v.ny, nz = v.nz, slice = nx * ny;
			for (uint32_t r = 0; r < 64; ++r) {
				const uint32_t x0 = tx * 8, y = ty * 8 + (r & 7), z = tz * 8 + (r >> 3);
				uint32_t open = 0;
				for (uint32_t i = 0; i < 8; ++i)
					if (!blocked(x0 + i, y, z)) open |= 1u << i;
				tile.open[r] = open;
				const uint32_t base = open ? travel_voxel_index(d, x0, y, z) : 0u;
				uint32_t* t = tile.t[r];
				for (uint32_t i = 0; i < 8; ++i) {
					t[i] = ((open >> i) & 1u) ? field[base + i] : kTravelNone;
					was[r][i] = round == 1u && t[i] == 0u ? kTravelNone : t[i];
				}
				if ((open & 1u) && x0 > 0) t[0] = travel_take(t[0], halo(base - 1), true, d.limit);
				if ((open & 0x80u) && x0 + 8u < nx) t[7] = travel_take(t[7], halo(base + 8), true, d.limit);
				for (uint32_t i = 0; i < 8; ++i) {
					if (!((open >> i) & 1u)) continue;
					if ((r & 7) == 0 && y > 0) t[i] = travel_take(t[i], halo(base - nx + i), true, d.limit);
					if ((r & 7) == 7 && y + 1 < ny) t[i] = travel_take(t[i], halo(base + nx + i), true, d.limit);
					if ((r >> 3) == 0 && z > 0) t[i] = travel_take(t[i], halo(base - slice + i), true, d.limit);
					if ((r >> 3) == 7 && z + 1 < nz) t[i] = travel_take(t[i], halo(base + slice + i), true, d.limit);
				}
			}
			EXPECT(settle(tile, d.limit) < kTravelTileSweeps);
			bool faces[6] = {false, false, false, false, false, false};
			for (uint32_t r = 0; r < 64; ++r) {
				const uint32_t base = tile.open[r] ? travel_voxel_index(d, tx * 8, ty * 8 + (r & 7), tz * 8 + (r >> 3)) : 0u;
				bool fell = false;
				for (uint32_t i = 0; i < 8; ++i)
					if (tile.t[r][i] < was[r][i]) {
						EXPECT(tile.t[r][i] < field[base + i] || (round == 1 && tile.t[r][i] == 0)); // a value only ever falls
						field[base + i] = tile.t[r][i];
						fell = true;
					}
				faces[0] = faces[0] || (tile.t[r][0] < was[r][0] && tx > 0);
				faces[1] = faces[1] || (tile.t[r][7] < was[r][7] && tx + 1 < d.tiles[0]);
				faces[2] = faces[2] || (fell && (r & 7) == 0 && ty > 0);
				faces[3] = faces[3] || (fell && (r & 7) == 7 && ty + 1 < d.tiles[1]);
				faces[4] = faces[4] || (fell && (r >> 3) == 0 && tz > 0);
				faces[5] = faces[5] || (fell && (r >> 3) == 7 && tz + 1 < d.tiles[2]);
			}
			const uint32_t step[3] = {1u, d.tiles[0], d.tiles[0] * d.tiles[1]};
			for (int f = 0; f < 6; ++f)
				if (faces[f]) list_tile(next, (f & 1) ? id + step[f >> 1] : id - step[f >> 1], round + 1);
		}
		EXPECT(next.size() <= d.tile_count);
		list.swap(next);
	}
	return out;
}

// the rounds against the host routine; returns the host's record
bm_travel_result compare(Volume& v, const std::vector<int32_t>& seeds, uint32_t max_steps, std::mt19937& rng, bool stale, uint32_t* rounds = nullptr) {
	const bm_travel_params p = params_of(v, max_steps);
	std::vector<uint32_t> want(v.bytes.size());
	bm_travel_result rec{};
	EXPECT(bm_host_travel_field(&p, v.bytes.data(), seeds.empty() ? nullptr : seeds.data(), static_cast<int64_t>(seeds.size() / 3), want.data(), &rec) == 0);
	const Rounds got = run_rounds(v, seeds, max_steps, rng, stale);
	EXPECT(got.field == want);
	if (rounds) *rounds = got.rounds;
	return rec;
}

// A corridor without a branch that winds through a whole tile (a voxel grid has no path through all 512 voxels that is also a shortest
// one: the corridor needs its walls).  Rows along axis a; in the planes 0, 2, 4, 6 of axis c the rows 0, 2, 4, 6 of axis b are open and
// joined at alternating ends by one voxel of the rows 1, 3, 5; the planes are joined by one voxel, by turns at row 6 and at row 0, where
// the walk of a plane ends.  35 voxels a plane and three joints: 143 voxels, the start at the origin.
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
	for (uint32_t pattern = 0; pattern < 4096; ++pattern) {
		Volume v = make_volume(12, 1, 1, 0);
		for (int i = 0; i < 12; ++i) v.bytes[i] = (pattern >> i) & 1u ? 200 : 0;
		compare(v, {static_cast<int32_t>(pattern % 12), 0, 0}, pattern % 5 == 0 ? 3 : 0, rng, true);
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
		const bm_travel_result rec = compare(v, {0, 0, 0}, 0, rng, false);
		snake_sweeps = std::max(snake_sweeps, most_sweeps);
		most_sweeps = std::max(most_sweeps, before);
		EXPECT(rec.reached == 143 && rec.farthest == 142); // one corridor without a branch: its length is its voxel count
		++snakes;
	}
	std::printf("snake %d snake_sweeps %d\n", snakes, snake_sweeps);
	// ---- random tiles with random halos: the sweeps against a relaxation to the fixed point
	int tiles = 0;
	for (int n = 0; n < 10000; ++n) {
		const uint32_t density = rng() % 5, limit = (rng() & 1u) ? kTravelMaxSteps : 1u + rng() % 40;
		Tile tile;
		std::vector<uint32_t> want(512);
		std::vector<bool> open(512);
		for (int r = 0; r < 64; ++r) {
			tile.open[r] = 0;
			for (int i = 0; i < 8; ++i) {
				const bool o = rng() % 10 >= density * 2;
				if (o) tile.open[r] |= 1u << i;
				// a value of its own, or a halo value already taken: either way a start of the relaxation
				const uint32_t roll = rng() % 16, value = roll == 0 ? rng() % 30 : kTravelNone;
				tile.t[r][i] = o && value <= limit ? value : kTravelNone;
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
					if (k >= 0 && want[k] != kTravelNone && want[k] + 1 <= limit && want[k] + 1 < want[j]) {
						want[j] = want[k] + 1;
						again = true;
					}
			}
		}
		EXPECT(settle(tile, limit) < kTravelTileSweeps);
		bool same = true;
		for (int r = 0; r < 64; ++r)
			for (int i = 0; i < 8; ++i) same = same && tile.t[r][i] == want[r * 8 + i];
		EXPECT(same);
		++tiles;
	}
	std::printf("tiles %d\n", tiles);
	// ---- the round scheme with stale halos
	int volumes = 0, rounds_over = 0;
	const uint32_t limits[7] = {0, 1, 7, 8, 9, 20, 0};
	const uint32_t densities[4] = {0, 20, 30, 45};
	for (int n = 0; n < 40; ++n) {
		Volume v = make_volume(1 + rng() % 29, 1 + rng() % 29, 1 + rng() % 29, 0);
		for (auto& b : v.bytes) b = rng() % 100 < densities[n % 4] ? 1 + rng() % 255 : 0;
		std::vector<int32_t> seeds;
		for (uint32_t s = 0, count = rng() % 4; s < count; ++s) {
			seeds.push_back(static_cast<int32_t>(rng() % (v.nx + 2)) - 1);
			seeds.push_back(static_cast<int32_t>(rng() % (v.ny + 2)) - 1);
			seeds.push_back(static_cast<int32_t>(rng() % (v.nz + 2)) - 1);
		}
		uint32_t rounds = 0;
		const bm_travel_result rec = compare(v, seeds, limits[n % 7], rng, true, &rounds);
		if (rec.farthest != BM_TRAVEL_NONE && rounds > rec.farthest + 2) ++rounds_over;
		if (rec.farthest == BM_TRAVEL_NONE) EXPECT(rounds == 0);
		++volumes;
	}
	std::printf("volumes %d rounds_over %d\n", volumes, rounds_over);
	// ---- refusals
	int refused = 0;
	{
		uint8_t vol[8] = {0};
		uint32_t field[8];
		int32_t seeds[3] = {0, 0, 0}, path[6], lengths[1];
		bm_travel_result rec{};
		auto bad = [&](bm_travel_params p, const uint8_t* v, const int32_t* s, int64_t n, uint32_t* f, bm_travel_result* r) {
			if (bm_host_travel_field(&p, v, s, n, f, r) == BM_EINVAL) ++refused;
		};
		bm_travel_params ok{};
		ok.extent[0] = 2;
		ok.extent[1] = 2;
		ok.extent[2] = 2;
		bm_travel_params p = ok;
		p.extent[0] = 0; bad(p, vol, seeds, 1, field, &rec);
		p = ok; p.extent[2] = 16385; bad(p, vol, seeds, 1, field, &rec);
		p = ok; p.extent[0] = p.extent[1] = 16384; p.extent[2] = 8; bad(p, vol, seeds, 1, field, &rec);
		p = ok; p.row_pitch = 1; bad(p, vol, seeds, 1, field, &rec);
		p = ok; p.row_pitch = -2; bad(p, vol, seeds, 1, field, &rec);
		p = ok; p.slice_pitch = 3; bad(p, vol, seeds, 1, field, &rec);
		p = ok; p.flags = 1; bad(p, vol, seeds, 1, field, &rec);
		p = ok; p.reserved = 1; bad(p, vol, seeds, 1, field, &rec);
		bad(ok, nullptr, seeds, 1, field, &rec);
		bad(ok, vol, nullptr, 1, field, &rec);
		bad(ok, vol, seeds, -1, field, &rec);
		bad(ok, vol, seeds, 1, nullptr, &rec);
		bad(ok, vol, seeds, 1, field, nullptr);
		if (bm_host_travel_field(nullptr, vol, seeds, 1, field, &rec) == BM_EINVAL) ++refused;
		EXPECT(bm_host_travel_field(&ok, vol, seeds, 1, field, &rec) == 0 && rec.reached == 8 && rec.farthest == 3 && rec.farthest_at == 7);
		if (bm_host_travel_paths(ok.extent, field, seeds, 1, 0, path, lengths) == BM_EINVAL) ++refused;
		if (bm_host_travel_paths(ok.extent, nullptr, seeds, 1, 2, path, lengths) == BM_EINVAL) ++refused;
		EXPECT(bm_host_travel_paths(ok.extent, field, seeds, 1, 2, path, lengths) == 0 && lengths[0] == 1);
	}
	std::printf("refused %d\n", refused);
	std::printf("most_sweeps %d\n", most_sweeps);
	std::printf("failures %d\n", failures);
	return failures == 0 ? 0 : 1;
}
