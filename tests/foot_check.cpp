// foot_check.cpp -- a program with its own main that links csrc/foot_host.cpp alone (no HIP, no library) and runs the level scheme of
// csrc/foot.hip on the host through the functions of csrc/foot.h: one queue, level k a segment of it, every pair (front node, direction)
// of a round handled in a random order, a target taking min(W, k) and being appended by whoever finds kFootNone there.  On 200 random
// volumes the field must equal bm_host_foot_field's, the rounds stay within farthest + 2, the queue within its bound, and every path
// of bm_host_foot_paths is a chain of legal moves down the field.  Built plain and with -fsanitize=address,undefined by
// tests/test_foot_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "../brickmap_amd/csrc/foot.h"
#include "../include/brickmap.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                   \
	do {                                                   \
		if (!(cond)) {                                     \
			if (++failures <= 20) {                        \
				std::printf("FAILED %s: ", #cond);         \
				std::printf(__VA_ARGS__);                  \
				std::printf("\n");                         \
			}                                              \
		}                                                  \
	} while (0)

struct Levels {
	std::vector<uint32_t> field;
	uint32_t rounds = 0, reached = 0;
};

// the device's scheme: rounds until the next front is empty (what the host loop of bm_foot_field looks at)
Levels run_levels(const bm::FootDims& d, const std::vector<uint8_t>& room, const std::vector<int32_t>& seeds, std::mt19937& rng) {
	using namespace bm;
	Levels out;
	out.field.assign(d.voxels, kFootNone);
	std::vector<uint32_t> queue;
	auto offer = [&](uint32_t q, uint32_t value) { // the atomic min and what its return decides
		const uint32_t old = out.field[q];
		out.field[q] = std::min(old, value);
		if (old == kFootNone) queue.push_back(q);
	};
	for (size_t s = 0; s < seeds.size() / 3; ++s) {
		const int32_t x = seeds[3 * s], y = seeds[3 * s + 1], z = seeds[3 * s + 2];
		if (x < 0 || y < 0 || z < 0 || x >= d.extent[0] || y >= d.extent[1] || z >= d.extent[2]) continue;
		const uint32_t i = foot_voxel_index(d, x, y, z);
		if (foot_stand(room[i], d.height)) offer(i, 0u);
	}
	size_t begin = 0, end = queue.size();
	while (end > begin) {
		const uint32_t round = ++out.rounds;
		if (round <= d.limit) {
			std::vector<std::pair<uint32_t, int>> pairs;
			for (size_t i = begin; i < end; ++i)
				for (int dir = 0; dir < 4; ++dir) pairs.push_back({queue[i], dir});
			std::shuffle(pairs.begin(), pairs.end(), rng);
			for (const auto& pr : pairs)
				foot_expand(d, pr.first, pr.second, [&](uint32_t i) { return static_cast<uint32_t>(room[i]); }, [&](uint32_t q) { offer(q, round); });
		}
		begin = end;
		end = queue.size();
	}
	CHECK(queue.size() <= d.queue, "%zu entries in a queue of %u", queue.size(), d.queue);
	out.reached = static_cast<uint32_t>(queue.size());
	return out;
}

} // namespace

int main() {
	using namespace bm;
	std::mt19937 rng(20261021u);
	auto pick = [&](int lo, int hi) { return static_cast<int>(rng() % static_cast<uint32_t>(hi - lo + 1)) + lo; };
	int volumes = 0, refused = 0;
	for (int run = 0; run < 200; ++run) {
		bm_foot_params p{};
		p.extent[0] = pick(1, 14);
		p.extent[1] = pick(1, 11);
		p.extent[2] = run % 17 == 0 ? pick(130, 150) : pick(1, 24);
		const int64_t row = p.extent[0] + (run % 3 == 0 ? pick(0, 5) : 0), slice = row * p.extent[1] + (run % 5 == 0 ? pick(0, 9) : 0);
		p.row_pitch = run % 2 ? row : (row == p.extent[0] ? 0 : row);
		p.slice_pitch = run % 2 ? slice : (slice == row * p.extent[1] ? 0 : slice);
		p.height = pick(1, 3);
		p.climb = pick(0, 3);
		p.drop = run % 7 == 0 ? pick(0, 64) : pick(0, 6);
		p.flags = (run % 2 ? BM_FOOT_TOWARD : 0u) | (run % 4 == 3 ? BM_FOOT_NO_FLOOR : 0u);
		p.max_steps = run % 6 == 5 ? static_cast<uint32_t>(pick(1, 12)) : 0u;
		const FootDims d = foot_dims(foot_params_view(p));
		const int density = pick(5, 45);
		std::vector<uint8_t> volume(static_cast<size_t>(slice) * p.extent[2], 0);
		for (auto& b : volume) b = pick(0, 99) < density ? static_cast<uint8_t>(pick(1, 255)) : 0;
		std::vector<uint8_t> room(d.voxels, 0xEE);
		CHECK(bm_host_foot_room(&p, volume.data(), room.data()) == 0, "run %d: the room is refused", run);
		// the room bytes against the definition, voxel by voxel
		for (int32_t z = 0; z < p.extent[2]; ++z)
			for (int32_t y = 0; y < p.extent[1]; ++y)
				for (int32_t x = 0; x < p.extent[0]; ++x) {
					auto blocked = [&](int32_t zz) { return volume[zz * slice + y * row + x] != 0; };
					uint32_t free = 0;
					int32_t zz = z;
					while (zz < p.extent[2] && !blocked(zz)) ++free, ++zz;
					if (zz == p.extent[2] && free > 0) free = 127;
					free = std::min(free, 127u);
					const bool below = z > 0 ? blocked(z - 1) : !(p.flags & BM_FOOT_NO_FLOOR);
					const uint32_t want = free | (free != 0 && below ? 0x80u : 0u);
					CHECK(room[foot_voxel_index(d, x, y, z)] == want, "run %d: room byte at %d,%d,%d is %u, not %u", run, x, y, z, room[foot_voxel_index(d, x, y, z)], want);
				}
		std::vector<int32_t> seeds;
		const int n = pick(0, 6);
		for (int s = 0; s < n; ++s) {
			seeds.push_back(pick(-1, p.extent[0]));
			seeds.push_back(pick(-1, p.extent[1]));
			seeds.push_back(pick(-1, p.extent[2]));
		}
		for (uint32_t i = 0; i < d.voxels && seeds.size() < 3 * static_cast<size_t>(n + 3); i += 1 + static_cast<uint32_t>(pick(0, 40))) // and some that are stands
			if (foot_stand(room[i], d.height)) {
				seeds.push_back(static_cast<int32_t>(i % static_cast<uint32_t>(p.extent[0])));
				seeds.push_back(static_cast<int32_t>(i % d.columns / static_cast<uint32_t>(p.extent[0])));
				seeds.push_back(static_cast<int32_t>(i / d.columns));
			}
		const int64_t count = static_cast<int64_t>(seeds.size() / 3);
		std::vector<uint32_t> field(d.voxels, 5u);
		bm_foot_result rec{};
		CHECK(bm_host_foot_field(&p, room.data(), count ? seeds.data() : nullptr, count, field.data(), &rec) == 0, "run %d: the field is refused", run);
		const Levels got = run_levels(d, room, seeds, rng);
		CHECK(got.field == field, "run %d: the level scheme's field is not the host routine's", run);
		CHECK(got.reached == rec.reached, "run %d: reached %u, the host routine %llu", run, got.reached, static_cast<unsigned long long>(rec.reached));
		const uint32_t farthest = rec.farthest == kFootNone ? 0u : rec.farthest;
		CHECK(got.rounds <= farthest + 2u, "run %d: %u rounds for a farthest value of %u", run, got.rounds, farthest);
		// every path is a chain of legal moves down the field
		const int32_t capacity = static_cast<int32_t>(farthest) + 1;
		std::vector<int32_t> path(static_cast<size_t>(count ? count : 1) * capacity * 3, -7), lengths(count ? count : 1, -7), starts(seeds);
		if (rec.reached > 0) { // the farthest voxel as the first start
			starts[0] = static_cast<int32_t>(rec.farthest_at % static_cast<uint32_t>(p.extent[0]));
			starts[1] = static_cast<int32_t>(rec.farthest_at % d.columns / static_cast<uint32_t>(p.extent[0]));
			starts[2] = static_cast<int32_t>(rec.farthest_at / d.columns);
		}
		CHECK(bm_host_foot_paths(&p, room.data(), field.data(), count ? starts.data() : nullptr, count, capacity, path.data(), lengths.data()) == 0, "run %d: the paths are refused", run);
		const bool toward = (p.flags & BM_FOOT_TOWARD) != 0;
		for (int64_t q = 0; q < count; ++q) {
			const int32_t* s = &starts[3 * q];
			const bool inside = s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && s[0] < p.extent[0] && s[1] < p.extent[1] && s[2] < p.extent[2];
			const uint32_t w = inside ? field[foot_voxel_index(d, s[0], s[1], s[2])] : kFootNone;
			CHECK(lengths[q] == (w == kFootNone ? 0 : static_cast<int32_t>(w) + 1), "run %d: path %lld has length %d for a value of %u", run, static_cast<long long>(q), lengths[q], w);
			const int32_t* v = &path[static_cast<size_t>(q) * capacity * 3];
			for (int32_t k = 1; k < lengths[q]; ++k) {
				const int32_t *a = v + 3 * (k - 1), *b = v + 3 * k; // a holds one more than b
				const uint32_t ra = room[foot_voxel_index(d, a[0], a[1], a[2])], rb = room[foot_voxel_index(d, b[0], b[1], b[2])];
				const int32_t dz = toward ? b[2] - a[2] : a[2] - b[2]; // the walk goes a -> b toward a seed, b -> a from one
				const bool side = (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) == 1;
				CHECK(side && dz <= p.climb && -dz <= p.drop && foot_move(toward ? ra : rb, toward ? rb : ra, dz, p.height), "run %d: path %lld, step %d is no legal move", run,
					  static_cast<long long>(q), k);
				CHECK(field[foot_voxel_index(d, b[0], b[1], b[2])] + 1u == field[foot_voxel_index(d, a[0], a[1], a[2])], "run %d: path %lld, step %d does not descend", run,
					  static_cast<long long>(q), k);
			}
		}
		++volumes;
	}
	// refusals of the host routines: nothing is written
	{
		bm_foot_params p{};
		p.extent[0] = p.extent[1] = p.extent[2] = 2;
		p.height = 2, p.climb = 1, p.drop = 3;
		uint8_t volume[8] = {0}, room[8];
		uint32_t field[8];
		std::fill(room, room + 8, 0xEE);
		std::fill(field, field + 8, 5u);
		bm_foot_result rec{};
		int32_t seed[3] = {0, 0, 0}, path[3], length = -7;
		auto bad = [&](bm_foot_params q) {
			const bool all = bm_host_foot_room(&q, volume, room) == BM_EINVAL && bm_host_foot_field(&q, room, seed, 1, field, &rec) == BM_EINVAL &&
							 bm_host_foot_paths(&q, room, field, seed, 1, 1, path, &length) == BM_EINVAL;
			CHECK(all, "params that should be refused pass");
			++refused;
		};
		bm_foot_params q = p;
		q.height = 0, bad(q), q.height = 33, bad(q), q = p;
		q.climb = -1, bad(q), q.climb = 33, bad(q), q = p;
		q.drop = -1, bad(q), q.drop = 65, bad(q), q = p;
		q.flags = 4u, bad(q), q = p;
		q.reserved = 1u, bad(q), q = p;
		q.reserved2 = 1, bad(q), q = p;
		q.extent[1] = 0, bad(q), q = p;
		q.row_pitch = 1, bad(q), q = p;
		CHECK(bm_host_foot_room(nullptr, volume, room) == BM_EINVAL && bm_host_foot_room(&p, nullptr, room) == BM_EINVAL && bm_host_foot_room(&p, volume, nullptr) == BM_EINVAL, "null");
		CHECK(bm_host_foot_field(&p, room, nullptr, 1, field, &rec) == BM_EINVAL && bm_host_foot_field(&p, room, seed, -1, field, &rec) == BM_EINVAL, "null seeds or n < 0");
		CHECK(bm_host_foot_paths(&p, room, field, seed, 1, 0, path, &length) == BM_EINVAL, "capacity 0");
		refused += 3;
		CHECK(std::all_of(room, room + 8, [](uint8_t b) { return b == 0xEE; }) && std::all_of(field, field + 8, [](uint32_t w) { return w == 5u; }) && length == -7,
			  "a refused call has written");
	}
	std::printf("volumes %d\nrefused %d\nfailures %d\n", volumes, refused, failures);
	return failures == 0 ? 0 : 1;
}
