// foot_host.cpp -- bm_host_foot_room, bm_host_foot_field and bm_host_foot_paths: ground navigation on host memory by the rules of foot.h,
// as plain loops: every column is walked downwards for the room bytes; the accepted seeds are the head of one queue, and every stand taken
// from it hands its legal targets that hold no value yet to the queue's end -- a breadth-first search, no levels and no rounds -- then one
// pass for the record; a path is the walk of foot.h.
// Needs nothing else of the library (no HIP header, no scene): tests/foot_check.cpp links this file alone.
#include <string>
#include <vector>

#include "../../include/brickmap.h"
#include "foot.h"

namespace bm {
// the library's error slot (error.h, defined in scene.cpp); absent -- a null address -- in a program that links this file alone
__attribute__((weak)) void set_error(const std::string& msg);
} // namespace bm

namespace {

int refuse(const char* who, const char* why) {
	if (bm::set_error) bm::set_error(std::string(who) + ": " + why);
	return BM_EINVAL;
}

} // namespace

extern "C" int bm_host_foot_room(const bm_foot_params* params, const uint8_t* volume, uint8_t* room) {
	using namespace bm;
	static_assert(sizeof(bm_foot_params) == sizeof(bm_travel_params) + 16 && sizeof(bm_foot_params) == 56, "the params' size");
	static_assert(BM_FOOT_NONE == kFootNone && BM_FOOT_TOWARD == kFootToward && BM_FOOT_NO_FLOOR == kFootNoFloor, "the constants");
	const char* who = "bm_host_foot_room";
	if (!params) return refuse(who, "null params");
	const FootParamsView pv = foot_params_view(*params);
	if (const char* why = foot_params_problem(pv)) return refuse(who, why);
	if (!volume || !room) return refuse(who, "null volume or room");
	const FootDims d = foot_dims(pv);
	const int32_t nx = d.extent[0], ny = d.extent[1], nz = d.extent[2];
	for (int32_t y = 0; y < ny; ++y)
		for (int32_t x = 0; x < nx; ++x) {
			auto blocked = [&](int32_t z) { return volume[z * d.slice_pitch + y * d.row_pitch + x] != 0; };
			uint32_t run = kFootRoomCap;
			for (int32_t z = nz - 1; z >= 0; --z) {
				run = foot_room_run(run, blocked(z));
				room[foot_voxel_index(d, x, y, z)] = static_cast<uint8_t>(foot_room_byte(run, z > 0 ? blocked(z - 1) : d.floor != 0));
			}
		}
	return 0;
}

extern "C" int bm_host_foot_field(const bm_foot_params* params, const uint8_t* room, const int32_t* seeds, int64_t n, uint32_t* field, bm_foot_result* result) {
	using namespace bm;
	static_assert(sizeof(bm_foot_result) == sizeof(FootRecord) && sizeof(bm_foot_result) == 32, "the record's size");
	const char* who = "bm_host_foot_field";
	if (!params) return refuse(who, "null params");
	const FootParamsView pv = foot_params_view(*params);
	if (const char* why = foot_params_problem(pv)) return refuse(who, why);
	if (n < 0) return refuse(who, "a negative number of seeds");
	if (!room || !field || !result || (n > 0 && !seeds)) return refuse(who, "null room, seeds, field or result");
	const FootDims d = foot_dims(pv);
	uint64_t standable = 0;
	for (size_t i = 0; i < d.voxels; ++i) {
		field[i] = kFootNone;
		if (foot_stand(room[i], d.height)) ++standable;
	}
	std::vector<uint32_t> queue;
	uint32_t rejected = 0;
	for (int64_t s = 0; s < n; ++s) {
		const int32_t x = seeds[3 * s], y = seeds[3 * s + 1], z = seeds[3 * s + 2];
		if (x < 0 || y < 0 || z < 0 || x >= d.extent[0] || y >= d.extent[1] || z >= d.extent[2] || !foot_stand(room[foot_voxel_index(d, x, y, z)], d.height)) {
			++rejected;
			continue;
		}
		const uint32_t i = foot_voxel_index(d, x, y, z);
		if (field[i] != 0) queue.push_back(i);
		field[i] = 0;
	}
	for (size_t head = 0; head < queue.size(); ++head) { // every stand enters once: bounded by their number
		const uint32_t p = queue[head], level = field[p] + 1u;
		if (level > d.limit) break; // the queue is in ascending value
		for (int dir = 0; dir < 4; ++dir)
			foot_expand(d, p, dir, [&](uint32_t i) { return static_cast<uint32_t>(room[i]); },
						[&](uint32_t q) {
							if (field[q] != kFootNone) return;
							field[q] = level;
							queue.push_back(q);
						});
	}
	uint64_t key = 0;
	for (const uint32_t i : queue) {
		const uint64_t k = foot_max_key(field[i], i);
		if (k > key) key = k;
	}
	const FootRecord rec = foot_record(key, queue.size(), rejected, standable);
	*result = {rec.reached, rec.farthest, rec.seeds_rejected, rec.farthest_at, rec.standable};
	return 0;
}

extern "C" int bm_host_foot_paths(const bm_foot_params* params, const uint8_t* room, const uint32_t* field, const int32_t* starts, int64_t n, int32_t capacity, int32_t* path,
								  int32_t* lengths) {
	using namespace bm;
	const char* who = "bm_host_foot_paths";
	if (!params) return refuse(who, "null params");
	const FootParamsView pv = foot_params_view(*params);
	if (const char* why = foot_params_problem(pv)) return refuse(who, why);
	if (n < 0) return refuse(who, "a negative number of starts");
	if (capacity < 1) return refuse(who, "a capacity below 1");
	if (!room || !field || (n > 0 && (!starts || !path || !lengths))) return refuse(who, "null room, field, starts, path or lengths");
	const FootDims d = foot_dims(pv);
	for (int64_t q = 0; q < n; ++q) {
		int32_t* out = path + static_cast<size_t>(q) * static_cast<size_t>(capacity) * 3;
		lengths[q] = foot_walk(
			d, starts[3 * q], starts[3 * q + 1], starts[3 * q + 2], capacity, [&](uint32_t i) { return field[i]; }, [&](uint32_t i) { return static_cast<uint32_t>(room[i]); },
			[&](int32_t k, int32_t x, int32_t y, int32_t z) {
				out[3 * k] = x;
				out[3 * k + 1] = y;
				out[3 * k + 2] = z;
			});
	}
	return 0;
}
