// travel_host.cpp -- bm_host_travel_field and bm_host_travel_paths: the travel field of host memory by the rules of travel.h, as plain
// loops: the accepted seeds are the first front, and every front hands its open neighbours that hold no value yet to the next one -- a
// breadth-first search, no tiles and no rounds -- then one pass for the record; a path is the walk of travel.h.
// Needs nothing else of the library (no HIP header, no scene): tests/travel_check.cpp links this file alone.
#include <string>
#include <vector>

#include "../../include/brickmap.h"
#include "travel.h"

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

extern "C" int bm_host_travel_field(const bm_travel_params* params, const uint8_t* volume, const int32_t* seeds, int64_t n, uint32_t* field, bm_travel_result* result) {
	using namespace bm;
	static_assert(sizeof(bm_travel_result) == sizeof(TravelRecord) && sizeof(bm_travel_result) == 32 && sizeof(bm_travel_params) == 40, "the records' sizes");
	static_assert(BM_TRAVEL_NONE == kTravelNone, "none");
	const char* who = "bm_host_travel_field";
	if (!params) return refuse(who, "null params");
	const TravelParamsView pv = travel_params_view(*params);
	if (const char* why = travel_params_problem(pv)) return refuse(who, why);
	if (n < 0) return refuse(who, "a negative number of seeds");
	if (!volume || !field || !result || (n > 0 && !seeds)) return refuse(who, "null volume, seeds, field or result");
	const TravelDims d = travel_dims(pv);
	const int32_t nx = d.extent[0], ny = d.extent[1], nz = d.extent[2];
	const size_t row = static_cast<size_t>(nx), slice = row * static_cast<size_t>(ny);
	auto blocked = [&](int32_t x, int32_t y, int32_t z) { return volume[z * d.slice_pitch + y * d.row_pitch + x] != 0; };
	for (size_t i = 0; i < d.voxels; ++i) field[i] = kTravelNone;
	std::vector<uint32_t> front, next;
	uint32_t rejected = 0;
	for (int64_t s = 0; s < n; ++s) {
		const int32_t x = seeds[3 * s], y = seeds[3 * s + 1], z = seeds[3 * s + 2];
		if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz || blocked(x, y, z)) {
			++rejected;
			continue;
		}
		const size_t i = z * slice + y * row + x;
		if (field[i] != 0) front.push_back(static_cast<uint32_t>(i));
		field[i] = 0;
	}
	for (uint32_t level = 1; !front.empty() && level <= d.limit; ++level) {
		next.clear();
		for (const uint32_t i : front) {
			const int32_t z = static_cast<int32_t>(i / slice), y = static_cast<int32_t>((i - z * slice) / row), x = static_cast<int32_t>(i - z * slice - y * row);
			for (int f = 0; f < 6; ++f) {
				int32_t q[3] = {x, y, z};
				q[f >> 1] += (f & 1) ? 1 : -1;
				if (q[f >> 1] < 0 || q[f >> 1] >= d.extent[f >> 1] || blocked(q[0], q[1], q[2])) continue;
				const size_t j = q[2] * slice + q[1] * row + q[0];
				if (field[j] != kTravelNone) continue;
				field[j] = level;
				next.push_back(static_cast<uint32_t>(j));
			}
		}
		front.swap(next);
	}
	uint64_t key = 0, reached = 0;
	for (size_t i = 0; i < d.voxels; ++i) {
		if (field[i] != kTravelNone) ++reached;
		const uint64_t k = travel_max_key(field[i], static_cast<uint32_t>(i));
		if (k > key) key = k;
	}
	const TravelRecord rec = travel_record(key, reached, rejected);
	*result = {rec.reached, rec.farthest, rec.seeds_rejected, rec.farthest_at, 0u};
	return 0;
}

extern "C" int bm_host_travel_paths(const int32_t extent[3], const uint32_t* field, const int32_t* starts, int64_t n, int32_t capacity, int32_t* path, int32_t* lengths) {
	using namespace bm;
	const char* who = "bm_host_travel_paths";
	if (!extent) return refuse(who, "null extent");
	if (const char* why = travel_extent_problem(extent)) return refuse(who, why);
	if (n < 0) return refuse(who, "a negative number of starts");
	if (capacity < 1) return refuse(who, "a capacity below 1");
	if (!field || (n > 0 && (!starts || !path || !lengths))) return refuse(who, "null field, starts, path or lengths");
	const size_t row = static_cast<size_t>(extent[0]), slice = row * static_cast<size_t>(extent[1]);
	for (int64_t q = 0; q < n; ++q) {
		int32_t* out = path + static_cast<size_t>(q) * static_cast<size_t>(capacity) * 3;
		lengths[q] = travel_walk(
			extent, starts[3 * q], starts[3 * q + 1], starts[3 * q + 2], capacity, [&](int32_t x, int32_t y, int32_t z) { return field[z * slice + y * row + x]; },
			[&](int32_t k, int32_t x, int32_t y, int32_t z) {
				out[3 * k] = x;
				out[3 * k + 1] = y;
				out[3 * k + 2] = z;
			});
	}
	return 0;
}
