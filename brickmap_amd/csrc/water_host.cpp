// water_host.cpp -- bm_host_water_field and bm_host_water_mask: the spill levels of host memory by the rules of water.h, as a plain
// priority flood: one bucket of voxels per height, the outlets first, and every voxel taken from the bucket of height h hands max(h, z)
// to its free neighbours that hold more -- no tiles and no rounds -- then one pass for the record.
// Needs nothing else of the library (no HIP header, no scene): tests/water_check.cpp links this file alone.
#include <string>
#include <vector>

#include "../../include/brickmap.h"
#include "water.h"

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

extern "C" int bm_host_water_field(const bm_water_params* params, const uint8_t* volume, const int32_t* drains, int64_t n, uint32_t* field, bm_water_result* result) {
	using namespace bm;
	static_assert(sizeof(bm_water_result) == sizeof(WaterRecord) && sizeof(bm_water_result) == 32 && sizeof(bm_water_params) == sizeof(bm_travel_params), "the records' sizes");
	static_assert(BM_WATER_NONE == kWaterNone, "none");
	const char* who = "bm_host_water_field";
	if (!params) return refuse(who, "null params");
	const TravelParamsView pv = water_params_view(*params);
	if (const char* why = water_params_problem(pv)) return refuse(who, why);
	if (n < 0) return refuse(who, "a negative number of drains");
	if (!volume || !field || !result || (n > 0 && !drains)) return refuse(who, "null volume, drains, field or result");
	const TravelDims d = water_dims(pv);
	const int32_t nx = d.extent[0], ny = d.extent[1], nz = d.extent[2];
	const uint32_t sea = params->sea_level, faces = params->flags & kWaterFaces;
	const size_t row = static_cast<size_t>(nx), slice = row * static_cast<size_t>(ny);
	auto solid = [&](int32_t x, int32_t y, int32_t z) { return volume[z * d.slice_pitch + y * d.row_pitch + x] != 0; };
	std::vector<std::vector<uint32_t>> bucket(static_cast<size_t>(nz) + 1); // a level is at most max(nz - 1, sea) <= nz
	auto outlet = [&](int32_t x, int32_t y, int32_t z) {
		const size_t i = z * slice + y * row + x;
		const uint32_t v = water_start(static_cast<uint32_t>(z), sea);
		if (field[i] == v) return;
		field[i] = v;
		bucket[v].push_back(static_cast<uint32_t>(i));
	};
	for (size_t i = 0; i < d.voxels; ++i) field[i] = kWaterNone;
	if (faces != 0)
		for (int32_t z = 0; z < nz; ++z)
			for (int32_t y = 0; y < ny; ++y)
				for (int32_t x = 0; x < nx; ++x)
					if ((water_faces_of(d.extent, x, y, z) & faces) != 0 && !solid(x, y, z)) outlet(x, y, z);
	uint32_t rejected = 0;
	for (int64_t s = 0; s < n; ++s) {
		const int32_t x = drains[3 * s], y = drains[3 * s + 1], z = drains[3 * s + 2];
		if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz || solid(x, y, z)) {
			++rejected;
			continue;
		}
		outlet(x, y, z);
	}
	for (uint32_t h = 0; h < bucket.size(); ++h) {
		std::vector<uint32_t>& todo = bucket[h];
		while (!todo.empty()) {
			const uint32_t i = todo.back();
			todo.pop_back();
			if (field[i] != h) continue; // (never: a voxel's first value is its least, see below)
			const int32_t z = static_cast<int32_t>(i / slice), y = static_cast<int32_t>((i - z * slice) / row), x = static_cast<int32_t>(i - z * slice - y * row);
			for (int f = 0; f < 6; ++f) {
				int32_t q[3] = {x, y, z};
				q[f >> 1] += (f & 1) ? 1 : -1;
				if (q[f >> 1] < 0 || q[f >> 1] >= d.extent[f >> 1] || solid(q[0], q[1], q[2])) continue;
				const size_t j = q[2] * slice + q[1] * row + q[0];
				// heights are taken in rising order and a candidate is at least h: whatever a voxel holds already is no larger
				const uint32_t c = water_step(field[j], h, static_cast<uint32_t>(q[2]), true);
				if (c == field[j]) continue;
				field[j] = c;
				bucket[c].push_back(static_cast<uint32_t>(j));
			}
		}
	}
	uint64_t key = 0, wet = 0, closed = 0;
	for (int32_t z = 0; z < nz; ++z)
		for (int32_t y = 0; y < ny; ++y)
			for (int32_t x = 0; x < nx; ++x) {
				const size_t i = z * slice + y * row + x;
				if (water_wet(field[i], static_cast<uint32_t>(z))) ++wet;
				if (field[i] == kWaterNone && !solid(x, y, z)) ++closed;
				const uint64_t k = water_depth_key(field[i], static_cast<uint32_t>(z), static_cast<uint32_t>(i));
				if (k > key) key = k;
			}
	const WaterRecord rec = water_record(key, wet, rejected, closed);
	*result = {rec.wet, rec.deepest, rec.drains_rejected, rec.deepest_at, rec.closed};
	return 0;
}

extern "C" int bm_host_water_mask(const int32_t extent[3], const uint32_t* field, uint32_t min_depth, uint8_t* mask) {
	using namespace bm;
	const char* who = "bm_host_water_mask";
	if (!extent) return refuse(who, "null extent");
	if (const char* why = travel_extent_problem(extent)) return refuse(who, why);
	if (min_depth < 1) return refuse(who, "a min_depth below 1");
	if (!field || !mask) return refuse(who, "null field or mask");
	const size_t slice = static_cast<size_t>(extent[0]) * static_cast<size_t>(extent[1]);
	for (int32_t z = 0; z < extent[2]; ++z)
		for (size_t i = 0; i < slice; ++i) mask[z * slice + i] = static_cast<uint8_t>(water_mask_byte(field[z * slice + i], static_cast<uint32_t>(z), min_depth));
	return 0;
}
