// distance_host.cpp -- bm_host_distance_field and bm_host_distance_mask: the distance field of host memory by the rules of distance.h, as
// plain loops: every row forwards and backwards for the nearest source along x, then every line along y and every line along z through
// the envelope of distance.h with its stack in a vector, then the minimum with the volume's border and the record.
// Needs nothing else of the library (no HIP header, no scene): tests/distance_check.cpp links this file alone.
#include <string>
#include <vector>

#include "../../include/brickmap.h"
#include "distance.h"

namespace bm {
// the library's error slot (error.h, defined in scene.cpp); absent -- a null address -- in a program that links this file alone
__attribute__((weak)) void set_error(const std::string& msg);
} // namespace bm

namespace {

int refuse(const char* who, const char* why) {
	if (bm::set_error) bm::set_error(std::string(who) + ": " + why);
	return BM_EINVAL;
}

// the envelope of the n values at in[0], in[stride], ... -> out at the same places
void line_pass(const uint32_t* in, uint32_t* out, size_t stride, uint32_t n, std::vector<uint32_t>& stack) {
	using namespace bm;
	auto f_at = [&](uint32_t j) { return in[j * stride]; };
	auto load_entry = [&](uint32_t k) { return stack[k]; };
	auto store_entry = [&](uint32_t k, uint32_t e) { stack[k] = e; };
	LineTop top = {0u, 0u, 0u, 0u};
	for (uint32_t u = 0; u < n; ++u)
		if (f_at(u) != kDistanceNone) distance_line_push(top, u, f_at(u), n, load_entry, store_entry, f_at);
	for (uint32_t u = n; u-- > 0;) out[u * stride] = distance_line_emit(top, u, load_entry, f_at);
}

} // namespace

extern "C" int bm_host_distance_field(const bm_distance_params* params, const uint8_t* volume, uint32_t* dist, bm_distance_result* result) {
	using namespace bm;
	static_assert(sizeof(bm_distance_result) == sizeof(DistanceRecord) && sizeof(bm_distance_result) == 32 && sizeof(bm_distance_params) == 40, "the records' sizes");
	const char* who = "bm_host_distance_field";
	if (!params) return refuse(who, "null params");
	const DistanceParamsView pv = distance_params_view(*params);
	if (const char* why = distance_params_problem(pv)) return refuse(who, why);
	if (!volume || !dist || !result) return refuse(who, "null volume, field or result");
	const DistanceDims d = distance_dims(pv);
	const int32_t nx = d.extent[0], ny = d.extent[1], nz = d.extent[2];
	const size_t row = static_cast<size_t>(nx), slice = row * static_cast<size_t>(ny);
	uint64_t sources = 0;
	// x: the distance to the last source seen, from the left and then from the right
	for (int32_t z = 0; z < nz; ++z)
		for (int32_t y = 0; y < ny; ++y) {
			const uint8_t* v = volume + z * d.slice_pitch + y * d.row_pitch;
			uint32_t* f = dist + z * slice + y * row;
			int32_t last = -1;
			for (int32_t x = 0; x < nx; ++x) {
				if (distance_is_source(v[x], d.to_empty)) {
					last = x;
					++sources;
				}
				f[x] = last < 0 ? kDistanceNone : distance_sq(x - last);
			}
			last = -1;
			for (int32_t x = nx - 1; x >= 0; --x) {
				if (distance_is_source(v[x], d.to_empty)) last = x;
				if (last >= 0 && distance_sq(last - x) < f[x]) f[x] = distance_sq(last - x);
			}
		}
	// y and z: a line at a time, through a plane of its own so that no pass overwrites what it still reads
	std::vector<uint32_t> h(static_cast<size_t>(d.voxels)), stack(static_cast<size_t>(ny > nz ? ny : nz));
	for (int32_t z = 0; z < nz; ++z)
		for (int32_t x = 0; x < nx; ++x) line_pass(dist + z * slice + x, h.data() + z * slice + x, row, static_cast<uint32_t>(ny), stack);
	for (int32_t y = 0; y < ny; ++y)
		for (int32_t x = 0; x < nx; ++x) line_pass(h.data() + y * row + x, dist + y * row + x, slice, static_cast<uint32_t>(nz), stack);
	uint64_t key = 0;
	for (int32_t z = 0; z < nz; ++z)
		for (int32_t y = 0; y < ny; ++y)
			for (int32_t x = 0; x < nx; ++x) {
				const size_t i = z * slice + y * row + x;
				if (d.outside) {
					const uint32_t edge = distance_outside_sq(d.extent, x, y, z);
					if (edge < dist[i]) dist[i] = edge;
				}
				const uint64_t k = distance_max_key(dist[i], static_cast<uint32_t>(i));
				if (k > key) key = k;
			}
	const DistanceRecord rec = distance_record(key, sources);
	*result = {rec.sources, rec.max_sq, 0u, rec.max_at, 0u};
	return 0;
}

extern "C" int bm_host_distance_mask(uint64_t count, const uint32_t* dist, uint32_t limit_sq, uint32_t flags, uint8_t* volume_out) {
	using namespace bm;
	const char* who = "bm_host_distance_mask";
	if (count == 0 || count > static_cast<uint64_t>(kDistanceMaxVoxels)) return refuse(who, "a count of 0 or above 2^31 - 2");
	if (flags & ~kDistanceMaskAbove) return refuse(who, "unknown flag");
	if (!dist || !volume_out) return refuse(who, "null buffer");
	for (uint64_t i = 0; i < count; ++i) volume_out[i] = static_cast<uint8_t>(distance_mask_byte(dist[i], limit_sq, flags & kDistanceMaskAbove));
	return 0;
}
