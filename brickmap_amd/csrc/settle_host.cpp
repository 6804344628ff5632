// settle_host.cpp -- bm_host_settle: rigid settling of host memory by the rules of settle.h, as plain loops: every column is walked
// upwards and its contacts relax the drops in place, again and again until a whole pass changes nothing -- no rounds, no groups -- then
// one pass scatters the voxels, and one over the records gives the drops and the sums.
// Needs nothing else of the library (no HIP header, no scene): tests/settle_check.cpp links this file alone.
#include <string>
#include <vector>

#include "../../include/brickmap.h"
#include "settle.h"

namespace bm {
// the library's error slot (error.h, defined in scene.cpp); absent -- a null address -- in a program that links this file alone
__attribute__((weak)) void set_error(const std::string& msg);
} // namespace bm

namespace {

int refuse(const char* why) {
	if (bm::set_error) bm::set_error(std::string("bm_host_settle: ") + why);
	return BM_EINVAL;
}

} // namespace

extern "C" int bm_host_settle(const int32_t extent[3], const int32_t* labels, const bm_component* comps, int64_t n, const uint8_t* chosen, uint8_t* out, int32_t* drops,
							  bm_settle_result* result) {
	using namespace bm;
	static_assert(sizeof(bm_settle_result) == sizeof(SettleRecord) && sizeof(bm_settle_result) == 32 && sizeof(bm_component) == kSettleRecordBytes, "the records' sizes");
	if (!extent) return refuse("null extent");
	if (const char* why = settle_extent_problem(extent)) return refuse(why);
	if (n < 0 || n > kSettleMaxVoxels) return refuse("a negative number of records, or more than 2^31 - 2");
	if (!labels || !out || !result || (n > 0 && (!comps || !chosen || !drops))) return refuse("null labels, records, chosen, out, drops or result");
	const SettleDims d = settle_dims(extent, n);
	auto moving = [&](int32_t label) {
		return settle_moving_slot([&](uint32_t slot) { return comps[slot].label; }, [&](uint32_t slot) { return chosen[slot]; }, d.n, label);
	};
	std::vector<uint32_t> drop(d.n);
	for (uint32_t s = 0; s < d.n; ++s) drop[s] = chosen[s] ? kSettleUnknown : 0u;
	uint64_t contacts = 0;
	bool first = true, changed = true;
	while (changed) { // every pass but the last lowers a drop, and a drop is a whole number that falls from at most nz: bounded
		changed = false;
		for (uint32_t col = 0; col < d.columns; ++col) {
			SettleBelow below = settle_floor();
			for (int32_t z = 0; z < d.nz; ++z) {
				const int32_t label = labels[static_cast<size_t>(z) * d.columns + col];
				SettleContact c;
				if (label == 0 || !settle_step(below, label, z, moving, c)) continue;
				if (first) ++contacts;
				const uint32_t cand = settle_candidate(c.lower >= 0 ? drop[c.lower] : 0u, c.gap);
				if (cand < drop[c.upper]) {
					drop[c.upper] = cand;
					changed = true;
				}
			}
		}
		first = false;
	}
	for (size_t i = 0; i < d.voxels; ++i) out[i] = 0;
	SettleRecord rec = {0, 0, 0, 0, 0, contacts};
	for (uint32_t col = 0; col < d.columns; ++col) {
		SettleBelow below = settle_floor();
		for (int32_t z = 0; z < d.nz; ++z) {
			const int32_t label = labels[static_cast<size_t>(z) * d.columns + col];
			if (label == 0) continue;
			SettleContact c;
			settle_step(below, label, z, moving, c);
			const uint32_t by = below.slot >= 0 ? settle_final_drop(drop[below.slot]) : 0u;
			if (by > static_cast<uint32_t>(z)) continue; // (never: settle.h)
			out[static_cast<size_t>(z - static_cast<int32_t>(by)) * d.columns + col] = static_cast<uint8_t>(settle_byte(by));
			if (by != 0) ++rec.moved_voxels;
		}
	}
	for (uint32_t s = 0; s < d.n; ++s) {
		const uint32_t by = chosen[s] ? settle_final_drop(drop[s]) : 0u;
		drops[s] = static_cast<int32_t>(by);
		if (chosen[s]) ++rec.chosen_pieces;
		if (by != 0) ++rec.moved_pieces;
		if (by > rec.largest_drop) rec.largest_drop = by;
	}
	*result = {rec.moved_voxels, rec.chosen_pieces, rec.moved_pieces, rec.largest_drop, 0u, rec.contacts};
	return 0;
}
