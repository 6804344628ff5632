// settle_check.cpp -- a program with its own main that links csrc/settle_host.cpp alone and runs the round scheme of csrc/settle.hip on
// the host, through the same functions of csrc/settle.h (settle_step, settle_moving_slot, settle_candidate), against a plain relaxation
// of a list of contacts taken by loops of its own, and against bm_host_settle:
//   volumes : 200 random label volumes (pieces of scattered voxels, tables that miss labels, random choices).  A round walks every column;
//             each read of D sees at random the value the round began with or the one already lowered in it, the minimum is taken on the
//             live value and a change is counted by what the minimum returns.  The drops equal the plain relaxation's and the host
//             routine's, no two voxels land on one, and the rounds -- the one without a change included -- never exceed chosen + 2.
//   refused : the refusals of the host routine
// Prints "name count" pairs; "failures 0" at the end says that everything agreed.  Built plain and with -fsanitize=address,undefined by
// tests/test_settle_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../brickmap_amd/csrc/settle.h"
#include "../include/brickmap.h"

using namespace bm;

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
	do {                                                                      \
		if (!(cond)) {                                                        \
			if (++failures <= 10) std::printf("line %d: %s\n", __LINE__, #cond); \
		}                                                                     \
	} while (0)

struct Case {
	int32_t extent[3];
	std::vector<int32_t> labels;
	std::vector<bm_component> table;
	std::vector<uint8_t> chosen;
};

// the round scheme: returns the rounds that ran, the last of which changed nothing
uint32_t rounds_of(const Case& c, std::mt19937& rng, std::vector<uint32_t>& D) {
	const SettleDims d = settle_dims(c.extent, static_cast<int64_t>(c.table.size()));
	D.assign(d.n, 0u);
	for (uint32_t s = 0; s < d.n; ++s) D[s] = c.chosen[s] ? kSettleUnknown : 0u;
	auto moving = [&](int32_t label) {
		return settle_moving_slot([&](uint32_t slot) { return c.table[slot].label; }, [&](uint32_t slot) { return c.chosen[slot]; }, d.n, label);
	};
	uint32_t rounds = 0, changes = 1;
	while (changes != 0 && rounds < d.n + 10) {
		++rounds;
		changes = 0;
		const std::vector<uint32_t> start = D;
		auto read = [&](int32_t slot) { return rng() & 1u ? start[slot] : D[slot]; };
		for (uint32_t col = 0; col < d.columns; ++col) {
			SettleBelow below = settle_floor();
			for (int32_t z = 0; z < d.nz; ++z) {
				const int32_t label = c.labels[static_cast<size_t>(z) * d.columns + col];
				SettleContact k;
				if (label == 0 || !settle_step(below, label, z, moving, k)) continue;
				const uint32_t cand = settle_candidate(k.lower >= 0 ? read(k.lower) : 0u, k.gap);
				if (cand < read(k.upper)) {
					const uint32_t old = D[k.upper]; // the atomic minimum and what it returns
					D[k.upper] = std::min(old, cand);
					if (cand < old) ++changes;
				}
			}
		}
	}
	return rounds;
}

// drops by loops of this file alone: the contacts as a list, relaxed until nothing changes
std::vector<uint32_t> plain(const Case& c) {
	struct Contact {
		int upper, lower, gap;
	};
	const int nx = c.extent[0], ny = c.extent[1], nz = c.extent[2], n = static_cast<int>(c.table.size());
	auto slot_of = [&](int32_t label) {
		for (int s = 0; s < n; ++s)
			if (c.table[s].label == label) return c.chosen[s] ? s : -1;
		return -1;
	};
	std::vector<Contact> contacts;
	for (int y = 0; y < ny; ++y)
		for (int x = 0; x < nx; ++x) {
			int32_t below_label = 0;
			int below_z = -1;
			for (int z = 0; z < nz; ++z) {
				const int32_t label = c.labels[(static_cast<size_t>(z) * ny + y) * nx + x];
				if (label == 0) continue;
				if (label != below_label && slot_of(label) >= 0) contacts.push_back({slot_of(label), below_label ? slot_of(below_label) : -1, z - below_z - 1});
				below_label = label;
				below_z = z;
			}
		}
	std::vector<uint32_t> drop(n);
	for (int s = 0; s < n; ++s) drop[s] = c.chosen[s] ? kSettleUnknown : 0u;
	for (bool changed = true; changed;) {
		changed = false;
		for (const Contact& k : contacts) {
			const uint32_t base = k.lower >= 0 ? drop[k.lower] : 0u;
			if (base != kSettleUnknown && base + k.gap < drop[k.upper]) {
				drop[k.upper] = base + k.gap;
				changed = true;
			}
		}
	}
	for (auto& v : drop) v = v == kSettleUnknown ? 0u : v;
	return drop;
}

} // namespace

int main() {
	std::mt19937 rng(20261021u);
	int volumes = 0, rounds_over = 0;
	const uint32_t densities[4] = {5, 15, 30, 60};
	for (int i = 0; i < 200; ++i) {
		Case c;
		c.extent[0] = 1 + rng() % 9;
		c.extent[1] = 1 + rng() % 7;
		c.extent[2] = 1 + rng() % 20;
		const uint32_t pieces = 1 + rng() % 14;
		c.labels.resize(static_cast<size_t>(c.extent[0]) * c.extent[1] * c.extent[2]);
		for (auto& l : c.labels) l = rng() % 100 < densities[i % 4] ? static_cast<int32_t>(3 * (1 + rng() % pieces)) : 0;
		for (uint32_t p = 1; p <= pieces; ++p)
			if (rng() % 8 != 0) { // (a label that is not in the table is static)
				bm_component rec{};
				rec.label = static_cast<int32_t>(3 * p);
				c.table.push_back(rec);
				c.chosen.push_back(rng() % 10 < 7 ? static_cast<uint8_t>(1 + rng() % 255) : 0);
			}
		const uint32_t n = static_cast<uint32_t>(c.table.size());
		uint32_t chosen = 0;
		for (const uint8_t b : c.chosen) chosen += b != 0;
		std::vector<uint32_t> D;
		const uint32_t rounds = rounds_of(c, rng, D);
		if (rounds > chosen + 2) ++rounds_over;
		const std::vector<uint32_t> want = plain(c);
		std::vector<uint8_t> out(c.labels.size(), 9);
		std::vector<int32_t> drops(n, -1);
		bm_settle_result rec{};
		EXPECT(bm_host_settle(c.extent, c.labels.data(), n ? c.table.data() : nullptr, n, n ? c.chosen.data() : nullptr, out.data(), n ? drops.data() : nullptr, &rec) == 0);
		bool same = true;
		uint32_t largest = 0, moved = 0;
		for (uint32_t s = 0; s < n; ++s) {
			const uint32_t by = c.chosen[s] ? settle_final_drop(D[s]) : 0u;
			same = same && by == want[s] && drops[s] == static_cast<int32_t>(want[s]);
			largest = std::max(largest, want[s]);
			moved += want[s] != 0;
		}
		EXPECT(same);
		EXPECT(rec.chosen_pieces == chosen && rec.moved_pieces == moved && rec.largest_drop == largest && rec.reserved == 0);
		size_t solid = 0, landed = 0, twos = 0;
		for (const int32_t l : c.labels) solid += l != 0;
		for (const uint8_t b : out) {
			EXPECT(b <= 2);
			landed += b != 0;
			twos += b == 2;
		}
		EXPECT(solid == landed && twos == rec.moved_voxels); // no two voxels on one
		++volumes;
	}
	EXPECT(rounds_over == 0);
	std::printf("volumes %d\nrounds_over %d\n", volumes, rounds_over);
	// ---- refusals
	int refused = 0;
	{
		int32_t labels[8] = {0, 0, 0, 0, 4, 0, 0, 0};
		bm_component table[1] = {};
		table[0].label = 4;
		uint8_t chosen[1] = {1}, out[8];
		int32_t drops[1];
		bm_settle_result rec{};
		const int32_t ok[3] = {2, 2, 2}, zero[3] = {0, 2, 2}, wide[3] = {2, 16385, 2}, many[3] = {16384, 16384, 8};
		if (bm_host_settle(zero, labels, table, 1, chosen, out, drops, &rec) == BM_EINVAL) ++refused;
		if (bm_host_settle(wide, labels, table, 1, chosen, out, drops, &rec) == BM_EINVAL) ++refused;
		if (bm_host_settle(many, labels, table, 1, chosen, out, drops, &rec) == BM_EINVAL) ++refused;
		if (bm_host_settle(ok, labels, table, -1, chosen, out, drops, &rec) == BM_EINVAL) ++refused;
		if (bm_host_settle(ok, nullptr, table, 1, chosen, out, drops, &rec) == BM_EINVAL) ++refused;
		if (bm_host_settle(ok, labels, nullptr, 1, chosen, out, drops, &rec) == BM_EINVAL) ++refused;
		EXPECT(bm_host_settle(ok, labels, table, 1, chosen, out, drops, &rec) == 0 && drops[0] == 1 && out[0] == 2 && out[4] == 0 && rec.moved_voxels == 1 && rec.contacts == 1);
	}
	std::printf("refused %d\n", refused);
	std::printf("failures %d\n", failures);
	return failures == 0 ? 0 : 1;
}
