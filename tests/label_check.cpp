// label_check.cpp -- a program around brickmap_amd/csrc/label_host.cpp alone (no HIP, no scene): bm_host_label_volume against a plain
// flood fill on seeded volumes, and the in-brick rounds of csrc/label.h -- run here lane by lane as label.hip runs them in a wave --
// against bm_host_label_volume on 8 x 8 x 8 bricks.  Built plain and under the address and undefined-behaviour sanitizers by
// tests/test_label_host.py.  Usage: label_check <volumes>.  Prints counts and "failures 0".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/brickmap.h"
#include "../brickmap_amd/csrc/label.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return static_cast<uint32_t>(rng_state >> 32);
}

// labels by flood fill in index order: the first voxel of a component is the first one the scan meets
uint64_t flood(const std::vector<uint8_t>& v, int nx, int ny, int nz, std::vector<int32_t>& out) {
	out.assign(v.size(), 0);
	uint64_t count = 0;
	std::vector<int> stack;
	for (int i = 0; i < static_cast<int>(v.size()); ++i) {
		if (!v[i] || out[i]) continue;
		++count;
		out[i] = i + 1;
		stack.push_back(i);
		while (!stack.empty()) {
			const int j = stack.back();
			stack.pop_back();
			const int x = j % nx, y = j / nx % ny, z = j / (nx * ny);
			const int nb[6] = {x > 0 ? j - 1 : -1, x + 1 < nx ? j + 1 : -1, y > 0 ? j - nx : -1, y + 1 < ny ? j + nx : -1, z > 0 ? j - nx * ny : -1, z + 1 < nz ? j + nx * ny : -1};
			for (int k : nb)
				if (k >= 0 && v[k] && !out[k]) { out[k] = i + 1; stack.push_back(k); }
		}
	}
	return count;
}

// the rounds of label_local (label.hip), the 64 lanes one after another on the state of the round before; returns the rounds taken
int brick_rounds(const uint32_t bits[64], bm::LabelRow rows[64]) {
	using namespace bm;
	for (uint32_t r = 0; r < 64; ++r) rows[r] = label_row_init(bits[r], r);
	for (int round = 0; round < kLabelBrickRounds; ++round) {
		LabelRow next[64];
		bool any = false;
		for (int r = 0; r < 64; ++r) {
			const int src[4] = {r - 1, r + 1, r - 8, r + 8};
			const bool have[4] = {(r & 7) != 0, (r & 7) != 7, (r >> 3) != 0, (r >> 3) != 7};
			LabelRow near = {{kLabelRowEmpty, kLabelRowEmpty, kLabelRowEmpty, kLabelRowEmpty}};
			for (int n = 0; n < 4; ++n)
				if (have[n]) near = label_row_min(near, rows[src[n]]);
			next[r] = rows[r];
			any = label_row_settle(next[r], bits[r], near) || any;
		}
		for (int r = 0; r < 64; ++r) rows[r] = next[r];
		if (!any) return round + 1;
	}
	return kLabelBrickRounds + 1; // did not settle within the bound
}

} // namespace

int main(int argc, char** argv) {
	const int volumes = argc > 1 ? std::atoi(argv[1]) : 20;
	long failures = 0, voxels = 0, components = 0, refused = 0, bricks = 0;
	int rounds_max = 0;
	std::vector<int32_t> want, got;
	for (int t = 0; t < volumes; ++t) {
		const int nx = 1 + rnd() % 40, ny = 1 + rnd() % 24, nz = 1 + rnd() % 24;
		static const uint32_t kFill[4] = {10, 30, 50, 90};
		const uint32_t fill = kFill[t % 4];
		std::vector<uint8_t> v(static_cast<size_t>(nx) * ny * nz);
		for (auto& b : v) b = rnd() % 100 < fill ? static_cast<uint8_t>(1 + rnd() % 255) : 0;
		got.assign(v.size(), -7);
		uint64_t n = ~0ull;
		if (bm_host_label_volume(v.data(), nx, ny, nz, got.data(), &n) != 0) { ++failures; continue; }
		const uint64_t m = flood(v, nx, ny, nz, want);
		if (n != m || got != want) ++failures;
		voxels += static_cast<long>(v.size());
		components += static_cast<long>(m);
	}
	// bricks: random fills, and a one-voxel-wide snake through all 512 voxels (the longest path a brick can hold)
	for (int t = 0; t < volumes + 1; ++t) {
		std::vector<uint8_t> v(512);
		if (t == volumes) {
			for (auto& b : v) b = 0;
			// rows along x on even y of even z, joined at alternating ends; layers joined at alternating corners
			for (int z = 0; z < 8; z += 2) {
				for (int y = 0; y < 8; y += 2) {
					for (int x = 0; x < 8; ++x) v[z * 64 + y * 8 + x] = 1;
					if (y + 2 < 8) v[z * 64 + (y + 1) * 8 + ((y / 2) % 2 == 0 ? 7 : 0)] = 1;
				}
				if (z + 2 < 8) v[(z + 1) * 64 + ((z / 2) % 2 == 0 ? 6 * 8 + 0 : 0)] = 1;
			}
		} else {
			static const uint32_t kFill[5] = {10, 30, 50, 70, 90};
			const uint32_t fill = kFill[t % 5];
			for (auto& b : v) b = rnd() % 100 < fill;
		}
		uint32_t bits[64];
		for (int r = 0; r < 64; ++r) {
			bits[r] = 0;
			for (int x = 0; x < 8; ++x) bits[r] |= (v[r * 8 + x] ? 1u : 0u) << x;
		}
		bm::LabelRow rows[64];
		const int rounds = brick_rounds(bits, rows);
		if (rounds > bm::kLabelBrickRounds) ++failures;
		rounds_max = rounds > rounds_max ? rounds : rounds_max;
		got.assign(512, -7);
		uint64_t n = 0;
		if (bm_host_label_volume(v.data(), 8, 8, 8, got.data(), &n) != 0) { ++failures; continue; }
		for (int i = 0; i < 512; ++i) {
			const uint32_t l = bm::label_row_get(rows[i >> 3], i & 7);
			if ((l == 0xFFFFu ? 0 : static_cast<int32_t>(l) + 1) != got[i]) { ++failures; break; }
		}
		++bricks;
	}
	// refusals, and the empty volume
	{
		uint8_t v[8] = {1, 1, 0, 0, 0, 0, 1, 1}; // two pieces
		int32_t l[8];
		uint64_t n = 5;
		refused += bm_host_label_volume(v, -1, 1, 1, l, &n) == BM_EINVAL;
		refused += bm_host_label_volume(v, 2, 2, 2, l, nullptr) == BM_EINVAL;
		refused += bm_host_label_volume(nullptr, 2, 2, 2, l, &n) == BM_EINVAL;
		refused += bm_host_label_volume(v, 2, 2, 2, nullptr, &n) == BM_EINVAL;
		refused += bm_host_label_volume(v, 1 << 20, 1 << 20, 1 << 20, l, &n) == BM_EINVAL;
		refused += bm_host_label_volume(v, (1ll << 31) - 1, 1, 1, l, &n) == BM_EINVAL;
		if (bm_host_label_volume(v, 0, 5, 5, nullptr, &n) != 0 || n != 0) ++failures;
		if (bm_host_label_volume(v, 2, 2, 2, l, &n) != 0 || n != 2) ++failures;
	}
	std::printf("volumes %d voxels %ld components %ld bricks %ld rounds_max %d refused %ld failures %ld\n", volumes, voxels, components, bricks, rounds_max, refused, failures);
	return failures == 0 ? 0 : 1;
}
