// voxelize_check.cpp -- a program with its own main around csrc/voxelize_host.cpp (linked alone: no HIP, no library), built by
// tests/test_voxelize_host.py plain and under the address and undefined-behaviour sanitizers.  It walks the cases at the 64-bit bounds of
// the contract -- |q| = 2^22, an extent of 2^19 -- where an overflow would be undefined behaviour, checks the row form of the surface rule
// against the voxel form, the refusals, and that bytes outside the rows stay.  Prints counters and "failures N".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/brickmap.h"
#include "../brickmap_amd/csrc/voxelize.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                      \
	do {                                                                  \
		if (!(cond)) {                                                    \
			++failures;                                                   \
			std::printf("line %d: %s\n", __LINE__, #cond);                \
		}                                                                 \
	} while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return static_cast<uint32_t>(rng_state >> 32);
}

bm_voxelize_params params(int lx, int ly, int lz, int nx, int ny, int nz, uint32_t mode, uint32_t flags = 0) {
	bm_voxelize_params p = {};
	p.lo[0] = lx; p.lo[1] = ly; p.lo[2] = lz;
	p.extent[0] = nx; p.extent[1] = ny; p.extent[2] = nz;
	p.mode = mode;
	p.flags = flags;
	return p;
}

} // namespace

int main(int argc, char** argv) {
	const int rounds = argc > 1 ? std::atoi(argv[1]) : 20;
	long voxels = 0, triangles = 0, refused = 0, rows = 0;

	// ---- the bounds: vertices at +-2^22 (16384 voxels from the origin), extents of exactly 2^19 and one unit more
	{
		const float far = 16384.0f, span = 2048.0f;
		// a triangle along the last 2048 voxels of a row of 16384: q_x reaches 2^22 and spans 2^19; then the same triangle about a volume
		// origin of -16384, from coordinates of -16384 on
		const float last[9] = {far, 4, 1, far - span, 6, 7, far, 2, 3};
		const float first[9] = {-far, -16380, -16383, -far + span, -16378, -16377, -far, -16382, -16381};
		for (int s = 0; s < 2; ++s) {
			const bm_voxelize_params p = s == 0 ? params(0, 0, 0, 16384, 8, 8, 3) : params(-16384, -16384, -16384, 16384, 8, 8, 3);
			std::vector<uint8_t> vol(static_cast<size_t>(16384) * 64, 0);
			bm_voxelize_result res = {9, 9, 9};
			EXPECT(bm_host_voxelize(&p, 1, s == 0 ? last : first, vol.data(), &res) == 0);
			EXPECT(res.rejected == 0 && res.degenerate == 0);
			long set = 0;
			for (uint8_t b : vol) set += b;
			EXPECT(set > 2000);
			voxels += set;
			++triangles;
		}
		// one unit beyond either bound is rejected and leaves nothing
		const bm_voxelize_params p = params(0, 0, 0, 64, 8, 8, 3);
		std::vector<uint8_t> vol(64 * 64, 0);
		bm_voxelize_result res = {};
		const float over_q[9] = {far + 1.0f / 256, 1, 1, far, 3, 1, far, 1, 3};
		const float over_span[9] = {0, 1, 1, span + 1.0f / 256, 3, 1, 2, 1, 3};
		const float at_span[9] = {0, 1, 1, span, 3, 1, 2, 1, 3};
		const float huge[9] = {4194304.5f, 1, 1, 2, 3, 1, 2, 1, 3}; // v * 256 = 2^30 + 128: beyond the float test
		const float inf[9] = {std::numeric_limits<float>::infinity(), 1, 1, 2, 3, 1, 2, 1, 3};
		const float nan[9] = {1, std::nanf(""), 1, 2, 3, 1, 2, 1, 3};
		const float big[9] = {3.0e38f, 1, 1, 2, 3, 1, 2, 1, 3}; // the product overflows to infinity
		const float* bad[6] = {over_q, over_span, huge, inf, nan, big};
		for (const float* b : bad) {
			EXPECT(bm_host_voxelize(&p, 1, b, vol.data(), &res) == 0);
			EXPECT(res.rejected == 1 && res.degenerate == 0 && res.open_columns == 0);
			long set = 0;
			for (uint8_t v : vol) set += v;
			EXPECT(set == 0);
		}
		const float neg_q[9] = {-far, 1, 1, -far + span, 3, 1, -far, 1, 3}; // q = -2^22: accepted, and wholly outside the volume
		EXPECT(bm_host_voxelize(&p, 1, at_span, vol.data(), &res) == 0);
		EXPECT(res.rejected == 0);
		const bm_voxelize_params ps = params(0, 0, 0, 64, 8, 8, 1); // (surface alone: the crossings of one triangle on the -x side fill its rows)
		EXPECT(bm_host_voxelize(&ps, 1, neg_q, vol.data(), &res) == 0);
		EXPECT(res.rejected == 0 && res.degenerate == 0 && res.open_columns == 0);
		{
			long set = 0;
			for (uint8_t v : vol) set += v;
			EXPECT(set == 0);
		}
		// the largest normal: a right triangle with legs of 2^19 on two axes, seen from a volume at its far corner
		const bm_voxelize_params pc = params(16384 - 2048, 16384 - 2048, 0, 2048, 16, 4, 3);
		std::vector<uint8_t> volc(static_cast<size_t>(2048) * 16 * 4, 0);
		const float legs[9] = {far - span, far - span, 1.5f, far, far - span, 1.5f, far - span, far, 2.5f};
		EXPECT(bm_host_voxelize(&pc, 1, legs, volc.data(), &res) == 0);
		EXPECT(res.rejected == 0 && res.degenerate == 0);
		++triangles;
	}

	// ---- the row form of the surface rule == the voxel form; the crossing rule stays inside 0 ... nx
	for (int r = 0; r < rounds; ++r) {
		float v[9];
		const int scale = r % 3 == 0 ? 4 : (r % 3 == 1 ? 64 : 1024);
		for (float& c : v) c = static_cast<float>(static_cast<int>(rnd() % (64u * scale)) - 16 * scale) / 4.0f; // quarter voxels
		const int32_t lo[3] = {0, 0, 0};
		bm::VxTri t;
		if (bm::vx_snap(v, lo, t) != bm::kVxOk) continue;
		++triangles;
		for (int probe = 0; probe < 64; ++probe) {
			const int x8 = 8 * ((t.mn[0] >> 11) + static_cast<int>(rnd() % 8u) - 1);
			const int y = (t.mn[1] >> 8) + static_cast<int>(rnd() % 16u) - 2, z = (t.mn[2] >> 8) + static_cast<int>(rnd() % 16u) - 2;
			const uint32_t m = bm::vx_surface_row8(t, x8, y, z);
			for (int i = 0; i < 8; ++i) EXPECT(((m >> i) & 1u) == (bm::vx_surface_voxel(t, x8 + i, y, z) ? 1u : 0u));
			++rows;
			int k = -1;
			if (t.n[0] != 0 && bm::vx_solid_crossing(t, y, z, 40, &k)) EXPECT(k >= 0 && k <= 40);
		}
	}

	// ---- a volume inside a larger array: the bytes between rows and slices stay, with and without KEEP
	for (uint32_t flags = 0; flags < 2; ++flags) {
		bm_voxelize_params p = params(0, 0, 0, 13, 9, 7, 3, flags);
		p.row_pitch = 20;
		p.slice_pitch = 20 * 11;
		std::vector<uint8_t> arr(static_cast<size_t>(20) * 11 * 7 + 5, 0xAB);
		const float box[2][9] = {{2, 2, 2, 9, 2, 2, 2, 7, 5}, {9, 2, 2, 9, 7, 5, 2, 7, 5}};
		bm_voxelize_result res = {};
		EXPECT(bm_host_voxelize(&p, 2, &box[0][0], arr.data() + 3, &res) == 0);
		long inside = 0;
		for (size_t i = 0; i < arr.size(); ++i) {
			const long o = static_cast<long>(i) - 3;
			const bool in_row = o >= 0 && o % 20 < 13 && (o / 20) % 11 < 9 && o / 220 < 7;
			if (!in_row) EXPECT(arr[i] == 0xAB);
			else if (flags) EXPECT(arr[i] == 0xAB);
			else { EXPECT(arr[i] <= 1); inside += arr[i]; }
		}
		EXPECT(flags || inside > 20);
		voxels += inside;
	}

	// ---- refusals
	{
		std::vector<uint8_t> vol(512, 3);
		const float tri[9] = {1, 1, 1, 5, 1, 1, 1, 5, 2};
		bm_voxelize_params p = params(0, 0, 0, 8, 8, 8, 3);
		auto refuse = [&](const bm_voxelize_params& q, int64_t n, const float* t, uint8_t* v) {
			EXPECT(bm_host_voxelize(&q, n, t, v, nullptr) == BM_EINVAL);
			++refused;
		};
		bm_voxelize_params q = p;
		q.extent[0] = 0; refuse(q, 1, tri, vol.data());
		q = p; q.extent[2] = 16385; refuse(q, 1, tri, vol.data());
		q = p; q.row_pitch = 7; refuse(q, 1, tri, vol.data());
		q = p; q.slice_pitch = 63; refuse(q, 1, tri, vol.data());
		q = p; q.row_pitch = -8; refuse(q, 1, tri, vol.data());
		q = p; q.mode = 0; refuse(q, 1, tri, vol.data());
		q = p; q.mode = 7; refuse(q, 1, tri, vol.data());
		q = p; q.flags = 2; refuse(q, 1, tri, vol.data());
		refuse(p, -1, tri, vol.data());
		refuse(p, 1, nullptr, vol.data());
		refuse(p, 1, tri, nullptr);
		EXPECT(bm_host_voxelize(nullptr, 1, tri, vol.data(), nullptr) == BM_EINVAL);
		++refused;
		for (uint8_t b : vol) EXPECT(b == 3);
		EXPECT(bm_host_voxelize(&p, 0, nullptr, vol.data(), nullptr) == 0); // no triangle: zeros
		for (uint8_t b : vol) EXPECT(b == 0);
	}

	std::printf("triangles %ld voxels %ld rows %ld refused %ld failures %d\n", triangles, voxels, rows, refused, failures);
	return failures == 0 ? 0 : 1;
}
