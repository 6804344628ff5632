// step_pair_check.cpp -- CPU test of the pair move (brickmap_amd/csrc/steps.h step_pair_ahead / step_pair_commit) and of the guard bytes
// round the cube field (brickmap_amd/csrc/field_layout.h field_guard_bytes), compiled and run by tests/test_step_pair.py.
//   1. Replay.  For (tmax, tdelta, increments, cell) states -- random, ties in every pair of axes and in all three, zero direction
//      components (tmax = 1e6, tdelta = 0), signed zeros, NaN, raw bit patterns -- the pair move equals plain moves bit for bit:
//        after step_pair_ahead               tmax, p, last_step of ONE plain move ("stops at cell 1": the lane keeps exactly this)
//        StepAhead::p, StepAhead::step       the cell and the increment of the SECOND plain move, committed or not
//        after step_pair_commit              tmax, p, last_step of TWO plain moves ("continues")
//      The plain move is written out here as the kernels' step_advance has it (traverse.h), from the reference's voxel.cuh:249-258.
//   2. Bounds.  For every BASELINE world (16, 128, 256, 512 cells per side), a flat one (1024 x 1024 x 16 cells) and a tall one
//      (16 x 16 x 992), with 8, 9 and 10 planes: from EVERY cell of the bordered box of the first and of the last plane, border cells
//      included, each of the six increments leads to an offset inside [-guard, planes x plane + guard), guard being what the allocation
//      uses.  (A committed cell is always inside its bordered plane; the cell a pair move looks at without committing is one move further.)
//      And what the kernels rely on because they extend an offset with zeros: with the increments a ray of the plane's own octant can
//      have (plane 0: none negative; the sun and view planes: any), no offset is below 0 or at 2^32 and beyond.
// usage: step_pair_check [states] [largest world's cells per side]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../brickmap_amd/csrc/field_layout.h"
#include "../brickmap_amd/csrc/steps.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return static_cast<uint32_t>(rng_state >> 32);
}
static float rndf() { return (rnd() >> 8) * (1.0f / 16777216.0f); }
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float fbits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static long failures = 0;
#define FAIL(...) do { if (failures < 10) { std::fprintf(stderr, "FAIL: " __VA_ARGS__); std::fprintf(stderr, "\n"); } failures++; } while (0)

struct Walk {
	float t[3], d[3];
	uint32_t p;
	int last_step;
};
// one plain move, as step_advance (traverse.h) makes it
static void plain_move(Walk& w, const int s[3]) {
	const bool mx = w.t[0] < w.t[1] && w.t[0] < w.t[2];
	const bool my = w.t[1] <= w.t[0] && w.t[1] < w.t[2];
	const bool mz = !(mx || my);
	const int step = mx ? s[0] : (my ? s[1] : s[2]);
	w.p += static_cast<uint32_t>(step);
	w.last_step = step;
	w.t[0] = w.t[0] + (mx ? w.d[0] : 0.f);
	w.t[1] = w.t[1] + (my ? w.d[1] : 0.f);
	w.t[2] = w.t[2] + (mz ? w.d[2] : 0.f);
}
// bit for bit -- but where tmax AND tdelta of an axis are NaN, which of the two payloads their sum carries is the compiler's choice of
// operand order (IEEE 754 leaves it open), in this file as in steps.h: there both must be NaN
static bool same(const Walk& a, const Walk& b) {
	for (int i = 0; i < 3; ++i) {
		const bool two_nans = a.d[i] != a.d[i] && a.t[i] != a.t[i] && b.t[i] != b.t[i];
		if (bits(a.t[i]) != bits(b.t[i]) && !two_nans) return false;
	}
	return a.p == b.p && a.last_step == b.last_step;
}

static float special(uint32_t k) {
	switch (k % 8) {
	case 0: return 0.f;
	case 1: return -0.f;
	case 2: return 1000000.f;
	case 3: return fbits(0x7FC00000u | (rnd() & 0x3FFFFFu));             // quiet NaN, any payload
	case 4: return fbits(0x7F800001u + (rnd() & 0x3FFFFEu));             // signalling NaN
	case 5: return fbits(rnd());                                          // any bit pattern
	case 6: return fbits(0x7F800000u | (rnd() & 0x80000000u));            // infinities
	default: return static_cast<float>(rnd() % 64) * 0.25f;               // small exact values: ties after a move as well
	}
}

int main(int argc, char** argv) {
	const long states = argc > 1 ? std::atol(argv[1]) : 20000000;
	const int largest = argc > 2 ? std::atoi(argv[2]) : 1024;

	// ---- 1. replay
	long stops = 0, ties2 = 0, ties3 = 0, zero_dir = 0, nan_in = 0, negzero = 0, axis_count[3] = {0, 0, 0};
	for (long i = 0; i < states; ++i) {
		Walk w{};
		const uint32_t mode = rnd() % 8;
		for (int a = 0; a < 3; ++a) {
			w.t[a] = mode == 0 ? fbits(rnd()) : (rndf() * (mode == 1 ? 4.f : 600.f));
			w.d[a] = mode == 0 && rnd() % 2 ? fbits(rnd()) : 1.f / (rndf() + 1e-6f);
		}
		if (mode == 2) { const int a = rnd() % 3, b = (a + 1 + rnd() % 2) % 3; w.t[b] = w.t[a]; ties2++; }                   // a tie in one pair
		if (mode == 3) { w.t[1] = w.t[0]; w.t[2] = w.t[0]; if (rnd() % 2) w.d[1] = w.d[0]; if (rnd() % 2) w.d[2] = w.d[0]; ties3++; } // all three, and again after the move
		if (mode == 4) { for (int a = 0; a < 3; ++a) if (rnd() % 3 == 0) { w.t[a] = 1000000.f; w.d[a] = 0.f; } zero_dir++; }     // zero direction components
		if (mode == 5) { w.t[rnd() % 3] = special(rnd()); if (rnd() % 2) w.t[rnd() % 3] = special(rnd()); if (rnd() % 4 == 0) w.d[rnd() % 3] = special(rnd()); }
		if (mode == 6) { for (int a = 0; a < 3; ++a) { w.t[a] = static_cast<float>(rnd() % 8) * 0.5f; w.d[a] = static_cast<float>(1 + rnd() % 4) * 0.5f; } } // exact: the second choice ties too
		for (int a = 0; a < 3; ++a) { nan_in += w.t[a] != w.t[a]; negzero += bits(w.t[a]) == 0x80000000u; }
		const int shift = 2 + static_cast<int>(rnd() % 9);
		const int pxy = static_cast<int>((3u + rnd() % 1024u) << shift);
		int s[3] = {1, 1 << shift, pxy};
		for (int a = 0; a < 3; ++a) { const uint32_t k = rnd() % 8; s[a] = k == 0 ? 0 : (k & 1 ? s[a] : -s[a]); }
		w.p = rnd() % 16 == 0 ? rnd() : rnd() % (1u << 30);
		w.last_step = static_cast<int>(rnd() % 3) - 1;

		Walk one = w, two;
		plain_move(one, s);
		two = one;
		plain_move(two, s);

		Walk pair = w;
		const bm::StepAhead a = bm::step_pair_ahead(pair.t[0], pair.t[1], pair.t[2], pair.d[0], pair.d[1], pair.d[2], pair.p, pair.last_step, s[0], s[1], s[2]);
		if (!same(pair, one)) FAIL("state %ld mode %u: after the first move t=(%a %a %a) p=%u last=%d, one plain move t=(%a %a %a) p=%u last=%d", i, mode, pair.t[0], pair.t[1],
								   pair.t[2], pair.p, pair.last_step, one.t[0], one.t[1], one.t[2], one.p, one.last_step);
		if (a.p != two.p || a.step != two.last_step) FAIL("state %ld mode %u: the pair looks at cell %u by %d, the second plain move reaches %u by %d", i, mode, a.p, a.step, two.p, two.last_step);
		if (static_cast<int>(a.m.x) + a.m.y + a.m.z != 1) FAIL("state %ld: not exactly one axis", i);
		if (rnd() % 4 == 0) { // stops at cell 1: the StepAhead is dropped, the lane keeps the state of one plain move, bit for bit
			bm::step_pair_commit(pair.t[0], pair.t[1], pair.t[2], pair.d[0], pair.d[1], pair.d[2], pair.p, pair.last_step, a, false);
			if (!same(pair, one)) FAIL("state %ld mode %u: a lane that stops does not keep the state of one plain move", i, mode);
			stops++;
			continue;
		}
		bm::step_pair_commit(pair.t[0], pair.t[1], pair.t[2], pair.d[0], pair.d[1], pair.d[2], pair.p, pair.last_step, a, true);
		if (!same(pair, two)) FAIL("state %ld mode %u: after the commit t=(%a %a %a) p=%u last=%d, two plain moves t=(%a %a %a) p=%u last=%d", i, mode, pair.t[0], pair.t[1], pair.t[2],
								   pair.p, pair.last_step, two.t[0], two.t[1], two.t[2], two.p, two.last_step);
		axis_count[a.m.x ? 0 : (a.m.y ? 1 : 2)]++;
	}

	// ---- 2. bounds
	struct Dims { int cells, cells_h; };
	const Dims worlds[] = {{16, 16}, {128, 128}, {256, 256}, {512, 512}, {1024, 16}, {16, 992}};
	long long cells_checked = 0, beyond = 0;
	int worlds_checked = 0;
	for (const Dims& dm : worlds) {
		if (dm.cells > largest || dm.cells_h > largest) continue;
		worlds_checked++;
		const bm::FieldLayout l = bm::field_layout(dm.cells, dm.cells_h);
		if (!l.fits) { FAIL("world %d x %d does not fit", dm.cells, dm.cells_h); continue; }
		const long long guard = static_cast<long long>(bm::field_guard_bytes(l)), pxy = static_cast<long long>(l.pxy), plane = static_cast<long long>(l.plane);
		if (guard < pxy) FAIL("guard %lld below the slice pitch %lld", guard, pxy);
		const long long inc[6] = {1, -1, 1ll << l.shift, -(1ll << l.shift), pxy, -pxy};
		const int X = dm.cells + 2, Z = dm.cells_h + 2;
		for (int planes = 8; planes <= 10; ++planes) {
			if (static_cast<unsigned long long>(plane) * planes >= (1ull << 32)) continue; // no such allocation (field_layout: ninth / tenth)
			const long long lo = -guard, hi = plane * planes + guard;
			for (const int pl : {0, planes - 1}) {
				if (pl == 0 && planes != 8) continue; // (the first plane's offsets and the lower bound are those of 8 planes, whose upper bound is the tightest)
				// the increments a ray that walks this plane can have: its octant's signs for an octant plane, any for the sun and view planes
				bool can[6];
				for (int k = 0; k < 6; ++k) can[k] = pl >= 8 || ((pl >> (k / 2)) & 1) == (k & 1);
				for (int z = 0; z < Z; ++z)
					for (int y = 0; y < X; ++y) {
						const long long row = plane * pl + ((static_cast<long long>(z) * X + y) << l.shift);
						for (int x = 0; x < X; ++x) {
							const long long p1 = row + x;
							for (int k = 0; k < 6; ++k) {
								const long long p2 = p1 + inc[k];
								if (p2 < lo || p2 >= hi) FAIL("world %d x %d, %d planes: cell (%d %d %d) of plane %d by %lld leaves the allocation: %lld outside [%lld, %lld)", dm.cells,
															  dm.cells_h, planes, x, y, z, pl, inc[k], p2, lo, hi);
								if (can[k] && (p2 < 0 || p2 >= (1ll << 32))) FAIL("world %d x %d, %d planes: offset %lld of plane %d does not extend with zeros", dm.cells, dm.cells_h, planes, p2, pl);
								beyond += p2 < 0 || p2 >= plane * planes;
							}
						}
						cells_checked += X;
					}
			}
		}
	}
	std::printf("states %ld stops %ld ties2 %ld ties3 %ld zerodir %ld nan %ld negzero %ld movex %ld movey %ld movez %ld worlds %d cells %lld beyond %lld failures %ld\n", states, stops, ties2,
				ties3, zero_dir, nan_in, negzero, axis_count[0], axis_count[1], axis_count[2], worlds_checked, cells_checked, beyond, failures);
	return failures ? 1 : 0;
}
