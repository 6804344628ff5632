// jump_worth_check.cpp -- CPU test of the rule "is a jump worth it here" (brickmap_amd/csrc/steps.h jump_worth, field_state),
// compiled and run by tests/test_jump_worth.py.
//   1. jump_worth implies jump_possible, on random and special tmax / tdelta triples (signed zeros, the 1e6 sentinel of a zero
//      direction component, tmax on and next to every binade end, tdelta from 1 to 1e6, raw bit patterns: NaN, infinities, negatives);
//      and the rule is what it says: the smallest tmax in [2^BM_JUMP_WORTH_EXP, 2^19).
//   2. A walk that does what the kernel does with field_state's answer -- single moves while the lane is ST_OUTER, a jump over the cube
//      byte when it is ST_JUMP, and now and then the jump an ST_OUTER lane takes when it rides in a jump pass of other lanes -- is in
//      the state of the reference's one-cell-at-a-time stepping (src/voxel.cuh:249-258) after every operation: the same steps per
//      axis, the same tmax bits.  Ray families: those of tests/jump_check.cpp.
//   3. A lane does not stay "not worth" for ever: each single move adds tdelta[a] > 0 to the smallest tmax, so after at most
//      floor(2^E / tdelta[a]) + 1 moves of axis a its tmax is at or above 2^E, and with all three there the lane is worth a jump again:
//      a run of not-worth moves is at most sum_a (floor(2^E / tdelta[a]) + 2) long (30 for a unit direction and E = 3) -- or the
//      smallest tmax has reached 2^19, beyond every supported world (1026 cells per axis): the walk has ended.
// usage: jump_worth_check [triples] [rays]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

// the rule written out: the smallest tmax (the reference's compares) is a number in [2^E, 2^19)
static bool want_worth(float tx, float ty, float tz) {
	float m = tx < ty ? tx : ty;
	m = m < tz ? m : tz;
	return m >= std::ldexp(1.f, BM_JUMP_WORTH_EXP) && m < std::ldexp(1.f, 19);
}
static void check_triple(float tx, float ty, float tz, float dx, float dy, float dz) {
	const bool w = bm::jump_worth(tx, ty, tz, dx, dy, dz), p = bm::jump_possible(tx, ty, tz);
	if (w && !p) FAIL("worth but not possible: t=(%a %a %a) d=(%a %a %a)", tx, ty, tz, dx, dy, dz);
	if (w != want_worth(tx, ty, tz)) FAIL("worth %d, the rule says %d: t=(%a %a %a)", w, !w, tx, ty, tz);
}

static float special_t(uint32_t k) {
	const uint32_t sel = k % 8;
	const int e = static_cast<int>(rnd() % 36) - 14; // binade ends 2^-14 ... 2^21: both ends of jump_possible and the floor of the rule
	const float end = std::ldexp(1.f, e);
	switch (sel) {
	case 0: return 0.f;
	case 1: return -0.f;
	case 2: return 1000000.f;
	case 3: return end;
	case 4: return std::nextafter(end, 0.f);
	case 5: return std::nextafter(end, 2.f * end);
	case 6: return fbits(rnd()); // any bit pattern
	default: return std::ldexp(1.f + rndf(), e);
	}
}
static float special_d() {
	const uint32_t sel = rnd() % 4;
	if (sel == 0) return 1.f;
	if (sel == 1) return 1000000.f;
	return std::exp(rndf() * std::log(1000000.f)); // 1 ... 1e6
}

struct Dda {
	float t[3], d[3];
	int step() { // one reference step (voxel.cuh:249-258); returns the axis
		const bool mx = t[0] < t[1] && t[0] < t[2];
		const bool my = t[1] <= t[0] && t[1] < t[2];
		const int a = mx ? 0 : (my ? 1 : 2);
		for (int i = 0; i < 3; ++i) t[i] = t[i] + (i == a ? 1.f : 0.f) * d[i]; // `tmax += mask * tdelta`, literally: a first tmax of -0 becomes +0
		return a;
	}
};

int main(int argc, char** argv) {
	const long triples = argc > 1 ? std::atol(argv[1]) : 20000000;
	const long rays = argc > 2 ? std::atol(argv[2]) : 200000;

	// ---- 1. worth => possible
	long n_worth = 0;
	for (long i = 0; i < triples; ++i) {
		float t[3], d[3];
		const uint32_t mode = rnd() % 4;
		for (int a = 0; a < 3; ++a) {
			if (mode == 0) t[a] = fbits(rnd());
			else if (mode == 1) t[a] = special_t(rnd());
			else t[a] = std::ldexp(1.f + rndf(), static_cast<int>(rnd() % 34) - 13); // 2^-13 ... 2^21
			d[a] = special_d();
		}
		if (mode == 3) t[rnd() % 3] = special_t(rnd()); // one special among plausible ones
		check_triple(t[0], t[1], t[2], d[0], d[1], d[2]);
		n_worth += bm::jump_worth(t[0], t[1], t[2], d[0], d[1], d[2]);
	}
	{ // the floor itself and both ends of the valid range, on each axis
		const float lo = std::ldexp(1.f, BM_JUMP_WORTH_EXP), hi = std::ldexp(1.f, 19);
		for (int a = 0; a < 3; ++a) {
			float t[3] = {1000000.f, 1000000.f, 1000000.f};
			t[a] = lo; if (!bm::jump_worth(t[0], t[1], t[2], 1.f, 1.f, 1.f)) FAIL("2^E is not worth a jump");
			t[a] = std::nextafter(lo, 0.f); if (bm::jump_worth(t[0], t[1], t[2], 1.f, 1.f, 1.f)) FAIL("below 2^E is worth a jump");
			t[a] = std::nextafter(hi, 0.f); if (!bm::jump_worth(t[0], t[1], t[2], 1.f, 1.f, 1.f)) FAIL("just below 2^19 is not worth a jump");
			t[a] = hi; if (bm::jump_worth(t[0], t[1], t[2], 1.f, 1.f, 1.f)) FAIL("2^19 is worth a jump");
		}
	}

	// ---- 2. + 3. walks
	long ops = 0, jumps = 0, rides = 0, singles = 0, ended = 0, longest_run = 0, longest_unit_run = 0, steps_total = 0;
	for (long ray = 0; ray < rays; ++ray) {
		float dir[3];
		const uint32_t kind = rnd() % 8;
		for (int i = 0; i < 3; ++i) dir[i] = rndf() * 2.f - 1.f;
		if (kind == 0) dir[rnd() % 3] *= 1e-3f;
		if (kind == 1) { dir[0] = 1.f; dir[1] = 0.5f; dir[2] = 0.25f; }          // exact binary slopes: tdelta ties
		if (kind == 2) { dir[0] = dir[1]; }                                       // equal components: tmax ties
		if (kind == 3) { dir[rnd() % 3] = 0.f; }                                  // zero component: the 1e6 sentinel
		if (kind == 4) { dir[0] = std::ldexp(1.f, -static_cast<int>(rnd() % 12)); dir[1] = std::ldexp(3.f, -static_cast<int>(rnd() % 12)); }
		const float len = std::sqrt((dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2]);
		if (len == 0.f) continue;
		const bool unit = kind != 1 && kind != 4;
		if (unit) for (int i = 0; i < 3; ++i) dir[i] *= 1.0f / len;
		float o[3];
		for (int i = 0; i < 3; ++i) o[i] = (kind == 5 ? static_cast<float>(rnd() % 100) : rndf() * 100.f) + (kind == 6 ? 0.5f : 0.f);
		Dda s;
		float inv[3];
		for (int i = 0; i < 3; ++i) { // voxel.cuh:166-187
			const int p = static_cast<int>(o[i]);
			const float cb = dir[i] > 0.f ? static_cast<float>(p + 1) : static_cast<float>(p);
			const float rdinv = dir[i] == 0.f ? 0.f : 1.f / dir[i];
			const float sgn = static_cast<float>((0.f < dir[i]) - (dir[i] < 0.f));
			s.t[i] = dir[i] != 0.f ? (cb - o[i]) * rdinv : 1000000.f;
			s.d[i] = sgn * rdinv;
			inv[i] = std::fabs(dir[i]);
		}
		// the longest run of not-worth moves this ray may make below 2^19 (3. above); an axis that never moves (tdelta 0: a zero
		// component) is never the smallest either -- its tmax is the sentinel
		long bound = 0;
		const float floor_t = std::ldexp(1.f, BM_JUMP_WORTH_EXP);
		for (int i = 0; i < 3; ++i) bound += s.d[i] > 0.f ? static_cast<long>(floor_t / s.d[i]) + 2 : 0;
		if (unit && BM_JUMP_WORTH_EXP == 3 && bound > 30) FAIL("bound %ld for a unit direction", bound);
		Dda ref = s; // the reference, one cell at a time
		const int walk = 1 + static_cast<int>(rnd() % (ray % 8 == 0 ? 3000 : 600));
		long done = 0, run = 0;
		while (done < walk) {
			// a cube-field byte for this cell: small cubes, jump-sized ones, now and then a candidate cell the ray passed through (0)
			const uint32_t sel = rnd() % 8;
			const uint32_t v = sel == 0 ? 0u : (sel < 3 ? 1u + rnd() % 3u : (sel < 6 ? 4u + rnd() % 29u : 4u + rnd() % 251u));
			const bool possible = bm::jump_possible(s.t[0], s.t[1], s.t[2]);
			const bool worth = bm::jump_worth(s.t[0], s.t[1], s.t[2], s.d[0], s.d[1], s.d[2]);
			if (worth && !possible) FAIL("walk: worth but not possible");
			uint32_t cube = 0;
			int st = bm::field_state(v, possible, cube, worth);
			if (v == 0u) { st = bm::ST_OUTER; } // a brick the ray passed through: the kernel goes on with ST_OUTER and cube 0
			if (st == bm::ST_JUMP && !(worth && possible && v >= BM_JUMP_MIN)) FAIL("ST_JUMP for byte %u possible %d worth %d", v, possible, worth);
			if (st != bm::ST_JUMP && st != bm::ST_OUTER) FAIL("state %d for byte %u", st, v);
			float mn = s.t[0] < s.t[1] ? s.t[0] : s.t[1];
			mn = mn < s.t[2] ? mn : s.t[2];
			if (!worth) {
				if (!(mn < std::ldexp(1.f, 19))) { ended++; break; } // beyond every supported world: the walk has ended
				if (++run > bound) { FAIL("ray %ld kind %u: %ld moves without becoming worth a jump (bound %ld) t=(%a %a %a)", ray, kind, run, bound, s.t[0], s.t[1], s.t[2]); break; }
				if (run > longest_run) longest_run = run;
				if (unit && run > longest_unit_run) longest_unit_run = run;
			} else {
				run = 0;
			}
			// what the lane does: ST_JUMP jumps; ST_OUTER takes a single move, or -- riding in a jump pass other lanes asked for, when its
			// tmax allows a jump at all (no kCubeNoJump) -- the jump over its own cube (a byte of 0 counts as 1)
			const bool ride = st == bm::ST_OUTER && !(cube & bm::kCubeNoJump) && rnd() % 4 == 0;
			uint32_t total;
			if (st == bm::ST_JUMP || ride) {
				uint32_t c[3];
				int last;
				bm::dda_jump(s.t[0], s.t[1], s.t[2], s.d[0], s.d[1], s.d[2], inv[0], inv[1], inv[2], cube & 0xFFu, c[0], c[1], c[2], last);
				total = c[0] + c[1] + c[2];
				const uint32_t n = (cube & 0xFFu) ? (cube & 0xFFu) : 1u;
				if (total < 1 || c[0] > n || c[1] > n || c[2] > n) FAIL("jump of %u %u %u cells over a cube of %u", c[0], c[1], c[2], n);
				uint32_t rc[3] = {0, 0, 0};
				for (uint32_t q = 0; q < total && q < 1000u; ++q) rc[ref.step()]++;
				if (rc[0] != c[0] || rc[1] != c[1] || rc[2] != c[2]) FAIL("ray %ld: jump c=(%u %u %u), reference (%u %u %u)", ray, c[0], c[1], c[2], rc[0], rc[1], rc[2]);
				if (ride) rides++; else jumps++;
			} else {
				const bm::StepAxis m = bm::step_choose(s.t[0], s.t[1], s.t[2]);
				s.t[0] = bm::step_add(s.t[0], s.d[0], m.x);
				s.t[1] = bm::step_add(s.t[1], s.d[1], m.y);
				s.t[2] = bm::step_add(s.t[2], s.d[2], m.z);
				const int a = ref.step();
				if ((a == 0) != m.x || (a == 1) != m.y || (a == 2) != m.z) FAIL("ray %ld: single move along another axis than the reference's", ray);
				total = 1;
				singles++;
			}
			for (int i = 0; i < 3; ++i)
				if (bits(s.t[i]) != bits(ref.t[i])) { FAIL("ray %ld kind %u: tmax[%d] %a, reference %a after %ld cells", ray, kind, i, s.t[i], ref.t[i], done + total); done = walk; break; }
			done += total;
			steps_total += total;
			ops++;
		}
	}
	std::printf("triples %ld worth %ld walks %ld ops %ld jumps %ld rides %ld singles %ld cells %ld ended %ld longest-run %ld longest-unit-run %ld failures %ld\n", triples, n_worth,
				rays, ops, jumps, rides, singles, steps_total, ended, longest_run, longest_unit_run, failures);
	return failures ? 1 : 0;
}
