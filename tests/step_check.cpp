// step_check.cpp -- CPU replay test of brickmap_amd/csrc/steps.h (compiled and run by tests/test_step_forms.py).
// The Amanatides-Woo move, the packed cell of the brick walk with its occupancy test and field_state are the very functions the
// kernels inline.  Here they are replayed against a literal transcription of the reference's move
// (src/voxel.cuh:122-130, 249-258: masks from three float comparisons, tmax += mask * tdelta) and of its cell arithmetic: identical
// tmax bit patterns, chosen axis, cell / offset increment, "inside", occupancy bit and state -- for random input and for the edge
// families listed in main().
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../brickmap_amd/csrc/steps.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return static_cast<uint32_t>(rng_state >> 32);
}
static float rndf() { return (rnd() >> 8) * (1.0f / 16777216.0f); }
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static long failures = 0, moves_checked = 0, cells_checked = 0;
static void fail(const char* what, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static void fail(const char* what, const char* fmt, ...) {
	if (failures++ < 10) {
		std::fprintf(stderr, "MISMATCH (%s) ", what);
		va_list ap;
		va_start(ap, fmt);
		std::vfprintf(stderr, fmt, ap);
		va_end(ap);
		std::fprintf(stderr, "\n");
	}
}

// ---- the reference's move, written out (voxel.cuh:249-258)
struct RefDda {
	float t[3], d[3];
	int step() {
		const bool mx = t[0] < t[1] && t[0] < t[2];
		const bool my = t[1] <= t[0] && t[1] < t[2];
		const bool mz = !(mx || my);
		t[0] += static_cast<float>(mx) * d[0];
		t[1] += static_cast<float>(my) * d[1];
		t[2] += static_cast<float>(mz) * d[2];
		return mx ? 0 : (my ? 1 : 2);
	}
};

// `n` moves of steps.h's move from (t, d), with per-axis increments inc[] (any non-zero distinct values), against the reference
static void check_moves(const char* family, const float t0[3], const float d[3], const int inc[3], int n) {
	RefDda ref;
	float t[3];
	for (int i = 0; i < 3; ++i) { ref.t[i] = t0[i]; ref.d[i] = d[i]; t[i] = t0[i]; }
	for (int k = 0; k < n; ++k) {
		const bm::StepAxis m = bm::step_choose(t[0], t[1], t[2]);
		const int got_inc = bm::step_pick(m, inc[0], inc[1], inc[2]);
		t[0] = bm::step_add(t[0], d[0], m.x);
		t[1] = bm::step_add(t[1], d[1], m.y);
		t[2] = bm::step_add(t[2], d[2], m.z);
		const int axis = ref.step();
		moves_checked++;
		if (m.x != (axis == 0) || m.y != (axis == 1) || m.z != (axis == 2) || got_inc != inc[axis] || bits(t[0]) != bits(ref.t[0]) || bits(t[1]) != bits(ref.t[1]) ||
			bits(t[2]) != bits(ref.t[2])) {
			fail(family, "move %d: start t=(%a %a %a) d=(%a %a %a): flags %d %d %d inc %d t=(%a %a %a); reference axis %d t=(%a %a %a)", k, t0[0], t0[1], t0[2], d[0],
				 d[1], d[2], m.x, m.y, m.z, got_inc, t[0], t[1], t[2], axis, ref.t[0], ref.t[1], ref.t[2]);
			return;
		}
	}
}

// tmax / tdelta of a ray as voxel.cuh:166-187 sets them up
static void setup(const float o[3], const float dir[3], float t[3], float d[3], int s[3]) {
	for (int i = 0; i < 3; ++i) {
		const int p = static_cast<int>(o[i]);
		const float cb = dir[i] > 0.f ? static_cast<float>(p + 1) : static_cast<float>(p);
		const float rdinv = dir[i] == 0.f ? 0.f : 1.f / dir[i];
		s[i] = (0.f < dir[i]) - (dir[i] < 0.f);
		t[i] = dir[i] != 0.f ? (cb - o[i]) * rdinv : 1000000.f;
		d[i] = static_cast<float>(s[i]) * rdinv;
	}
}

// ---- the brick walk: every move of a ray through an N^3 block, the packed cell against plain coordinates
template <int N>
static void check_walk(const char* family, const int start[3], const float o[3], const float dir[3], const uint32_t* words /* N == 8: 16 */, uint32_t byte) {
	typedef bm::BrickCell<N> C;
	float t0[3], d[3];
	int s[3];
	setup(o, dir, t0, d, s);
	RefDda ref;
	float t[3];
	for (int i = 0; i < 3; ++i) { ref.t[i] = t0[i]; ref.d[i] = d[i]; t[i] = t0[i]; }
	int c[3] = {start[0], start[1], start[2]};
	uint32_t cell = C::start(start[0], start[1], start[2]);
	const int inc[3] = {s[0] * C::kStepX, s[1] * C::kStepY, s[2] * C::kStepZ};
	for (int k = 0; k < 3 * N + 2; ++k) {
		const bool inside = c[0] >= 0 && c[0] < N && c[1] >= 0 && c[1] < N && c[2] >= 0 && c[2] < N;
		cells_checked++;
		if ((C::outside(cell) == 0u) != inside || (C::outside(cell) & 1u)) { fail(family, "cell (%d %d %d): packed %08x says outside = %x", c[0], c[1], c[2], cell, C::outside(cell)); return; }
		if (!inside) return; // the walk is over: nothing reads the cell's other fields
		const uint32_t v = static_cast<uint32_t>(c[0] + N * c[1] + N * N * c[2]);
		// the reference's occupancy bit: bit v of the block's mask in linear order (voxel.cuh:104, 52)
		const uint32_t want_bit = N == 8 ? (words[v >> 5] >> (v & 31u)) & 1u : (byte >> v) & 1u;
		const uint32_t got_bit = C::bit(cell, N == 8 ? words[C::word(cell)] : byte);
		if (C::linear(cell) != v || (N == 8 && C::word(cell) != (v >> 5)) || (N == 8 && (cell & C::kWordMask) != ((v >> 5) << 10)) || got_bit != want_bit) {
			fail(family, "cell (%d %d %d): packed %08x linear %u word %u bit %u, want %u %u %u", c[0], c[1], c[2], cell, C::linear(cell), C::word(cell), got_bit, v, v >> 5, want_bit);
			return;
		}
		const bm::StepAxis m = bm::step_choose(t[0], t[1], t[2]);
		const int got_inc = bm::step_pick(m, inc[0], inc[1], inc[2]);
		cell += static_cast<uint32_t>(got_inc);
		t[0] = bm::step_add(t[0], d[0], m.x);
		t[1] = bm::step_add(t[1], d[1], m.y);
		t[2] = bm::step_add(t[2], d[2], m.z);
		const int axis = ref.step();
		c[axis] += s[axis];
		moves_checked++;
		if (got_inc != inc[axis] || bits(t[0]) != bits(ref.t[0]) || bits(t[1]) != bits(ref.t[1]) || bits(t[2]) != bits(ref.t[2])) {
			fail(family, "walk move %d from (%d %d %d): inc %d want %d (axis %d)", k, start[0], start[1], start[2], got_inc, inc[axis], axis);
			return;
		}
		if (s[axis] == 0) return; // a zero component chosen (1e6 the smallest): cannot happen inside a block, nothing more to compare
	}
	fail(family, "walk from (%d %d %d) did not leave the block", start[0], start[1], start[2]);
}

// ---- NaN input (a bounce off a zero normal gives a direction of three NaN; the kernels only guard against hanging).  The decision
// (steps.h): the move keeps the reference's compares, so a NaN tmax compares false everywhere -- the flags and the tmax patterns are the
// reference's, which check_moves asserts below for NaN tmax and for the all-NaN state of a NaN direction.  The brick walk then either leaves the block
// through z (every comparison with a NaN is false: z is chosen) or, when the z step is 0 (isign(NaN) = 0), never moves: this replays
// intersect_grid's loop -- `stop == 0 && guard > 0`, guard = 3N + 1 -- on an EMPTY block and asserts which of the two exits it takes.
template <int N>
static void check_nan_walk(const float t0[3], const float d[3], const int s[3], bool expect_guard_exit) {
	typedef bm::BrickCell<N> C;
	float t[3] = {t0[0], t0[1], t0[2]};
	const uint32_t first = C::start(3 % N, 1, 0);
	uint32_t cell = first;
	const int inc[3] = {s[0] * C::kStepX, s[1] * C::kStepY, s[2] * C::kStepZ};
	uint32_t stop = 0; // an empty block: only leaving it can stop the walk
	int guard = 3 * N + 1, zmoves = 0;
	for (; stop == 0u && guard > 0; --guard) {
		const bm::StepAxis m = bm::step_choose(t[0], t[1], t[2]);
		if (m.x || m.y || !m.z) { fail("NaN walk", "a NaN tmax chose x or y"); return; }
		cell += static_cast<uint32_t>(bm::step_pick(m, inc[0], inc[1], inc[2]));
		t[0] = bm::step_add(t[0], d[0], m.x);
		t[1] = bm::step_add(t[1], d[1], m.y);
		t[2] = bm::step_add(t[2], d[2], m.z);
		stop = C::outside(cell);
		zmoves++;
	}
	cells_checked++;
	if (expect_guard_exit ? !(guard == 0 && stop == 0u && cell == first) : !(stop != 0u && guard > 0 && zmoves == N))
		fail("NaN walk", "N %d: guard %d stop %x cell %08x after %d moves (expected %s)", N, guard, stop, cell, zmoves, expect_guard_exit ? "the guard to expire" : "an exit through z");
}

static void unit(float dir[3]) {
	const float len = std::sqrt((dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2]);
	for (int i = 0; i < 3; ++i) dir[i] *= 1.0f / len;
}

int main(int argc, char** argv) {
	const long rays = argc > 1 ? std::atol(argv[1]) : 400000;
	const int inc_grid[3] = {1, 64, 64 * 130}, inc_tall[3] = {-1, 256, -256 * 34}; // offset increments of two cube-field pitches, mixed signs

	// 1. random rays, ten moves each (the mixture of tests/jump_check.cpp: near-axis, binary slopes, equal components, zero components)
	for (long ray = 0; ray < rays; ++ray) {
		float dir[3], o[3], t[3], d[3];
		int s[3];
		const uint32_t kind = rnd() % 8;
		for (int i = 0; i < 3; ++i) dir[i] = rndf() * 2.f - 1.f;
		if (kind == 0) dir[rnd() % 3] *= 1e-3f;
		if (kind == 1) { dir[0] = 1.f; dir[1] = 0.5f; dir[2] = 0.25f; }
		if (kind == 2) dir[0] = dir[1];
		if (kind == 3) dir[rnd() % 3] = 0.f;
		if (kind == 7) { dir[0] = dir[1]; dir[2] = rnd() & 1 ? dir[0] : -dir[0]; }
		if ((dir[0] == 0.f && dir[1] == 0.f && dir[2] == 0.f)) continue;
		if (kind != 1) unit(dir);
		for (int i = 0; i < 3; ++i) o[i] = (kind == 5 ? static_cast<float>(rnd() % 100) : rndf() * 100.f) + (kind == 6 ? 0.5f : 0.f);
		setup(o, dir, t, d, s);
		const int inc[3] = {s[0] * (ray & 1 ? inc_grid[0] : inc_tall[0]), s[1] * (ray & 1 ? inc_grid[1] : inc_tall[1]), s[2] * (ray & 1 ? inc_grid[2] : inc_tall[2])};
		check_moves("random", t, d, inc, 10);
	}

	// 2. ties: equal tmax on two and on three axes, every pattern, several magnitudes and deltas
	const float vals[] = {0.f, 0.25f, 1.f, 1.5f, 3.f, 1000.f, 65536.f, 999999.f};
	for (float a : vals) for (float b : vals) for (int pat = 0; pat < 8; ++pat) {
		const float t[3] = {a, pat & 1 ? a : b, pat & 2 ? a : (pat & 4 ? b : a + b)};
		const float d[3] = {1.f + a * 0.125f, 1.f + b * 0.125f, 2.f};
		check_moves("ties", t, d, inc_grid, 12);
		const float d2[3] = {1.f, 1.f, 1.f}; // equal deltas: the ties repeat at every move
		check_moves("ties, equal deltas", t, d2, inc_tall, 12);
	}

	// 3. a zero direction component (tmax = 1e6, tdelta = 0), alone and in pairs, against small and large tmax on the live axes
	for (int zero = 1; zero < 7; ++zero) for (float live : {0.f, 0.5f, 7.f, 999999.f, 1000000.f, 1000001.f}) {
		float t[3], d[3];
		for (int i = 0; i < 3; ++i) { t[i] = (zero >> i) & 1 ? 1000000.f : live + 0.125f * i; d[i] = (zero >> i) & 1 ? 0.f : 1.f + i; }
		check_moves("zero component", t, d, inc_grid, 16);
	}

	// 4. -0.0 and +0.0 start values, in every combination over the axes, with the third value zero / positive
	for (int neg = 0; neg < 8; ++neg) for (int zeros = 1; zeros < 8; ++zeros) {
		float t[3];
		for (int i = 0; i < 3; ++i) t[i] = (zeros >> i) & 1 ? ((neg >> i) & 1 ? -0.0f : 0.0f) : 0.75f;
		const float d[3] = {1.25f, 1.5f, 1.75f};
		check_moves("signed zero", t, d, inc_tall, 8);
	}
	{ // ... and as set-up makes them: an origin on a cell face with a negative direction
		const float o[3] = {5.f, 7.f, 3.25f}, dir0[3] = {-0.6f, -0.8f, 0.f};
		float t[3], d[3];
		int s[3];
		setup(o, dir0, t, d, s);
		if (bits(t[0]) != 0x80000000u) fail("signed zero", "set-up did not produce -0");
		const int inc[3] = {s[0], s[1] * 64, s[2] * 8320};
		check_moves("signed zero (set-up)", t, d, inc, 8);
	}

	// 5. tmax values that straddle a binade end: the last values below 2^k against the first ones above it
	for (int k = -10; k <= 19; ++k) {
		const float p = std::ldexp(1.f, k);
		const float below = std::nextafter(p, 0.f), above = std::nextafter(p, 2.f * p);
		const float cand[] = {below, p, above, std::nextafter(below, 0.f)};
		for (float a : cand) for (float b : cand) for (float c : cand) {
			const float t[3] = {a, b, c};
			const float d[3] = {std::ldexp(1.f, k - 24), std::ldexp(1.5f, k - 23), p}; // below an ulp, an ulp and a half, a whole binade
			check_moves("binade end", t, d, inc_grid, 12);
		}
	}

	// 6. the smallest and the largest tdelta of a unit fp32 direction: 1 (an axis direction) and 2^126 (a component of 2^-126, the
	// smallest normal number)
	for (int big = 0; big < 3; ++big) {
		float dir[3] = {0.6f, 0.8f, 0.6f}, o[3] = {3.5f, 4.25f, 5.75f}, t[3], d[3];
		int s[3];
		dir[big] = std::ldexp(1.f, -126);
		setup(o, dir, t, d, s);
		check_moves("largest tdelta", t, d, inc_grid, 12);
		float axis_dir[3] = {0.f, 0.f, 0.f};
		axis_dir[big] = big == 1 ? -1.f : 1.f;
		setup(o, axis_dir, t, d, s);
		const int inc[3] = {s[0], s[1] * 64, s[2] * 8320};
		check_moves("smallest tdelta", t, d, inc, 12);
	}

	// 7. negative start values (an origin a rounding error outside the box, on an axis the ray moves down)
	for (int k = 0; k < 2000; ++k) {
		float t[3] = {rndf() * 2.f, rndf() * 2.f, rndf() * 2.f};
		t[rnd() % 3] = -rndf() * 1e-3f - 1e-9f;
		if (k & 1) t[rnd() % 3] = -rndf() * 1e-3f - 1e-9f;
		const float d[3] = {1.f + rndf(), 1.f + rndf() * 4.f, 1.f + rndf() * 16.f};
		check_moves("negative start", t, d, inc_tall, 8);
	}

	// 8. the brick walk: every start voxel of an 8^3 brick with all eight octants (and a few directions each), on a random brick;
	// every cell and every move of every walk is compared
	{
		uint32_t words[16];
		for (auto& w : words) w = rnd();
		for (int v = 0; v < 512; ++v) for (int oct = 0; oct < 8; ++oct) for (int rep = 0; rep < 3; ++rep) {
			const int start[3] = {v & 7, (v >> 3) & 7, v >> 6};
			float dir[3] = {rndf() + 1e-3f, rndf() + 1e-3f, rndf() + 1e-3f};
			if (rep == 1) dir[0] = dir[1] = dir[2] = 1.f;                      // the diagonal: three-way ties at every corner
			if (rep == 2) { dir[rnd() % 3] = 0.f; dir[0] += 1e-3f; }           // a zero component
			for (int i = 0; i < 3; ++i) if ((oct >> i) & 1) dir[i] = -dir[i];
			unit(dir);
			float o[3];
			for (int i = 0; i < 3; ++i) o[i] = 8.f * (1 + (rnd() % 100)) + start[i] + (rep == 1 ? (dir[i] < 0.f ? 1.f - 1.f / 64 : 1.f / 64) : rndf());
			const int p[3] = {static_cast<int>(o[0]), static_cast<int>(o[1]), static_cast<int>(o[2])};
			const int st[3] = {p[0] % 8, p[1] % 8, p[2] % 8};
			check_walk<8>("brick walk", st, o, dir, words, 0u);
		}
	}
	// 9. all 512 voxel positions against bricks that have exactly that bit set, and bricks that have every other bit set
	for (int v = 0; v < 512; ++v) for (int inverted = 0; inverted < 2; ++inverted) {
		uint32_t words[16];
		for (int w = 0; w < 16; ++w) words[w] = inverted ? ~0u : 0u;
		words[v >> 5] ^= 1u << (v & 31);
		for (int q = 0; q < 512; ++q) {
			const uint32_t cell = bm::BrickCell<8>::start(q & 7, (q >> 3) & 7, q >> 6);
			const uint32_t got = bm::BrickCell<8>::bit(cell, words[bm::BrickCell<8>::word(cell)]);
			const uint32_t want = static_cast<uint32_t>((q == v) != (inverted != 0));
			cells_checked++;
			if (got != want || (cell & bm::BrickCell<8>::kWordMask) >> 10 != static_cast<uint32_t>(q >> 5)) { fail("single bit", "brick bit %d%s, voxel %d: got %u", v, inverted ? " (inverted)" : "", q, got); break; }
		}
	}
	// 10. the 2^3 LoD walk: every start cell, octant and mask byte
	for (int v = 0; v < 8; ++v) for (int oct = 0; oct < 8; ++oct) for (uint32_t byte = 0; byte < 256; ++byte) {
		const int start[3] = {v & 1, (v >> 1) & 1, v >> 2};
		float dir[3] = {rndf() + 1e-3f, rndf() + 1e-3f, rndf() + 1e-3f};
		if (byte & 1) dir[0] = dir[1] = dir[2] = 1.f;
		for (int i = 0; i < 3; ++i) if ((oct >> i) & 1) dir[i] = -dir[i];
		unit(dir);
		float o[3];
		for (int i = 0; i < 3; ++i) o[i] = 2.f * (1 + (rnd() % 100)) + start[i] + rndf();
		check_walk<2>("LoD walk", start, o, dir, nullptr, byte);
	}

	// 11. field_state: all 256 byte values x both values of "possible", against the rule written out (traverse.h "cube-field walk")
	long states = 0;
	for (uint32_t v = 0; v < 256; ++v) for (int possible = 0; possible < 2; ++possible) {
		uint32_t cube = 0xdeadbeefu;
		const int got = bm::field_state(v, possible != 0, cube);
		int want;
		if (v == 255u) want = bm::ST_NEED;
		else if (v == 0u) want = bm::ST_CAND;
		else if (v >= 4u && possible) want = bm::ST_JUMP;
		else want = bm::ST_OUTER;
		const uint32_t want_cube = possible ? v : (v | 0x100u);
		states++;
		if (got != want || cube != want_cube) fail("field_state", "byte %u possible %d: state %d cube %x, want %d %x", v, possible, got, cube, want, want_cube);
	}

	// 12. NaN: tmax and tdelta with one, two and three NaN components -- flags and bit patterns as the reference's; then the two ways a
	// NaN walk ends (see check_nan_walk)
	{
		const float nan = std::nanf(""), vals3[3] = {0.5f, 2.f, 1000000.f};
		for (int mask = 1; mask < 8; ++mask) { // (finite tdelta: `mask ? delta : 0` is `mask * delta` only there -- steps.h step_add)
			float t[3], d[3];
			for (int i = 0; i < 3; ++i) { t[i] = (mask >> i) & 1 ? nan : vals3[i]; d[i] = 1.f + i; }
			check_moves("NaN tmax", t, d, inc_grid, 8);
		}
		const float all_t[3] = {nan, nan, nan}, all_d[3] = {nan, nan, nan}; // what a NaN direction gives: every tmax and tdelta NaN
		check_moves("NaN direction", all_t, all_d, inc_tall, 8);
		const float tn[3] = {nan, nan, nan}, dn[3] = {nan, nan, nan};
		const int s0[3] = {0, 0, 0};                       // isign(NaN) = 0 on every axis: the cell never moves, the guard ends the loop
		check_nan_walk<8>(tn, dn, s0, true);
		check_nan_walk<2>(tn, dn, s0, true);
		const float tz[3] = {nan, nan, 0.25f}, dz[3] = {nan, nan, 1.5f};
		const int sz[3] = {0, 0, 1};                       // a live z axis: z is chosen every time, the walk leaves after N moves
		check_nan_walk<8>(tz, dz, sz, false);
		check_nan_walk<2>(tz, dz, sz, false);
	}

	std::printf("moves %ld cells %ld states %ld failures %ld\n", moves_checked, cells_checked, states, failures);
	return failures ? 1 : 0;
}
