// shadow_origin_check.cpp -- CPU test of bm::shadow_origin (brickmap_amd/csrc/shadowheight.h), compiled and run by tests/test_shadow_origin_rule.py.
// The shade block of trace.hip decides with that function whether a shadow ray is drawn at all: it must name the very cell ray_setup would start
// the ray in, and be undecided wherever ray_setup would not take its short way.
//   1. The function against its definition, written out a second time below in double precision and 64-bit integers, for origins whose
//      coordinates come from a list of hard values -- 0 and -0, exact multiples of 8 and their fp32 neighbours, the grid's size and height and
//      one ulp either side, negative values, denormals, infinities, NaN -- mixed with random interior points, in worlds of 16^3, 32 x 32 x 16
//      and 16 x 16 x 32 cells.
//   2. A slice built with the functions of shadowheight_host.h, as the kernel's table is; from random origins that the function calls dark
//      against that slice, rays of the cone are set up the way ray_setup sets them up (origin / 8) and walked cell by cell with the move of steps.h
//      (the reference's rounded tmax): every one must enter a full cell before it leaves the grid.
// Usage: shadow_origin_check [origins per world for part 1, in thousands].  The last line holds the counts; exit status 1 if anything failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../brickmap_amd/csrc/steps.h"
#include "../brickmap_amd/csrc/sunfield_host.h"
#include "../brickmap_amd/csrc/shadowheight_host.h"

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return static_cast<uint32_t>(rng_state >> 32);
}
static float rndf() { return (rnd() >> 8) * (1.0f / 16777216.0f); }

static long failures = 0, origins = 0, decided = 0, undecided = 0, dark_origins = 0, rays = 0, violations = 0;
#define FAIL(...) do { if (failures++ < 10) { std::fprintf(stderr, "MISMATCH " __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

struct Layout {
	int cells, cells_h, shift;
	float size, height;
	uint32_t pxy, plane;
	Layout(int c, int ch) : cells(c), cells_h(ch), shift(0), size(8.f * c), height(8.f * ch) {
		while ((1 << shift) < c + 2) ++shift; // rows padded to a power of two (device_types.h)
		pxy = static_cast<uint32_t>(c + 2) << shift;
		plane = static_cast<uint32_t>(ch + 2) * pxy;
	}
};

// ---- the definition, a second time: no float division, no float-to-int conversion, no 32-bit offsets
static bool by_definition(const Layout& l, const float o[3], uint64_t& entry, uint64_t& cell) {
	const double lim[3] = {l.size, l.size, l.height};
	const int n[3] = {l.cells, l.cells, l.cells_h};
	long long c[3];
	for (int k = 0; k < 3; ++k) {
		if (std::isnan(o[k]) || o[k] <= 0.f || static_cast<double>(o[k]) >= lim[k]) return false; // not strictly inside the box
		c[k] = static_cast<long long>(std::floor(static_cast<double>(o[k]) / 8.0));                  // (o / 8.f is exact for every float but a denormal, whose cell is 0 either way)
		if (c[k] < 0 || c[k] >= n[k]) return false;
	}
	const uint64_t column = (static_cast<uint64_t>(c[1] + 1) << l.shift) + static_cast<uint64_t>(c[0] + 1);
	entry = 8ull * l.pxy + column;
	cell = 8ull * l.plane + static_cast<uint64_t>(c[2] + 1) * l.pxy + column;
	return true;
}

static bm::ShadowOrigin rule(const Layout& l, const float o[3]) {
	return bm::shadow_origin(l.size, l.height, l.cells, l.cells_h, l.shift, l.pxy, 8u * l.plane, o[0], o[1], o[2]);
}

static void check_origin(const Layout& l, const float o[3]) {
	uint64_t entry = 0, cell = 0;
	const bool want = by_definition(l, o, entry, cell);
	const bm::ShadowOrigin so = rule(l, o);
	++origins;
	if (want != !bm::shadow_undecided(so)) { FAIL("origin %a %a %a in %d x %d x %d: decided %d, definition %d", o[0], o[1], o[2], l.cells, l.cells, l.cells_h, !bm::shadow_undecided(so), want); return; }
	if (!want) {
		++undecided;
		if (so.entry != 0u || so.cell != bm::kShadowUndecided) FAIL("undecided origin %a %a %a: entry %u cell %u", o[0], o[1], o[2], so.entry, so.cell);
		return;
	}
	++decided;
	if (so.entry != entry || so.cell != cell) FAIL("origin %a %a %a: entry %u cell %u, definition %llu %llu", o[0], o[1], o[2], so.entry, so.cell, static_cast<unsigned long long>(entry), static_cast<unsigned long long>(cell));
	if (so.entry >= 9ull * l.pxy || so.cell >= 9ull * l.plane) FAIL("origin %a %a %a: entry or cell outside its table", o[0], o[1], o[2]);
}

// hard values of one coordinate whose box is (0, limit)
static std::vector<float> hard_values(float limit) {
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), den = std::numeric_limits<float>::denorm_min();
	std::vector<float> v = {0.f, -0.f, den, -den, std::numeric_limits<float>::min(), 1e-30f, -1e-30f, -1.f, -8.f, -limit, -1e30f, inf, -inf, nan, -nan, 1e30f, 2.f * limit,
							limit, std::nextafter(limit, 0.f), std::nextafter(limit, inf), limit - 8.f, std::nextafter(limit - 8.f, 0.f), std::nextafter(limit - 8.f, inf)};
	for (float m = 8.f; m < limit; m += 8.f) { v.push_back(m); v.push_back(std::nextafter(m, 0.f)); v.push_back(std::nextafter(m, inf)); }
	return v;
}

static void part_one(const Layout& l, long count) {
	const std::vector<float> hx = hard_values(l.size), hz = hard_values(l.height);
	// every hard value on every axis, the other two coordinates inside
	for (int axis = 0; axis < 3; ++axis)
		for (float h : axis == 2 ? hz : hx) {
			float o[3] = {0.3f * l.size, 0.6f * l.size, 0.5f * l.height};
			o[axis] = h;
			check_origin(l, o);
		}
	for (long i = 0; i < count; ++i) {
		float o[3];
		for (int k = 0; k < 3; ++k) {
			const float lim = k == 2 ? l.height : l.size;
			const std::vector<float>& h = k == 2 ? hz : hx;
			const uint32_t pick = rnd() % 8u;
			if (pick < 4u) o[k] = rndf() * lim;                               // a random interior point
			else if (pick < 7u) o[k] = h[rnd() % h.size()];                   // a hard value
			else o[k] = (rndf() * 3.f - 1.f) * lim;                           // anywhere from one box below to one above
		}
		check_origin(l, o);
	}
}

// ---- part 2: a world, its slice, and the walk
struct World {
	int n[3];
	std::vector<uint8_t> occ, full; // [z][y][x]
	std::vector<int> zd;
	World(int xy, int z) : n{xy, xy, z}, occ(static_cast<size_t>(xy) * xy * z, 0), full(occ.size(), 0) {}
	size_t at(int x, int y, int z) const { return (static_cast<size_t>(z) * n[1] + y) * n[0] + x; }
};

// hills of full cells under a partly filled surface cell, and two full walls across the world: shadow for every sun below
static void fill(World& w) {
	const float fx = 0.2f + 0.5f * rndf(), fy = 0.2f + 0.5f * rndf(), ph = 6.f * rndf();
	for (int y = 0; y < w.n[1]; ++y)
		for (int x = 0; x < w.n[0]; ++x) {
			int h = static_cast<int>((0.35f + 0.25f * std::sin(fx * x + ph) * std::cos(fy * y)) * w.n[2]);
			if (x == w.n[0] / 2 || y == w.n[1] / 2) h = w.n[2] * 3 / 4;
			for (int z = 0; z < w.n[2] && z < h; ++z) { w.occ[w.at(x, y, z)] = 1; w.full[w.at(x, y, z)] = 1; }
			if (h > 0 && h <= w.n[2] && x != w.n[0] / 2 && y != w.n[1] / 2) w.full[w.at(x, y, h - 1)] = 0; // the surface brick is partly filled: occupied, not full
		}
}

// the ray of traverse.h ray_setup from an origin strictly inside the box (voxel units), walked with the move of steps.h: does it enter a full cell before
// it leaves the grid?  first_cell: the cell the set-up starts in
static bool reaches_full(const World& w, const float origin_voxels[3], const float dir[3], int first_cell[3]) {
	float o[3], t[3], d[3];
	int c[3], sgn[3];
	for (int k = 0; k < 3; ++k) {
		o[k] = origin_voxels[k] / 8.f;
		c[k] = static_cast<int>(o[k]);
		first_cell[k] = c[k];
		sgn[k] = (0.f < dir[k]) - (dir[k] < 0.f);
		const float cb = dir[k] > 0.f ? static_cast<float>(c[k] + 1) : static_cast<float>(c[k]);
		const float r = dir[k] == 0.0f ? 0.0f : 1.f / dir[k];
		t[k] = dir[k] != 0.f ? (cb - o[k]) * r : 1000000.f;
		d[k] = static_cast<float>(sgn[k]) * r;
	}
	for (int moves = 0; moves < 4096; ++moves) {
		const bm::StepAxis m = bm::step_choose(t[0], t[1], t[2]);
		const int axis = m.x ? 0 : (m.y ? 1 : 2);
		c[axis] += sgn[axis];
		t[0] = bm::step_add(t[0], d[0], m.x); t[1] = bm::step_add(t[1], d[1], m.y); t[2] = bm::step_add(t[2], d[2], m.z);
		for (int k = 0; k < 3; ++k) if (c[k] < 0 || c[k] >= w.n[k]) return false;
		if (w.full[w.at(c[0], c[1], c[2])]) return true;
	}
	return false;
}

static void normalize(float v[3]) {
	const float l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
	for (int k = 0; k < 3; ++k) v[k] /= l;
}

// a direction of the cone around `axis`: axis * (1 - u * extent) + a perpendicular of the matching length; half of them on the rim
static void cone_direction(const float axis[3], float extent, float out[3]) {
	float o1[3], o2[3];
	if (std::fabs(axis[0]) > std::fabs(axis[2])) { o1[0] = -axis[1]; o1[1] = axis[0]; o1[2] = 0.f; } else { o1[0] = 0.f; o1[1] = -axis[2]; o1[2] = axis[1]; }
	normalize(o1);
	o2[0] = axis[1] * o1[2] - o1[1] * axis[2]; o2[1] = axis[2] * o1[0] - o1[2] * axis[0]; o2[2] = axis[0] * o1[1] - o1[0] * axis[1];
	normalize(o2);
	const float phi = rndf() * 6.2831853f;
	const float ry = (rnd() & 1u) ? 1.0f - extent : 1.0f - rndf() * extent;
	const float om = std::sqrt(1.0f - ry * ry), cs = std::cos(phi), sn = std::sin(phi);
	for (int k = 0; k < 3; ++k) out[k] = (o1[k] * (cs * om) + o2[k] * (sn * om)) + axis[k] * ry;
}

static void part_two(const Layout& l, const float sun[3], float extent, long tries) {
	World w(l.cells, l.cells_h);
	fill(w);
	const bm::ShadowPlan p = bm::shadow_plan(sun, extent);
	if (!p.valid) { FAIL("no shadow plan for the sun %g %g %g", sun[0], sun[1], sun[2]); return; }
	bm::shadow_heights_host(p, w.n, w.full, w.zd);
	// the table's slice as the device holds it: 9 * pxy entries, slice 8 filled with shadow_entry, everything else zero
	std::vector<uint32_t> table(9u * static_cast<size_t>(l.pxy), 0u);
	for (int y = 0; y < l.cells; ++y)
		for (int x = 0; x < l.cells; ++x)
			table[8u * static_cast<size_t>(l.pxy) + (static_cast<size_t>(y + 1) << l.shift) + static_cast<size_t>(x + 1)] = bm::shadow_entry(8u * l.plane, l.pxy, w.zd[static_cast<size_t>(y) * l.cells + x]);
	long dark_here = 0;
	for (long i = 0; i < tries; ++i) {
		float o[3];
		for (int k = 0; k < 3; ++k) {
			const float lim = k == 2 ? l.height : l.size;
			o[k] = rndf() * lim;
			const uint32_t pick = rnd() % 8u; // cell faces, from either side: where the origin's cell and its neighbour's differ
			const float face = 8.f * static_cast<float>(1 + rnd() % static_cast<uint32_t>((k == 2 ? l.cells_h : l.cells) - 1));
			if (pick == 0u) o[k] = face;
			if (pick == 1u) o[k] = std::nextafter(face, 0.f);
		}
		const bm::ShadowOrigin so = rule(l, o);
		if (bm::shadow_undecided(so) || !(so.cell < table[so.entry])) continue;
		++dark_here;
		float dir[3];
		int first[3];
		cone_direction(sun, extent, dir);
		++rays;
		const bool ok = reaches_full(w, o, dir, first);
		// the cell the rule tested is the cell the walk starts in, and it is one of the column's dark cells
		const uint32_t walk_cell = 8u * l.plane + static_cast<uint32_t>(first[2] + 1) * l.pxy + (static_cast<uint32_t>(first[1] + 1) << l.shift) + static_cast<uint32_t>(first[0] + 1);
		if (walk_cell != so.cell) FAIL("origin %a %a %a: the rule's cell %u is not the walk's %u", o[0], o[1], o[2], so.cell, walk_cell);
		else if (first[2] >= w.zd[static_cast<size_t>(first[1]) * l.cells + first[0]]) FAIL("origin %a %a %a: called dark above its column's dark height", o[0], o[1], o[2]);
		if (!ok && violations++ < 5) std::fprintf(stderr, "VIOLATION from %g %g %g along %g %g %g\n", o[0], o[1], o[2], dir[0], dir[1], dir[2]);
	}
	dark_origins += dark_here;
	std::printf("%2d x %2d x %2d, sun %5.2f %5.2f %5.2f: %ld of %ld origins dark\n", l.cells, l.cells, l.cells_h, sun[0], sun[1], sun[2], dark_here, tries);
	if (dark_here * 20 < tries) FAIL("a world built to cast shadow has too few dark origins (%ld of %ld)", dark_here, tries);
}

int main(int argc, char** argv) {
	const long thousands = argc > 1 ? std::atol(argv[1]) : 400;
	const int dims[3][2] = {{16, 16}, {32, 16}, {16, 32}};
	const float narrow = 1.0f - std::cos(1.5f * 3.14159265f / 180.f);
	float suns[3][3] = {{-0.904f, -0.294f, 0.310f}, {0.30f, 0.85f, 0.43f}, {0.95f, 0.30f, 0.08f}}; // x dominant, y dominant, a very low sun
	for (auto& s : suns) normalize(s);
	for (const auto& dm : dims) {
		const Layout l(dm[0], dm[1]);
		part_one(l, thousands * 1000);
		for (const auto& s : suns) part_two(l, s, narrow, 20000);
	}
	std::printf("origins %ld decided %ld undecided %ld dark_origins %ld rays %ld violations %ld failures %ld\n", origins, decided, undecided, dark_origins, rays, violations, failures);
	return failures || violations ? 1 : 0;
}
