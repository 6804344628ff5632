// shadowheight_check.cpp -- CPU replay test of brickmap_amd/csrc/shadowheight.h (compiled and run by tests/test_shadowheight_rule.py).
// The plan and the recurrence of the shadow heights are the very functions sunfield.hip builds the table's slice with.  Here small worlds
// get their dark heights from those functions, slab by slab as the kernel does (shadowheight_host.h), and
//   1. the result is compared with the definition, written out a second time below without the header's functions: S of every slab kept,
//      every cell of a column tested for "dark" on its own;
//   2. no cell that the sun plane stamps 255 is dark;
//   3. from random points of EVERY dark cell, rays of the cone are walked cell by cell the way the reference walks them (the move of
//      steps.h, rounded tmax): every one must enter a full cell before it leaves the grid or reaches a 255 stamp.  Cells that are occupied
//      but not full -- partly filled bricks, bricks that are not resident -- let the ray pass: the worst case.
// Usage: shadowheight_check [rays per dark cell].  Prints, per world, how many rays the rule ended; the exit status is 1 if anything failed
// or a world built to cast shadow ended none.  Built with -DBM_SHADOWHEIGHT_LOOSE=1 (the rise's lower bound in place of the upper one) or
// =2 (no margin, a cell dark by its floor) the run must FAIL: a check that a wrong rule passes proves nothing.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../brickmap_amd/csrc/steps.h"
#include "../brickmap_amd/csrc/sunfield_host.h"
#include "../brickmap_amd/csrc/shadowheight_host.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return static_cast<uint32_t>(rng_state >> 32);
}
static float rndf() { return (rnd() >> 8) * (1.0f / 16777216.0f); }

static long failures = 0, violations = 0, rays_ended = 0, dark_cells = 0, slices = 0, zero_slices = 0, barren = 0;
#define FAIL(...) do { if (failures++ < 10) { std::fprintf(stderr, "MISMATCH " __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

struct World {
	int n[3]; // cells along x, y, z
	std::vector<uint8_t> occ, full, plane; // [z][y][x]; full implies occ
	std::vector<int> zd;                   // [y][x]
	World(int xy, int z) : n{xy, xy, z}, occ(static_cast<size_t>(xy) * xy * z, 0), full(occ.size(), 0) {}
	size_t at(int x, int y, int z) const { return (static_cast<size_t>(z) * n[1] + y) * n[0] + x; }
	bool inside(const int c[3]) const { return c[0] >= 0 && c[0] < n[0] && c[1] >= 0 && c[1] < n[1] && c[2] >= 0 && c[2] < n[2]; }
	void set(int x, int y, int z, int v) { if (x >= 0 && x < n[0] && y >= 0 && y < n[1] && z >= 0 && z < n[2]) { occ[at(x, y, z)] = v != 0; full[at(x, y, z)] = v == 2; } } // 0 empty, 1 partly filled, 2 full
};

// ---- the definition, a second time: S[slab][w][b] for every slab, then every cell on its own
static void by_definition(const World& w, const bm::ShadowPlan& p, std::vector<int>& zd) {
	const bm::SunPlan& s = p.sun;
	const int B = bm::kSunBins, U = bm::kSunHeightUnit, nd = w.n[s.dom], n1 = w.n[s.m1], nz = w.n[2];
	zd.assign(static_cast<size_t>(w.n[0]) * w.n[1], 0);
	auto xy = [&](int ud, int u1, int& x, int& y) {
		const int cd = (s.octant >> s.dom & 1) ? nd - 1 - ud : ud, c1 = (s.octant >> s.m1 & 1) ? n1 - 1 - u1 : u1;
		x = s.dom == 0 ? cd : c1; y = s.dom == 0 ? c1 : cd;
	};
	std::vector<int> S(static_cast<size_t>(nd + 1) * n1 * B, 0); // slab nd: outside, 0
	auto Sat = [&](int ud, int u1, int b) { return u1 < n1 ? S[(static_cast<size_t>(ud) * n1 + u1) * B + b] : 0; };
	for (int ud = nd - 1; ud >= 0; --ud)
		for (int u1 = 0; u1 < n1; ++u1) {
			int x, y; xy(ud, u1, x, y);
			int top = 0;
			while (top < nz && w.full[w.at(x, y, top)]) ++top;
			for (int b = 0; b < B; ++b) {
				int least = INT32_MAX;
				for (int g = b + s.lo1; g <= b + s.hi1; ++g) least = std::min(least, Sat(ud + 1, u1 + g / B, g % B) - p.rise_hi);
				S[(static_cast<size_t>(ud) * n1 + u1) * B + b] = std::max(top * U, least);
			}
			int z = 0;
			for (; z < nz; ++z) { // dark: the cell's top, the rise of what is left of the slab and the margin stay below every S it can enter
				bool dark = true;
				for (int g = 0; g <= B - 1 + s.hi1; ++g) dark = dark && (z + 1) * U + p.rise_hi + bm::kShadowMargin < Sat(ud + 1, u1 + g / B, g % B);
				if (!dark) break;
			}
			zd[static_cast<size_t>(y) * w.n[0] + x] = z;
		}
}

// one ray from `origin` (cell units, inside the grid) along `dir`, set up as traverse.h ray_setup does and walked with the move of steps.h:
// true if it enters a full cell before it leaves the grid or stands in a cell stamped 255
static bool reaches_full(const World& w, const float origin[3], const float dir[3]) {
	int c[3] = {static_cast<int>(origin[0]), static_cast<int>(origin[1]), static_cast<int>(origin[2])};
	int sgn[3];
	float t[3], d[3];
	for (int k = 0; k < 3; ++k) {
		sgn[k] = (0.f < dir[k]) - (dir[k] < 0.f);
		const float cb = dir[k] > 0.f ? static_cast<float>(c[k] + 1) : static_cast<float>(c[k]);
		const float r = dir[k] == 0.0f ? 0.0f : 1.f / dir[k];
		t[k] = dir[k] != 0.f ? (cb - origin[k]) * r : 1000000.f;
		d[k] = static_cast<float>(sgn[k]) * r;
	}
	for (int moves = 0; moves < 4096; ++moves) {
		const bm::StepAxis m = bm::step_choose(t[0], t[1], t[2]);
		const int axis = m.x ? 0 : (m.y ? 1 : 2);
		c[axis] += sgn[axis];
		t[0] = bm::step_add(t[0], d[0], m.x); t[1] = bm::step_add(t[1], d[1], m.y); t[2] = bm::step_add(t[2], d[2], m.z);
		if (!w.inside(c)) return false;
		const size_t i = w.at(c[0], c[1], c[2]);
		if (w.full[i]) return true;
		if (w.plane[i] == 255) return false;
	}
	return false;
}

static void normalize(float v[3]) {
	const float l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
	for (int k = 0; k < 3; ++k) v[k] /= l;
}

// a direction of the cone, as traverse.h cone_sample draws it (the frame of frame_plan.cpp)
static void cone_direction(const float axis[3], float extent, float out[3]) {
	float o1[3], o2[3];
	if (std::fabs(axis[0]) > std::fabs(axis[2])) { o1[0] = -axis[1]; o1[1] = axis[0]; o1[2] = 0.f; } else { o1[0] = 0.f; o1[1] = -axis[2]; o1[2] = axis[1]; }
	normalize(o1);
	o2[0] = axis[1] * o1[2] - o1[1] * axis[2]; o2[1] = axis[2] * o1[0] - o1[2] * axis[0]; o2[2] = axis[0] * o1[1] - o1[0] * axis[1];
	normalize(o2);
	const float phi = rndf() * 6.2831853f;
	float ry = 1.0f - rndf() * extent;
	if (rnd() % 2 == 0) ry = 1.0f - extent; // the rim of the cone
	const float om = std::sqrt(1.0f - ry * ry), cs = std::cos(phi), sn = std::sin(phi);
	for (int k = 0; k < 3; ++k) out[k] = (o1[k] * (cs * om) + o2[k] * (sn * om)) + axis[k] * ry;
}

enum Kind { TERRAIN, RIDGE_NOTCH, OVERHANG, HOLLOW, PARTIAL_TOP, EMPTY, KINDS };
static const char* kind_name[KINDS] = {"terrain", "ridge with a notch", "overhang and floating bricks", "hollow mountain", "partly filled top layer", "empty"};

static void fill(World& w, int kind) {
	std::fill(w.occ.begin(), w.occ.end(), 0);
	std::fill(w.full.begin(), w.full.end(), 0);
	const int X = w.n[0], Z = w.n[2];
	auto hills = [&](bool partial_top) {
		const float fx = 0.2f + 0.5f * rndf(), fy = 0.2f + 0.5f * rndf(), ph = 6.f * rndf();
		for (int y = 0; y < X; ++y)
			for (int x = 0; x < X; ++x) {
				const int h = static_cast<int>((0.4f + 0.35f * std::sin(fx * x + ph) * std::cos(fy * y)) * Z + 2.f * rndf());
				for (int z = 0; z < Z && z < h; ++z) w.set(x, y, z, 2);
				if (partial_top && h > 0 && h <= Z) w.set(x, y, h - 1, 1); // the surface brick of every column is partly filled, as a terrain's is
			}
	};
	if (kind == TERRAIN) hills(false);
	else if (kind == PARTIAL_TOP) hills(true);
	else if (kind == RIDGE_NOTCH) { // a full ground layer, a cross of two walls, each cut to the ground by notches one cell wide
		const int top = Z * 3 / 4, wx = X / 2 + static_cast<int>(rnd() % 3) - 1, wy = X / 2 + static_cast<int>(rnd() % 3) - 1;
		for (int y = 0; y < X; ++y) for (int x = 0; x < X; ++x) w.set(x, y, 0, 2);
		for (int k = 0; k < X; ++k) for (int z = 1; z < top; ++z) { w.set(wx, k, z, 2); w.set(k, wy, z, 2); }
		for (int k = 0; k < 3; ++k) {
			const int a = static_cast<int>(rnd() % X), b = static_cast<int>(rnd() % X);
			for (int z = 1; z < top; ++z) { if (a != wy) w.set(wx, a, z, 0); if (b != wx) w.set(b, wy, z, 0); }
		}
	} else if (kind == OVERHANG) { // hills, slabs that float beside them, and full bricks above a gap (which count for nothing)
		hills(false);
		for (int k = 0; k < 6; ++k) {
			const int x0 = static_cast<int>(rnd() % X), y0 = static_cast<int>(rnd() % X), z0 = Z / 2 + static_cast<int>(rnd() % (Z / 2));
			for (int y = y0; y < y0 + 5; ++y) for (int x = x0; x < x0 + 5; ++x) w.set(x, y, z0, 2);
		}
		for (int k = 0; k < 8; ++k) { // a gap cut into a column: what is above it no longer counts
			const int x = static_cast<int>(rnd() % X), y = static_cast<int>(rnd() % X);
			w.set(x, y, 1 + static_cast<int>(rnd() % 3), k & 1);
		}
	} else if (kind == HOLLOW) { // a mountain whose inside is empty above a full floor: a full shell one cell thick
		const int c = X / 2, r = X / 3, top = Z * 3 / 4;
		for (int y = 0; y < X; ++y) for (int x = 0; x < X; ++x) w.set(x, y, 0, 2);
		for (int y = c - r; y <= c + r; ++y)
			for (int x = c - r; x <= c + r; ++x)
				for (int z = 1; z <= top; ++z) {
					const bool shell = x == c - r || x == c + r || y == c - r || y == c + r || z == top;
					if (shell) w.set(x, y, z, 2);
				}
	}
}

int main(int argc, char** argv) {
	const int per_cell = argc > 1 ? std::atoi(argv[1]) : 6;
	const float narrow = 1.0f - std::cos(1.5f * 3.14159265f / 180.f), wide = 1.0f - std::cos(5.f * 3.14159265f / 180.f);
	struct Sun { float dir[3]; float extent; bool heights; const char* name; };
	Sun suns[] = {
		{{-0.904f, -0.294f, 0.310f}, narrow, true, "x dominant, octant 3"},
		{{0.80f, -0.50f, 0.33f}, narrow, true, "x dominant, octant 2"},
		{{0.30f, 0.85f, 0.43f}, narrow, true, "y dominant, octant 0"},
		{{-0.45f, 0.75f, 0.48f}, wide, true, "y dominant, octant 1, wide cone"},
		{{0.95f, 0.30f, 0.08f}, narrow, true, "x dominant, very low sun"},
		{{0.25f, -0.35f, 0.90f}, narrow, false, "z dominant"},
		{{0.90f, 0.01f, 0.43f}, narrow, false, "cone across the y = 0 octant boundary"},
	};
	const int dims[3][2] = {{16, 16}, {32, 16}, {16, 32}};
	for (Sun& s : suns) {
		normalize(s.dir);
		const bm::ShadowPlan p = bm::shadow_plan(s.dir, s.extent);
		if ((p.valid != 0) != s.heights) { FAIL("(%s) shadow plan valid = %d", s.name, p.valid); continue; }
		if (p.valid && !(p.rise_hi > p.sun.rise || BM_SHADOWHEIGHT_LOOSE == 1)) FAIL("(%s) rise %d .. %d", s.name, p.sun.rise, p.rise_hi);
		for (int dm = 0; dm < 3; ++dm)
			for (int kind = 0; kind < KINDS; ++kind) {
				World w(dims[dm][0], dims[dm][1]);
				fill(w, kind);
				bm::shadow_heights_host(p, w.n, w.full, w.zd);
				++slices;
				if (!p.valid) { // no shadow heights for this sun: the slice is zero
					for (int v : w.zd) if (v != 0) { FAIL("(%s) a dark height without a plan", s.name); break; }
					++zero_slices;
					continue;
				}
				std::vector<int> want;
				by_definition(w, p, want);
				if (want != w.zd) FAIL("(%s, %s) the slab-by-slab build differs from the definition", s.name, kind_name[kind]);
				bm::sun_plane_host(p.sun, w.n, w.occ, w.plane);
				long ended = 0, bad = 0;
				for (int y = 0; y < w.n[1]; ++y)
					for (int x = 0; x < w.n[0]; ++x)
						for (int z = 0; z < w.zd[static_cast<size_t>(y) * w.n[0] + x]; ++z) {
							++dark_cells;
							if (w.plane[w.at(x, y, z)] == 255) FAIL("(%s, %s) dark cell %d %d %d is stamped 255", s.name, kind_name[kind], x, y, z);
							for (int i = 0; i < per_cell; ++i) {
								float o[3], dir[3];
								cone_direction(s.dir, s.extent, dir);
								const int c[3] = {x, y, z};
								for (int k = 0; k < 3; ++k) {
									o[k] = static_cast<float>(c[k]) + rndf();
									if (i % 3 == 1 && (rnd() & 1)) o[k] = static_cast<float>(c[k]);                      // on the cell's lower face
									if (i % 3 == 2 && (rnd() & 1)) o[k] = std::nextafter(static_cast<float>(c[k] + 1), 0.f); // just below its upper one
									if (static_cast<int>(o[k]) != c[k]) o[k] = static_cast<float>(c[k]) + 0.5f;
								}
								++ended;
								if (!reaches_full(w, o, dir)) {
									if (bad++ == 0 && violations < 5) std::fprintf(stderr, "VIOLATION (%s, %s) from %g %g %g along %g %g %g\n", s.name, kind_name[kind], o[0], o[1], o[2], dir[0], dir[1], dir[2]);
								}
							}
						}
				std::printf("%-40s %-30s %2d x %2d x %2d: %6ld rays ended, %ld violations\n", s.name, kind_name[kind], w.n[0], w.n[1], w.n[2], ended, bad);
				rays_ended += ended;
				violations += bad;
				if (kind != EMPTY && ended == 0) { ++barren; std::fprintf(stderr, "BARREN (%s, %s): a world built to cast shadow ended no ray\n", s.name, kind_name[kind]); }
				if (kind == EMPTY && ended != 0) FAIL("(%s) dark cells in an empty world", s.name);
			}
	}
	std::printf("slices %ld zero_slices %ld dark_cells %ld rays_ended %ld violations %ld barren %ld failures %ld\n", slices, zero_slices, dark_cells, rays_ended, violations, barren, failures);
	return failures || violations || barren ? 1 : 0;
}
