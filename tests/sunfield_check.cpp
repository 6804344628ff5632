// sunfield_check.cpp -- CPU replay test of brickmap_amd/csrc/sunfield.h (compiled and run by tests/test_sunfield_rule.py).
// The plan of a sun and the recurrences of the sun plane are the very functions sunfield.hip builds the plane with.  Here small worlds
// get their plane from those functions, slab by slab as the kernels do, and rays of the cone are walked cell by cell the way the
// reference walks them (the move of steps.h) from random points until they leave the grid.  In every cell a ray visits:
//   byte 0 exactly where the cell is occupied; from a cell of byte 255 the rest of the walk meets no occupied cell; from a cell of byte n
//   (1 ... 254) no occupied cell is entered before one of the axes has moved n cells.
// Usage: sunfield_check [rays per sun].  Prints counters; the exit status is the number of failures (capped).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../brickmap_amd/csrc/steps.h"
#include "../brickmap_amd/csrc/sunfield_host.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return static_cast<uint32_t>(rng_state >> 32);
}
static float rndf() { return (rnd() >> 8) * (1.0f / 16777216.0f); }

static long failures = 0, rays_walked = 0, cells_walked = 0, rays_stamped = 0, planes = 0, invalid = 0, long_bytes = 0;
#define FAIL(...) do { if (failures++ < 10) { std::fprintf(stderr, "MISMATCH " __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

struct World {
	int n[3]; // cells along x, y, z
	std::vector<uint8_t> occ, plane; // [z][y][x]
	World(int xy, int z) : n{xy, xy, z}, occ(static_cast<size_t>(xy) * xy * z, 0) {}
	size_t at(int x, int y, int z) const { return (static_cast<size_t>(z) * n[1] + y) * n[0] + x; }
	bool inside(const int c[3]) const { return c[0] >= 0 && c[0] < n[0] && c[1] >= 0 && c[1] < n[1] && c[2] >= 0 && c[2] < n[2]; }

	// the plane, slab by slab from the far end of the dominant axis, as sunfield.hip builds it (sunfield_host.h)
	void build(const bm::SunPlan& p) {
		bm::sun_plane_host(p, n, occ, plane);
		++planes;
	}
};

// one ray from `origin` (cell units, inside the grid) along `dir`, set up as traverse.h ray_setup does and walked with the move of steps.h
static void walk(const World& w, const float origin[3], const float dir[3], const char* what) {
	int c[3] = {static_cast<int>(origin[0]), static_cast<int>(origin[1]), static_cast<int>(origin[2])};
	if (!w.inside(c)) return;
	int sgn[3];
	float t[3], d[3];
	for (int k = 0; k < 3; ++k) {
		sgn[k] = (0.f < dir[k]) - (dir[k] < 0.f);
		const float cb = dir[k] > 0.f ? static_cast<float>(c[k] + 1) : static_cast<float>(c[k]);
		const float r = dir[k] == 0.0f ? 0.0f : 1.f / dir[k];
		t[k] = dir[k] != 0.f ? (cb - origin[k]) * r : 1000000.f;
		d[k] = static_cast<float>(sgn[k]) * r;
	}
	struct Visit { uint8_t occupied, byte, axis; }; // axis: of the move that LEAVES the cell
	std::vector<Visit> path;
	while (w.inside(c)) {
		const size_t i = w.at(c[0], c[1], c[2]);
		const bm::StepAxis m = bm::step_choose(t[0], t[1], t[2]);
		const int axis = m.x ? 0 : (m.y ? 1 : 2);
		path.push_back({w.occ[i], w.plane[i], static_cast<uint8_t>(axis)});
		c[axis] += sgn[axis];
		t[0] = bm::step_add(t[0], d[0], m.x); t[1] = bm::step_add(t[1], d[1], m.y); t[2] = bm::step_add(t[2], d[2], m.z);
		if (sgn[axis] == 0 || path.size() > 4096) { FAIL("(%s) walk does not end", what); return; }
	}
	++rays_walked;
	cells_walked += static_cast<long>(path.size());
	bool stamped = false;
	for (size_t i = 0; i < path.size(); ++i) {
		const Visit& v = path[i];
		if ((v.byte == 0) != (v.occupied != 0)) { FAIL("(%s) byte %d in a cell that is %s", what, v.byte, v.occupied ? "occupied" : "empty"); return; }
		if (stamped && v.occupied) { FAIL("(%s) occupied cell %zu cells into the walk, behind a 255 cell (dir %g %g %g)", what, i, dir[0], dir[1], dir[2]); return; }
		if (v.byte == 255) stamped = true;
		if (v.byte == 0 || v.byte == 255) continue;
		if (v.byte >= 4) ++long_bytes;
		int moved[3] = {0, 0, 0};
		for (size_t j = i; j + 1 < path.size(); ++j) { // cells entered before an axis has moved `byte` cells
			if (++moved[path[j].axis] >= v.byte) break;
			if (path[j + 1].occupied) {
				FAIL("(%s) byte %d, but an occupied cell after moves (%d, %d, %d) (dir %g %g %g)", what, v.byte, moved[0], moved[1], moved[2], dir[0], dir[1], dir[2]);
				return;
			}
		}
	}
	if (stamped) ++rays_stamped;
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
	if (rnd() % 4 == 0) ry = 1.0f - extent; // the rim of the cone
	const float om = std::sqrt(1.0f - ry * ry), cs = std::cos(phi), sn = std::sin(phi);
	for (int k = 0; k < 3; ++k) out[k] = (o1[k] * (cs * om) + o2[k] * (sn * om)) + axis[k] * ry;
}

static void fill(World& w, int kind) {
	std::fill(w.occ.begin(), w.occ.end(), 0);
	const int X = w.n[0], Z = w.n[2];
	if (kind == 0) { // random, sparse to a fifth full
		const uint32_t density = 2u + rnd() % 50u;
		for (auto& v : w.occ) v = (rnd() & 255u) < density;
	} else if (kind == 1 || kind == 2) { // terrain: smooth hills, columns filled from the ground; kind 2: with overhangs (slabs that float beside a hill)
		const float fx = 0.2f + 0.5f * rndf(), fy = 0.2f + 0.5f * rndf(), ph = 6.f * rndf();
		for (int y = 0; y < X; ++y)
			for (int x = 0; x < X; ++x) {
				const float h = (0.35f + 0.3f * std::sin(fx * x + ph) * std::cos(fy * y)) * Z + 2.f * rndf();
				for (int z = 0; z < Z && z < static_cast<int>(h); ++z) w.occ[w.at(x, y, z)] = 1;
			}
		if (kind == 2)
			for (int k = 0; k < 6; ++k) {
				const int x0 = static_cast<int>(rnd() % X), y0 = static_cast<int>(rnd() % X), z0 = Z / 2 + static_cast<int>(rnd() % (Z / 2));
				for (int y = y0; y < X && y < y0 + 5; ++y) for (int x = x0; x < X && x < x0 + 5; ++x) w.occ[w.at(x, y, z0)] = 1;
			}
	} else { // a single floating brick
		w.occ[w.at(static_cast<int>(rnd() % X), static_cast<int>(rnd() % X), static_cast<int>(rnd() % Z))] = 1;
	}
}

int main(int argc, char** argv) {
	const long per_sun = argc > 1 ? std::atol(argv[1]) : 100000;
	const float narrow = 1.0f - std::cos(1.5f * 3.14159265f / 180.f), wide = 1.0f - std::cos(5.f * 3.14159265f / 180.f);
	struct Sun { float dir[3]; float extent; bool valid; const char* name; };
	Sun suns[] = {
		{{-0.904f, -0.294f, 0.310f}, narrow, true, "x dominant, octant 3"},
		{{0.80f, -0.50f, 0.33f}, narrow, true, "x dominant, octant 2"},
		{{0.30f, 0.85f, 0.43f}, narrow, true, "y dominant, octant 0"},
		{{-0.45f, 0.75f, 0.48f}, wide, true, "y dominant, octant 1, wide cone"},
		{{0.25f, -0.35f, 0.90f}, narrow, true, "z dominant, octant 2"},
		{{-0.30f, -0.20f, 0.93f}, wide, true, "z dominant, octant 3, wide cone"},
		{{0.95f, 0.30f, 0.08f}, narrow, true, "very low sun"},
		{{0.90f, 0.01f, 0.43f}, narrow, false, "cone across the y = 0 octant boundary"},
		{{0.70f, 0.50f, -0.50f}, narrow, false, "sun below the horizon"},
		{{0.60f, 0.59f, 0.54f}, narrow, false, "a minor slope reaches 1"},
	};
	const int dims[3][2] = {{16, 16}, {32, 16}, {16, 32}};
	for (Sun& s : suns) {
		normalize(s.dir);
		const bm::SunPlan p = bm::sun_plan(s.dir, s.extent);
		if ((p.valid != 0) != s.valid) { FAIL("(%s) plan valid = %d", s.name, p.valid); continue; }
		if (!p.valid) { ++invalid; continue; }
		if (p.lo1 > p.hi1 || p.lo2 > p.hi2 || p.hi1 > bm::kSunBins || p.hi2 > bm::kSunBins || p.hi1 < 1 || p.hi2 < 1) FAIL("(%s) bins %d..%d, %d..%d", s.name, p.lo1, p.hi1, p.lo2, p.hi2);
		const long per_world = per_sun / 12 + 1;
		for (int dm = 0; dm < 3; ++dm)
			for (int kind = 0; kind < 4; ++kind) {
				World w(dims[dm][0], dims[dm][1]);
				fill(w, kind);
				w.build(p);
				for (long i = 0; i < per_world; ++i) {
					float o[3], dir[3];
					cone_direction(s.dir, s.extent, dir);
					for (int k = 0; k < 3; ++k) {
						o[k] = rndf() * static_cast<float>(w.n[k]);
						if (i % 4 == 3 && (rnd() & 1)) o[k] = static_cast<float>(rnd() % static_cast<uint32_t>(w.n[k])); // on a cell face
						if (!(o[k] < static_cast<float>(w.n[k]))) o[k] = static_cast<float>(w.n[k]) - 0.5f;
					}
					if (i % 3 == 0) o[2] *= 0.5f; // more starts near the ground
					walk(w, o, dir, s.name);
				}
			}
	}
	std::printf("rays %ld cells %ld stamped %ld long_bytes %ld planes %ld invalid %ld failures %ld\n", rays_walked, cells_walked, rays_stamped, long_bytes, planes, invalid, failures);
	return failures ? 1 : 0;
}
