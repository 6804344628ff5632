// view_check.cpp -- CPU replay test of brickmap_amd/csrc/viewfield.h (compiled and run by tests/test_view_rule.py).
// The plan of a camera position and the rule of a cell's byte are the very functions viewfield.hip builds the view plane with.  Here
// small worlds get their plane from those functions (viewfield_host.h), the plane is compared with the rule written out a second time
// (second_byte below: a predicate per cell instead of rectangles per face), and rays from the camera's position are walked cell by
// cell the way the reference walks them (ray_setup's tmax, the move of steps.h) until they leave the grid.  In every cell a ray visits:
//   byte 0 exactly where the cell is occupied; from a cell of byte 255 the rest of the walk meets no occupied cell; from a cell of byte n
//   (1 ... 254) every cell entered before one of the axes has moved n cells is empty and inside the grid.
// Usage: view_check [rays per position]            the test: prints counters; the exit status is the number of failures (capped)
//        view_check plane <in> <out>                the plane of one world: in = int32 n[3], float32 origin[3] (voxels), float32 lens_radius,
//                                                   then n[0] * n[1] * n[2] occupancy bytes [z][y][x]; out = the plane's bytes, none if no plan
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../brickmap_amd/csrc/steps.h"
#include "../brickmap_amd/csrc/viewfield_host.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return static_cast<uint32_t>(rng_state >> 32);
}
static float rndf() { return (rnd() >> 8) * (1.0f / 16777216.0f); }

static long failures = 0, rays_walked = 0, cells_walked = 0, planes = 0, refused = 0, longer = 0;
static long seen_n = 0, seen_255 = 0, seen_0 = 0; // visited cells per class, of the world in hand
#define FAIL(...) do { if (failures++ < 10) { std::fprintf(stderr, "MISMATCH " __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

struct World {
	int n[3]; // cells along x, y, z
	std::vector<uint8_t> occ, plane; // [z][y][x]
	World(int xy, int z) : n{xy, xy, z}, occ(static_cast<size_t>(xy) * xy * z, 0) {}
	size_t at(int x, int y, int z) const { return (static_cast<size_t>(z) * n[1] + y) * n[0] + x; }
	bool inside(const int c[3]) const { return c[0] >= 0 && c[0] < n[0] && c[1] >= 0 && c[1] < n[1] && c[2] >= 0 && c[2] < n[2]; }
	void set(int x, int y, int z, int v = 1) { const int c[3] = {x, y, z}; if (inside(c)) occ[at(x, y, z)] = static_cast<uint8_t>(v); }
	int top(int x, int y) const { int t = -1; for (int z = 0; z < n[2]; ++z) if (occ[at(x, y, z)]) t = z; return t; }
};

// ---- the rule a second time: the largest n such that every cell of the cube of edge n, outside the known-empty octant cube, that the
// pencil can touch is empty and inside the grid.  A cell at directed offsets u, j = max(u), is touched if for a face a with u_a = j the
// pencil's interval along both other axes overlaps the cell's.
static int second_byte(const bm::ViewPlan& v, const bm::ViewHostField& f, const int c[3]) {
	int amb = 0, oct = 0;
	for (int k = 0; k < 3; ++k) { if (c[k] == v.cell[k]) amb |= 1 << k; else if (c[k] < v.cell[k]) oct |= 1 << k; }
	int n0 = 254;
	bool escaped = true;
	for (int o = 0; o < 8; ++o) {
		if ((o | amb) != (oct | amb)) continue;
		const int b = f.cube[o][f.at(c[0], c[1], c[2])], e = f.threshold(o, v.cell[0], v.cell[1]);
		if (b < n0) n0 = b;
		if ((o & 4) ? !(c[2] < e) : !(c[2] > e)) escaped = false;
	}
	if (n0 == 0) return 0;
	if (escaped) return 255;
	if (amb) return n0;
	const double m = v.margin;
	double l[3], h[3], nr[3];
	int s[3];
	for (int k = 0; k < 3; ++k) {
		s[k] = (oct >> k & 1) ? -1 : 1;
		nr[k] = s[k] > 0 ? c[k] - v.p[k] : v.p[k] - (c[k] + 1);
		l[k] = nr[k] - m; h[k] = nr[k] + 1.0 + m;
		if (!(l[k] > 0.0)) return n0;
	}
	auto touched = [&](const int u[3], int j) {
		for (int a = 0; a < 3; ++a) {
			if (u[a] != j) continue;
			bool all = true;
			for (int b = 0; b < 3; ++b) {
				if (b == a) continue;
				const double low = (l[a] + j) * (1.0 / h[a]) * l[b] - nr[b] - m, high = (h[a] + j) * (1.0 / l[a]) * h[b] - nr[b] + m;
				// floor(low) <= u_b <= floor(high)
				if (!(low < u[b] + 1.0 && high >= u[b])) all = false;
			}
			if (all) return true;
		}
		return false;
	};
	int n = n0;
	for (int j = n0; j < bm::kViewCap; ++j) {
		int u[3];
		for (u[2] = 0; u[2] <= j; ++u[2])
			for (u[1] = 0; u[1] <= j; ++u[1])
				for (u[0] = 0; u[0] <= j; ++u[0]) {
					if (u[0] != j && u[1] != j && u[2] != j) continue;
					if (!touched(u, j)) continue;
					const int x[3] = {c[0] + s[0] * u[0], c[1] + s[1] * u[1], c[2] + s[2] * u[2]};
					if (x[0] < 0 || x[0] >= f.n[0] || x[1] < 0 || x[1] >= f.n[1] || x[2] < 0 || x[2] >= f.n[2]) return n;
					if (f.cube[oct][f.at(x[0], x[1], x[2])] == 0) return n;
				}
		n = j + 1;
	}
	return n;
}

// one ray from `origin` (cell units, inside the grid) along `dir`, set up as traverse.h ray_setup does and walked with the move of steps.h;
// count: a violation is a failure (false: only counted, the margin-0 record).  Returns the violations.
static long walk(const World& w, const float origin[3], const float dir[3], const char* what, bool count) {
	int c[3] = {static_cast<int>(origin[0]), static_cast<int>(origin[1]), static_cast<int>(origin[2])};
	if (!w.inside(c)) return 0;
	if (dir[0] == 0.f && dir[1] == 0.f && dir[2] == 0.f) return 0;
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
	static Visit path[512];
	size_t len = 0;
	while (w.inside(c)) {
		const size_t i = w.at(c[0], c[1], c[2]);
		const bm::StepAxis m = bm::step_choose(t[0], t[1], t[2]);
		const int axis = m.x ? 0 : (m.y ? 1 : 2);
		path[len++] = {w.occ[i], w.plane[i], static_cast<uint8_t>(axis)};
		c[axis] += sgn[axis];
		t[0] = bm::step_add(t[0], d[0], m.x); t[1] = bm::step_add(t[1], d[1], m.y); t[2] = bm::step_add(t[2], d[2], m.z);
		if (sgn[axis] == 0 || len >= 512) { FAIL("(%s) walk does not end", what); return 0; }
	}
	long bad = 0;
	bool stamped = false;
	for (size_t i = 0; i < len; ++i) {
		const Visit& v = path[i];
		if (count) { if (v.byte == 0) ++seen_0; else if (v.byte == 255) ++seen_255; else ++seen_n; }
		if ((v.byte == 0) != (v.occupied != 0)) { ++bad; if (count) FAIL("(%s) byte %d in a cell that is %s", what, v.byte, v.occupied ? "occupied" : "empty"); break; }
		if (stamped && v.occupied) { ++bad; if (count) FAIL("(%s) occupied cell %zu cells into the walk, behind a 255 cell (dir %g %g %g)", what, i, dir[0], dir[1], dir[2]); break; }
		if (v.byte == 255) stamped = true;
		if (v.byte == 0 || v.byte == 255) continue;
		int moved[3] = {0, 0, 0};
		for (size_t j = i;; ++j) { // cells entered before an axis has moved `byte` cells
			if (++moved[path[j].axis] >= v.byte) break;
			if (j + 1 == len) { ++bad; if (count) FAIL("(%s) byte %d, but the walk leaves the grid after moves (%d, %d, %d) (dir %g %g %g)", what, v.byte, moved[0], moved[1], moved[2], dir[0], dir[1], dir[2]); break; }
			if (path[j + 1].occupied) { ++bad; if (count) FAIL("(%s) byte %d, but an occupied cell after moves (%d, %d, %d) (dir %g %g %g)", what, v.byte, moved[0], moved[1], moved[2], dir[0], dir[1], dir[2]); break; }
		}
		if (bad) break;
	}
	if (count) { ++rays_walked; cells_walked += static_cast<long>(len); }
	return bad;
}

// ---- worlds.  kind 0: terrain; 1: a cross of ridges with one-cell notches; 2: terrain with overhangs and floating bricks; 3: a hollow
// mountain; 4: empty
static void fill(World& w, int kind) {
	std::fill(w.occ.begin(), w.occ.end(), 0);
	const int X = w.n[0], Z = w.n[2];
	auto terrain = [&](float base, float amp) {
		const float fx = 0.2f + 0.5f * rndf(), fy = 0.2f + 0.5f * rndf(), ph = 6.f * rndf();
		for (int y = 0; y < X; ++y)
			for (int x = 0; x < X; ++x) {
				const float h = (base + amp * std::sin(fx * x + ph) * std::cos(fy * y)) * Z + 1.5f * rndf();
				for (int z = 0; z < Z && z < static_cast<int>(h); ++z) w.set(x, y, z);
			}
	};
	if (kind == 0) terrain(0.3f, 0.2f);
	if (kind == 1) {
		for (int y = 0; y < X; ++y) for (int x = 0; x < X; ++x) w.set(x, y, 0);
		const int hgt = Z / 2;
		for (int i = 0; i < X; ++i) for (int z = 1; z <= hgt; ++z) { w.set(i, X / 2, z); w.set(X / 2, i, z); }
		for (int z = 1; z <= hgt; ++z) { w.set(X / 4, X / 2, z, 0); w.set(X / 2, X / 4 * 3, z, 0); } // the notches: one cell wide, down to the floor
	}
	if (kind == 2) {
		terrain(0.25f, 0.15f);
		for (int k = 0; k < 4; ++k) {
			const int x0 = static_cast<int>(rnd() % X), y0 = static_cast<int>(rnd() % X), z0 = Z / 2 + static_cast<int>(rnd() % (Z / 2));
			for (int y = y0; y < y0 + 4; ++y) for (int x = x0; x < x0 + 5; ++x) w.set(x, y, z0);
		}
		for (int k = 0; k < 6; ++k) w.set(static_cast<int>(rnd() % X), static_cast<int>(rnd() % X), Z / 3 + static_cast<int>(rnd() % (Z - Z / 3)));
	}
	if (kind == 3) {
		const int cx = X / 2, cy = X / 2, r = X / 2 - 2, hgt = Z - 3;
		for (int z = 0; z < hgt; ++z)
			for (int y = 0; y < X; ++y)
				for (int x = 0; x < X; ++x) {
					const int d = std::max(std::abs(x - cx), std::abs(y - cy)), rz = r - z * r / hgt;
					if (z == 0 || d == rz || (d < rz && z == hgt - 1)) w.set(x, y, z); // floor, shell
				}
		w.set(cx, cy - (r - 1 * r / hgt), 1, 0); // a one-cell door
	}
}

struct Position { float p[3]; const char* what; };

static std::vector<Position> positions(const World& w, int kind) {
	const int X = w.n[0], Z = w.n[2];
	std::vector<Position> out;
	out.push_back({{X * 0.5f + 0.37f, X * 0.5f - 0.21f, Z * 0.5f + 0.13f}, "centre"});
	{ const int x = X / 3, y = X / 3 + 1; out.push_back({{x + 0.4f, y + 0.6f, static_cast<float>(std::min(Z - 1, w.top(x, y) + 1)) + 0.5f}, "one cell above the terrain"}); }
	if (kind == 1) out.push_back({{X / 4 + 0.5f, X / 2 + 0.3f, 1.5f}, "inside a notch"});
	if (kind == 3) out.push_back({{X / 2 + 0.3f, X / 2 - 0.6f, 2.4f}, "inside the hollow"});
	out.push_back({{X * 0.25f + 0.2f, X * 0.7f + 0.1f, Z - 0.3f}, "top layer"});
	out.push_back({{0.7f, X - 0.2f, Z - 0.6f}, "corner cell"});
	out.push_back({{static_cast<float>(X / 2 + 1), static_cast<float>(X / 3), static_cast<float>(Z - 2)}, "integer coordinates"});
	out.push_back({{X / 2 + 0.0001f, X / 4 + 0.9999f, Z * 0.75f + 0.5f}, "1e-4 cell from a face"});
	return out;
}

// directions: uniform over the sphere; aimed at corners and edges of cells; with a zero component
static void direction(const World& w, const float p[3], long k, float out[3]) {
	const int mode = static_cast<int>(k % 8);
	if (mode < 5) { // uniform
		const float z = 2.f * rndf() - 1.f, phi = 6.2831853f * rndf(), r = std::sqrt(1.f - z * z);
		out[0] = r * std::cos(phi); out[1] = r * std::sin(phi); out[2] = z;
	} else if (mode < 7) { // a corner of a cell (mode 5) or a point of an edge (mode 6), hit exactly or missed by a few ulps
		float q[3];
		for (int a = 0; a < 3; ++a) q[a] = static_cast<float>(rnd() % static_cast<uint32_t>(w.n[a] + 1));
		if (mode == 6) q[rnd() % 3] += rndf();
		for (int a = 0; a < 3; ++a) out[a] = q[a] - p[a];
		if (rnd() & 1) out[rnd() % 3] *= 1.f + (static_cast<int>(rnd() % 9) - 4) * 1.1920929e-7f;
	} else { // a zero component, or two
		const float z = 2.f * rndf() - 1.f, phi = 6.2831853f * rndf(), r = std::sqrt(1.f - z * z);
		out[0] = r * std::cos(phi); out[1] = r * std::sin(phi); out[2] = z;
		out[rnd() % 3] = 0.f;
		if (rnd() % 4 == 0) out[rnd() % 3] = 0.f;
	}
	const float len = std::sqrt(out[0] * out[0] + out[1] * out[1] + out[2] * out[2]);
	if (len > 0.f) for (int a = 0; a < 3; ++a) out[a] /= len;
}

static int plane_mode(const char* in, const char* out) {
	std::FILE* f = std::fopen(in, "rb");
	if (!f) return 2;
	int32_t n[3];
	float origin[3], lens;
	if (std::fread(n, 4, 3, f) != 3 || std::fread(origin, 4, 3, f) != 3 || std::fread(&lens, 4, 1, f) != 1) { std::fclose(f); return 2; }
	std::vector<uint8_t> occ(static_cast<size_t>(n[0]) * n[1] * n[2]), plane;
	const size_t got = std::fread(occ.data(), 1, occ.size(), f);
	std::fclose(f);
	if (got != occ.size()) return 2;
	const bm::ViewPlan v = bm::view_plan(origin, lens, 8.f * n[0], 8.f * n[2], n[0], n[2]);
	if (v.valid) { const int nn[3] = {n[0], n[1], n[2]}; bm::view_plane_host(v, bm::view_host_field(nn, occ), plane); }
	f = std::fopen(out, "wb");
	if (!f) return 2;
	const size_t put = std::fwrite(plane.data(), 1, plane.size(), f);
	std::fclose(f);
	return put == plane.size() ? 0 : 2;
}

int main(int argc, char** argv) {
	if (argc == 4 && std::strcmp(argv[1], "plane") == 0) return plane_mode(argv[2], argv[3]);
	const long per_position = argc > 1 ? std::atol(argv[1]) : 100000;
	long margin0 = 0, margin0_rays = 0;
	const int dims[3][2] = {{16, 16}, {32, 16}, {16, 32}};
	for (int kind = 0; kind < 5; ++kind)
		for (const auto& dm : dims) {
			World w(dm[0], dm[1]);
			fill(w, kind);
			const bm::ViewHostField field = bm::view_host_field(w.n, w.occ);
			seen_n = seen_255 = seen_0 = 0;
			for (const Position& pos : positions(w, kind)) {
				float origin[3] = {pos.p[0] * 8.f, pos.p[1] * 8.f, pos.p[2] * 8.f};
				bm::ViewPlan v = bm::view_plan(origin, 0.f, 8.f * w.n[0], 8.f * w.n[2], w.n[0], w.n[2]);
				if (!v.valid) { FAIL("(%s) no plan for a position inside the world", pos.what); continue; }
				const float p[3] = {origin[0] / 8.f, origin[1] / 8.f, origin[2] / 8.f};
				bm::view_plane_host(v, field, w.plane);
				++planes;
				for (int z = 0; z < w.n[2]; ++z)
					for (int y = 0; y < w.n[1]; ++y)
						for (int x = 0; x < w.n[0]; ++x) {
							const int c[3] = {x, y, z};
							const int want = second_byte(v, field, c), got = w.plane[w.at(x, y, z)];
							if (got != want) FAIL("(%s) cell %d %d %d: byte %d, the rule written out again gives %d", pos.what, x, y, z, got, want);
							int oct = 0;
							for (int k = 0; k < 3; ++k) if (c[k] < v.cell[k]) oct |= 1 << k;
							if (got != 0 && got != 255 && got > field.cube[oct][w.at(x, y, z)]) ++longer;
						}
				for (long k = 0; k < per_position; ++k) {
					float dir[3];
					direction(w, p, k, dir);
					walk(w, p, dir, pos.what, true);
				}
				// the record: the same plane with no margin at all, rays aimed at corners and edges
				v.margin = 0.0;
				bm::view_plane_host(v, field, w.plane);
				for (long k = 0; k < per_position / 4; ++k) {
					float dir[3];
					direction(w, p, 5 + (k & 1), dir);
					margin0 += walk(w, p, dir, pos.what, false);
					++margin0_rays;
				}
			}
			// (the empty world is built to have byte 255 alone: every cell has escaped)
			if (seen_255 == 0 || (kind != 4 && (seen_n == 0 || seen_0 == 0))) FAIL("world kind %d (%d x %d): visited byte-n %ld, byte-255 %ld, byte-0 %ld cells: a class was not exercised", kind, dm[0], dm[1], seen_n, seen_255, seen_0);
			std::printf("world_%d_%dx%d_n %ld world_%d_%dx%d_255 %ld world_%d_%dx%d_0 %ld\n", kind, dm[0], dm[1], seen_n, kind, dm[0], dm[1], seen_255, kind, dm[0], dm[1], seen_0);
		}
	// plans that must be refused: outside the box, on its boundary, NaN, a lens
	{
		const float nan = std::nanf("");
		const float bad[5][3] = {{-1.f, 5.f, 5.f}, {5.f, 128.f, 5.f}, {5.f, 5.f, 0.f}, {nan, 5.f, 5.f}, {5.f, 5.f, 300.f}};
		for (const auto& o : bad) if (!bm::view_plan(o, 0.f, 128.f, 128.f, 16, 16).valid) ++refused;
		const float ok[3] = {5.f, 5.f, 5.f};
		if (!bm::view_plan(ok, 0.5f, 128.f, 128.f, 16, 16).valid) ++refused;
		if (!bm::view_plan(ok, nan, 128.f, 128.f, 16, 16).valid) ++refused;
		if (!bm::view_plan(ok, 0.f, 128.f, 128.f, 16, 16).valid) FAIL("a plain inside position was refused");
	}
	std::printf("planes %ld refused %ld rays %ld cells %ld longer_bytes %ld margin0_rays %ld margin0_violations %ld failures %ld\n", planes, refused, rays_walked, cells_walked, longer,
				margin0_rays, margin0, failures);
	return failures > 100 ? 100 : static_cast<int>(failures);
}
