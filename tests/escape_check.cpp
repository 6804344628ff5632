// escape_check.cpp -- CPU replay test of brickmap_amd/csrc/escape.h (compiled and run by tests/test_escape_rule.py).
// The escape predicate and the table's definition are the very functions the kernels inline (escape.hip builds the table with them,
// traverse.h tests rays against it).  Here small random worlds get their table from those functions -- checked against the definition
// written out as loops -- and random rays are walked cell by cell the way the reference walks them (src/voxel.cuh:249-258: the move of
// steps.h, which tests/step_check.cpp ties to the reference), from their start cell until they leave the grid.  From the first cell in
// which the predicate holds, the walk must never meet an occupied cell: ending the ray there as a miss changes nothing.
// The families of main(): every octant, zero direction components, starts on cell faces, empty and full worlds, a single brick in the far
// corner cell of the quadrant (the quadrant is inclusive), a ceiling above the start cell.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../brickmap_amd/csrc/escape.h"
#include "../brickmap_amd/csrc/steps.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return static_cast<uint32_t>(rng_state >> 32);
}
static float rndf() { return (rnd() >> 8) * (1.0f / 16777216.0f); }

static long failures = 0, rays_walked = 0, cells_walked = 0, rays_escaped = 0, rays_escaped_at_start = 0, tables_checked = 0;
#define FAIL(...) do { if (failures++ < 10) { std::fprintf(stderr, "MISMATCH " __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

// a small world with the cube field's layout constants (scene.cpp cube_field_layout) and its escape table
struct World {
	int X, Z, shift;          // cells along x and y, cells along z, log2 of the row pitch
	uint32_t pxy, plane;
	std::vector<uint8_t> occ; // [z][y][x]
	std::vector<uint32_t> table;
	World(int cells, int height) : X(cells), Z(height), shift(2) {
		while ((1 << shift) < X + 2) ++shift;
		pxy = static_cast<uint32_t>(X + 2) << shift;
		plane = pxy * static_cast<uint32_t>(Z + 2);
		occ.assign(static_cast<size_t>(X) * X * Z, 0);
	}
	uint8_t& at(int x, int y, int z) { return occ[(static_cast<size_t>(z) * X + y) * X + x]; }
	bool inside(int x, int y, int z) const { return x >= 0 && x < X && y >= 0 && y < X && z >= 0 && z < Z; }
	uint32_t cell_offset(int oct, int x, int y, int z) const {
		return static_cast<uint32_t>(oct) * plane + static_cast<uint32_t>(z + 1) * pxy + (static_cast<uint32_t>(y + 1) << shift) + static_cast<uint32_t>(x + 1);
	}
	// the table, pass by pass as escape.hip builds it
	void build_table() {
		std::vector<int> top(static_cast<size_t>(X) * X), bottom(top.size());
		for (int y = 0; y < X; ++y)
			for (int x = 0; x < X; ++x) {
				int t = bm::escape_none(0, Z), b = bm::escape_none(4, Z);
				for (int z = 0; z < Z; ++z) bm::escape_column_fold(t, b, z, at(x, y, z) != 0);
				top[static_cast<size_t>(y) * X + x] = t; bottom[static_cast<size_t>(y) * X + x] = b;
			}
		table.assign(bm::escape_entries(pxy), 0xDEADBEEFu);
		for (int o = 0; o < 8; ++o) {
			for (int x = 0; x < X; ++x) {
				int acc = bm::escape_none(o, Z);
				const int step = (o & 2) ? 1 : -1;
				for (int k = 0, y = (o & 2) ? 0 : X - 1; k < X; ++k, y += step) {
					acc = bm::escape_fold(o, acc, top[static_cast<size_t>(y) * X + x], bottom[static_cast<size_t>(y) * X + x]);
					table[bm::escape_index(o, shift, pxy, x, y)] = static_cast<uint32_t>(acc);
				}
			}
			for (int y = 0; y < X; ++y) {
				int acc = bm::escape_none(o, Z);
				const int step = (o & 1) ? 1 : -1;
				for (int k = 0, x = (o & 1) ? 0 : X - 1; k < X; ++k, x += step) {
					const uint32_t i = bm::escape_index(o, shift, pxy, x, y);
					const int v = static_cast<int>(table[i]);
					acc = bm::escape_fold(o, acc, v, v);
					table[i] = bm::escape_entry(o, acc, pxy, plane);
				}
			}
		}
	}
	// the definition, written out: highest (lowest) occupied z over the columns of the octant's quadrant that starts at (x, y)
	int threshold(int o, int x, int y) {
		int e = (o & 4) ? Z : -1;
		for (int yy = 0; yy < X; ++yy)
			for (int xx = 0; xx < X; ++xx) {
				if ((o & 1) ? xx > x : xx < x) continue;
				if ((o & 2) ? yy > y : yy < y) continue;
				for (int z = 0; z < Z; ++z)
					if (at(xx, yy, z)) { if (o & 4) { if (z < e) e = z; } else if (z > e) e = z; }
			}
		return e;
	}
	void check_table() {
		++tables_checked;
		for (int o = 0; o < 8; ++o)
			for (int y = 0; y < X; ++y)
				for (int x = 0; x < X; ++x) {
					const int want = threshold(o, x, y), got = bm::escape_height_of(o, table[bm::escape_index(o, shift, pxy, x, y)], pxy, plane);
					if (want != got) FAIL("(table) octant %d column (%d, %d): threshold %d, definition %d", o, x, y, got, want);
				}
	}
};

// One ray from `origin` (cell units, inside the grid) along `dir`, set up as traverse.h ray_setup does and walked with the move of steps.h.
// Returns whether it escaped; *at_start: in its very first cell.
static bool walk(World& w, const float origin[3], const float dir[3], const char* family, bool* at_start) {
	int c[3] = {static_cast<int>(origin[0]), static_cast<int>(origin[1]), static_cast<int>(origin[2])};
	if (!w.inside(c[0], c[1], c[2])) return false;
	const int oct = (dir[0] < 0.f ? 1 : 0) | (dir[1] < 0.f ? 2 : 0) | (dir[2] < 0.f ? 4 : 0);
	int sgn[3];
	float t[3], d[3];
	for (int k = 0; k < 3; ++k) {
		sgn[k] = (0.f < dir[k]) - (dir[k] < 0.f);
		const float cb = dir[k] > 0.f ? static_cast<float>(c[k] + 1) : static_cast<float>(c[k]);
		const float r = dir[k] == 0.0f ? 0.0f : 1.f / dir[k];
		t[k] = dir[k] != 0.f ? (cb - origin[k]) * r : 1000000.f;
		d[k] = static_cast<float>(sgn[k]) * r;
	}
	const int step_z = sgn[2] * static_cast<int>(w.pxy);
	const uint32_t esc = w.table[bm::escape_index(oct, w.shift, w.pxy, c[0], c[1])];
	++rays_walked;
	bool escaped = false;
	*at_start = false;
	for (int n = 0; w.inside(c[0], c[1], c[2]); ++n) {
		++cells_walked;
		if (n > 3 * (w.X + w.Z)) { FAIL("(%s) walk does not end", family); break; }
		const bool now = bm::escape_reached(w.cell_offset(oct, c[0], c[1], c[2]), esc, step_z);
		if (now && !escaped) { escaped = true; *at_start = n == 0; }
		if (escaped && !now) FAIL("(%s) octant %d: escaped, then not escaped in cell (%d, %d, %d)", family, oct, c[0], c[1], c[2]);
		if (escaped && w.at(c[0], c[1], c[2]))
			FAIL("(%s) octant %d: occupied cell (%d, %d, %d) after the escape point (dir %g %g %g)", family, oct, c[0], c[1], c[2], dir[0], dir[1], dir[2]);
		const bm::StepAxis m = bm::step_choose(t[0], t[1], t[2]);
		const int axis = m.x ? 0 : (m.y ? 1 : 2);
		c[axis] += sgn[axis];
		t[0] = bm::step_add(t[0], d[0], m.x); t[1] = bm::step_add(t[1], d[1], m.y); t[2] = bm::step_add(t[2], d[2], m.z);
		if (sgn[axis] == 0) { FAIL("(%s) move along an axis with a zero direction component", family); break; }
	}
	if (escaped) { ++rays_escaped; if (*at_start) ++rays_escaped_at_start; }
	return escaped;
}

// a direction of octant `oct`; bits of `zero` name components that are exactly 0 (a zero component counts as positive: only asked for
// where the octant's bit is clear); never all three
static void direction(int oct, int zero, float dir[3]) {
	for (int k = 0; k < 3; ++k) {
		const float m = 0.02f + rndf();
		dir[k] = (zero >> k & 1) ? 0.f : ((oct >> k & 1) ? -m : m);
	}
	if (dir[0] == 0.f && dir[1] == 0.f && dir[2] == 0.f) dir[rnd() % 3] = 1.f;
}

// `n` rays per octant through `w` (whose table is built and checked here): random starts, starts on cell faces, zero components
static void rays(World& w, const char* family, int n, long* escaped = nullptr, long* at_start = nullptr) {
	w.build_table();
	w.check_table();
	const int lim[3] = {w.X, w.X, w.Z};
	for (int oct = 0; oct < 8; ++oct)
		for (int i = 0; i < n; ++i) {
			float o[3], dir[3];
			const int zero = (i % 4 == 1) ? static_cast<int>(rnd() % 8) & ~oct : 0;
			direction(oct, zero, dir);
			for (int k = 0; k < 3; ++k) {
				o[k] = rndf() * static_cast<float>(lim[k]);
				if (i % 4 >= 2 && (rnd() & 1)) o[k] = static_cast<float>(rnd() % static_cast<uint32_t>(lim[k])); // on a cell face
				if (!(o[k] < static_cast<float>(lim[k]))) o[k] = static_cast<float>(lim[k]) - 0.5f;
			}
			bool first = false;
			const bool e = walk(w, o, dir, family, &first);
			if (escaped && e) ++*escaped;
			if (at_start && e && first) ++*at_start;
		}
}

int main(int argc, char** argv) {
	const int worlds = argc > 1 ? std::atoi(argv[1]) : 200;
	// ---- random worlds: a few bricks to half full; cubes, flat and tall grids
	for (int i = 0; i < worlds; ++i) {
		World w(2 + static_cast<int>(rnd() % 7), 1 + static_cast<int>(rnd() % 8));
		const uint32_t density = 1u + rnd() % 128u; // of 256
		for (auto& v : w.occ) v = (rnd() & 255u) < density && (rnd() & 3u) == 0u;
		rays(w, "random", 40);
	}
	// ---- terrain-like worlds: columns filled from the ground up to a random height (what the table is for)
	for (int i = 0; i < worlds; ++i) {
		World w(3 + static_cast<int>(rnd() % 6), 3 + static_cast<int>(rnd() % 6));
		for (int y = 0; y < w.X; ++y)
			for (int x = 0; x < w.X; ++x) { const int h = static_cast<int>(rnd() % static_cast<uint32_t>(w.Z)); for (int z = 0; z < h; ++z) w.at(x, y, z) = 1; }
		rays(w, "terrain", 40);
	}
	// ---- an empty world: every ray has escaped in its first cell; a full one: none ever does
	{
		World w(5, 4);
		long escaped = 0, first = 0;
		const long before = rays_walked;
		rays(w, "empty", 100, &escaped, &first);
		if (escaped != rays_walked - before || first != escaped) FAIL("(empty) %ld of %ld rays escaped, %ld of them at the start", escaped, rays_walked - before, first);
		World f(5, 4);
		for (auto& v : f.occ) v = 1;
		escaped = 0;
		rays(f, "full", 100, &escaped);
		if (escaped != 0) FAIL("(full) %ld rays escaped", escaped);
	}
	// ---- a single brick in the far corner cell of the octant's quadrant (and of its z range): the quadrant includes it.  Rays are aimed at
	// the brick's cell from everywhere, so some of them do arrive; a ray of the octant never escapes before it has passed the brick's slice
	for (int oct = 0; oct < 8; ++oct) {
		World w(6, 5);
		const int bx = (oct & 1) ? 0 : w.X - 1, by = (oct & 2) ? 0 : w.X - 1, bz = (oct & 4) ? 0 : w.Z - 1;
		w.at(bx, by, bz) = 1;
		w.build_table();
		w.check_table();
		long hits = 0;
		for (int i = 0; i < 2000; ++i) {
			float o[3] = {rndf() * w.X, rndf() * w.X, rndf() * w.Z}, dir[3];
			if (i & 1) { o[0] = static_cast<float>(static_cast<int>(o[0])); o[2] = static_cast<float>(static_cast<int>(o[2])); }
			const float target[3] = {bx + rndf(), by + rndf(), bz + rndf()};
			for (int k = 0; k < 3; ++k) dir[k] = target[k] - o[k];
			if (dir[0] == 0.f && dir[1] == 0.f && dir[2] == 0.f) continue;
			bool first = false;
			const int c[3] = {static_cast<int>(o[0]), static_cast<int>(o[1]), static_cast<int>(o[2])};
			const bool e = walk(w, o, dir, "far corner", &first);
			const int ray_oct = (dir[0] < 0.f ? 1 : 0) | (dir[1] < 0.f ? 2 : 0) | (dir[2] < 0.f ? 4 : 0);
			if (ray_oct == oct && !(c[0] == bx && c[1] == by && c[2] == bz)) { ++hits; if (e && first) FAIL("(far corner) octant %d: a ray towards the brick escaped in its first cell", oct); }
		}
		if (hits < 100) FAIL("(far corner) octant %d: only %ld rays of the octant", oct, hits);
		// the same world from the brick's own column: the own column counts
		float o[3] = {bx + 0.5f, by + 0.5f, (oct & 4) ? w.Z - 0.5f : 0.5f}, dir[3] = {0.f, 0.f, (oct & 4) ? -1.f : 1.f};
		bool first = false;
		if (walk(w, o, dir, "own column", &first) && first) FAIL("(own column) octant %d: escaped under / over the brick of its own column", oct);
	}
	// ---- a ceiling above (a floor below) the start cell: rays towards it must not escape before it
	for (int pass = 0; pass < 2; ++pass) {
		World w(6, 6);
		const int slab = pass ? 1 : 4;
		for (int y = 0; y < w.X; ++y) for (int x = 0; x < w.X; ++x) w.at(x, y, slab) = 1;
		w.at(2, 3, pass ? 4 : 1) = 1; // and something on the near side of the start cells
		w.build_table();
		w.check_table();
		for (int oct = 0; oct < 8; ++oct)
			for (int i = 0; i < 500; ++i) {
				float o[3] = {rndf() * w.X, rndf() * w.X, pass ? 2.f + 2.f * rndf() : 2.f * rndf() + 1.f}, dir[3];
				direction(oct, (i % 3 == 0) ? static_cast<int>(rnd() % 4) & ~oct : 0, dir);
				bool first = false;
				const bool e = walk(w, o, dir, "ceiling", &first);
				const bool towards = pass ? dir[2] < 0.f : dir[2] > 0.f;
				if (towards && e && first) FAIL("(ceiling) octant %d: a ray towards the slab escaped in its first cell", oct);
			}
	}
	std::printf("rays %ld cells %ld escaped %ld at_start %ld tables %ld failures %ld\n", rays_walked, cells_walked, rays_escaped, rays_escaped_at_start, tables_checked, failures);
	return failures ? 1 : 0;
}
