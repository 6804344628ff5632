// jump_room_sim.cpp -- CPU replay behind the rule "is a jump worth it here" (csrc/steps.h jump_worth; profiles/r17_jump_room.txt section 1).
// Analysis tool, not product, not a test.
// Rays: every ray of the oracle's per-pixel render of bench config 2 (1024^3 world, its camera) at 160 x 90, 1 spp, 4 segments
// (orc_set_ray_probe), split by kind: primary / bounce / shadow.  Every ray is walked with the product's own arithmetic -- the octant
// cube field of world.cpp, dda_jump of jump.h, single moves -- for as many cells as the reference visits (orc_intersect_voxel's index loads).
// The view plane, the sun plane, the escape rule and the shadow heights are NOT modelled: primary rays walk their octant plane here, so
// their cubes near the camera are smaller than the kernel's, and shadow rays walk further than the kernel lets them.
//   part 1 (the parent's rule): jumps by the binade exponent of their smallest tmax -- how many, the cells they advance, what ended them;
//   part 2 (per candidate rule): stops per ray, a lane on its own: single moves, jumps, candidates, and the lane-level cost
//           jumps x 162 + single moves x 25 (weighted VALU of A.jump / A.single, tools/isa_passes.py);
//   part 3 (per candidate rule): a wave-level model -- 64 consecutive rays of one kind start together and are run to the end under the
//           kernel's pass choice (candidate quorum 1/2, jump pass when nJ * 4 >= nO, up to 6 jump passes per round while a quarter
//           keeps walking, else 4 single-move passes; a not-worth lane rides in a jump pass with its own cube): J / S / B passes and
//           lanes per pass, cost J x 162 + S x 25.  tools/sim/sched_sim.cpp models the whole scheduler with refills and
//           the machine but takes no rule; this is the part of it the rule changes, for waves that start in step (a refill of primary rays).
// Rules: (a) a floor E on the exponent of the smallest tmax, E = -10 (the parent: jump_possible alone), 0 ... 4;
//        (b) room left in the binade >= K x the smallest tdelta, K = 2, 4, 8.
// build: g++ -O2 -std=c++17 -ffp-contract=off -Ibrickmap_amd/csrc tools/sim/jump_room_sim.cpp brickmap_amd/csrc/world.cpp -Loracle -l:liboracle.so -Wl,-rpath,$PWD/oracle -lpthread -o scratch/jump_room_sim
// run:   scratch/jump_room_sim [width height]
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jump.h"
#include "world.h"

extern "C" {
void* orc_world_create(int, int);
void orc_world_generate(void*, int);
void orc_world_reset_device(void*, int);
void orc_camera_direction(double, double, float*);
typedef void (*orc_ray_probe_t)(unsigned, int, int, const float*, const float*);
void orc_set_ray_probe(orc_ray_probe_t);
struct OrcCamera { float position[3], direction[3], up[3], focal, lens; };
struct OrcFrame { int width, height, spp, sample_base, max_bounces; unsigned base_frame; int primary_only, band_rows, shard_rank, shard_count; float sun_x, sun_y; };
double orc_render(void*, const OrcCamera*, const OrcFrame*, float*, uint32_t*, void*, int);
int orc_intersect_voxel(void* w, const float* origin, const float* direction, float* normal_io, float* distance_io, const int* campos, int* out4, uint64_t* index_loads);
}

struct RayRec { float o[3], d[3]; int kind; uint64_t loads; };
static std::vector<RayRec> g_rays;
static float g_cam[3];
static void ray_probe(unsigned, int, int kind, const float* o, const float* d) {
	RayRec r;
	memcpy(r.o, o, 12); memcpy(r.d, d, 12);
	r.kind = kind == 1 ? 2 : (memcmp(o, g_cam, 12) == 0 ? 0 : 1); // 0 primary, 1 bounce, 2 shadow
	r.loads = 0;
	g_rays.push_back(r);
}

static inline float gmin(float a, float b) { return (b < a) ? b : a; }
static inline float gmax(float a, float b) { return (a < b) ? b : a; }
static inline int isign(float x) { return (0.f < x) - (x < 0.f); }

struct Rule { int E, K; const char* name; };
static const Rule kRules[] = {{-10, 0, "parent (E=-10)"}, {0, 0, "a: E=0"}, {1, 0, "a: E=1"}, {2, 0, "a: E=2"}, {3, 0, "a: E=3"}, {4, 0, "a: E=4"},
							  {-10, 2, "b: K=2"}, {-10, 4, "b: K=4"}, {-10, 8, "b: K=8"}};
constexpr int kNRules = sizeof(kRules) / sizeof(kRules[0]);
constexpr int JUMP_MIN = 4, JUMP_RATIO = 4, JUMP_PASSES = 6, KEEP_DIV = 4, STEPS = 4;
constexpr double COST_J = 162, COST_S = 25;

static bool worth(const Rule& R, float tx, float ty, float tz, float dx, float dy, float dz) {
	const float m = gmin(gmin(tx, ty), tz);
	const uint32_t lo = uint32_t(127 + R.E) << 23;
	bool w = bm::jump_bits(m) - lo < bm::kJumpMaxBits - lo;
	if (R.K) {
		const float d = gmin(gmin(dx, dy), dz);
		const float end = bm::jump_float((bm::jump_bits(m) & 0x7F800000u) + (1u << 23));
		w = w && (end - m) >= float(R.K) * d;
	}
	return w;
}

enum { S_DONE = 0, S_OUTER = 1, S_CAND = 2, S_JUMP = 3 };
struct World {
	std::vector<uint8_t> field;
	int cells, cells_h, cfx; size_t plane; float gs, gh;
	int F(int oct, int x, int y, int z) const {
		if (x < -1 || y < -1 || z < -1 || x > cells || y > cells || z > cells_h) return 255;
		return field[oct * plane + (size_t(z + 1) * cfx + (y + 1)) * cfx + (x + 1)];
	}
};
static World g_w;

struct JumpHist { uint64_t n[40] = {}, cells[40] = {}, binade[40] = {}; }; // by exponent + 12 (2^-12 ... 2^27)
struct Lane {
	float tx, ty, tz, dx, dy, dz, ix, iy, iz;
	int px, py, pz, sx, sy, sz, oct, st = S_DONE;
	uint32_t cube = 0; bool nojump = false;
	uint64_t visited = 0, loads = 0;
	uint64_t n_single = 0, n_jump = 0, n_cand = 0;
};
static int lookup(Lane& s, const Rule& R) {
	const int v = g_w.F(s.oct, s.px, s.py, s.pz);
	const bool possible = bm::jump_possible(s.tx, s.ty, s.tz);
	s.cube = uint32_t(v); s.nojump = !possible;
	int st = (v >= JUMP_MIN && possible && worth(R, s.tx, s.ty, s.tz, s.dx, s.dy, s.dz)) ? S_JUMP : S_OUTER;
	if (v == 0) st = S_CAND;
	if (v == 255) st = S_DONE;
	return st;
}
static int setup(Lane& s, const RayRec& r, const Rule& R) { // traverse.h ray_setup
	float ox = r.o[0], oy = r.o[1], oz = r.o[2];
	const float dx = r.d[0], dy = r.d[1], dz = r.d[2];
	const float gs = g_w.gs, gh = g_w.gh;
	const float t1x = (0.f - ox) / dx, t1y = (0.f - oy) / dy, t1z = (0.f - oz) / dz, t2x = (gs - ox) / dx, t2y = (gs - oy) / dy, t2z = (gh - oz) / dz;
	const float tminn = gmax(gmax(gmin(t1x, t2x), 0.f), gmax(gmin(t1y, t2y), gmin(t1z, t2z)));
	if (!(gmin(gmax(t1x, t2x), gmin(gmax(t1y, t2y), gmax(t1z, t2z))) > tminn)) return S_DONE;
	if (tminn > 0) {
		ox += dx * tminn; oy += dy * tminn; oz += dz * tminn;
		const float cx = gs / 2.f - ox, cy = gs / 2.f - oy, cz = gh / 2.f - oz;
		const float ax = fabsf(cx) * (1.f / (gs / gh)), ay = fabsf(cy) * (1.f / (gs / gh)), az = fabsf(cz) * 1.f;
		const float m = gmax(ax, gmax(ay, az));
		const float nx = float(isign(-cx)) * truncf(ax / m + 0.000001f), ny = float(isign(-cy)) * truncf(ay / m + 0.000001f), nz = float(isign(-cz)) * truncf(az / m + 0.000001f);
		ox -= nx * 0.001f; oy -= ny * 0.001f; oz -= nz * 0.001f;
	}
	ox /= 8.f; oy /= 8.f; oz /= 8.f;
	s.px = int(ox); s.py = int(oy); s.pz = int(oz);
	if (s.px < 0 || s.px >= g_w.cells || s.py < 0 || s.py >= g_w.cells || s.pz < 0 || s.pz >= g_w.cells_h) return S_DONE;
	s.sx = isign(dx); s.sy = isign(dy); s.sz = isign(dz);
	const float rx = dx == 0.f ? 0.f : 1.f / dx, ry = dy == 0.f ? 0.f : 1.f / dy, rz = dz == 0.f ? 0.f : 1.f / dz;
	s.tx = dx != 0.f ? ((dx > 0 ? float(s.px + 1) : float(s.px)) - ox) * rx : 1000000.f;
	s.ty = dy != 0.f ? ((dy > 0 ? float(s.py + 1) : float(s.py)) - oy) * ry : 1000000.f;
	s.tz = dz != 0.f ? ((dz > 0 ? float(s.pz + 1) : float(s.pz)) - oz) * rz : 1000000.f;
	s.dx = float(s.sx) * rx; s.dy = float(s.sy) * ry; s.dz = float(s.sz) * rz;
	s.ix = fabsf(dx); s.iy = fabsf(dy); s.iz = fabsf(dz);
	s.oct = (dx < 0 ? 1 : 0) | (dy < 0 ? 2 : 0) | (dz < 0 ? 4 : 0);
	s.visited = 1; s.loads = r.loads;
	s.n_single = s.n_jump = s.n_cand = 0;
	return lookup(s, R);
}
static int single_step(Lane& s, const Rule& R) {
	const bool mx = s.tx < s.ty && s.tx < s.tz, my = s.ty <= s.tx && s.ty < s.tz;
	if (mx) { s.px += s.sx; s.tx += s.dx; }
	else if (my) { s.py += s.sy; s.ty += s.dy; }
	else { s.pz += s.sz; s.tz += s.dz; }
	s.visited++; s.n_single++;
	return lookup(s, R);
}
static int jump(Lane& s, const Rule& R, JumpHist* h) {
	if (s.nojump) return single_step(s, R);
	uint32_t cx, cy, cz; int axis;
	const float m = gmin(gmin(s.tx, s.ty), s.tz);
	const bool cube_end = bm::dda_jump(s.tx, s.ty, s.tz, s.dx, s.dy, s.dz, s.ix, s.iy, s.iz, s.cube & 0xFFu, cx, cy, cz, axis);
	s.px += int(cx) * s.sx; s.py += int(cy) * s.sy; s.pz += int(cz) * s.sz;
	s.visited += cx + cy + cz; s.n_jump++;
	if (h) {
		const int e = std::min(39, std::max(0, int(bm::jump_bits(m) >> 23) - 127 + 12));
		h->n[e]++; h->cells[e] += cx + cy + cz; h->binade[e] += !cube_end;
	}
	return lookup(s, R);
}
static int candidate(Lane& s) { // the brick is tested: the ray ends here (its last cell) or passes through: cube 0, a plain move next
	s.n_cand++;
	if (s.visited >= s.loads) return S_DONE;
	s.cube = 0;
	return S_OUTER;
}

int main(int argc, char** argv) {
	const int G = 1024, W = argc > 2 ? atoi(argv[1]) : 160, H = argc > 2 ? atoi(argv[2]) : 90;
	void* ow = orc_world_create(G, G);
	orc_world_generate(ow, 8);
	orc_world_reset_device(ow, 1);
	OrcCamera cam{};
	cam.position[0] = G / 2.f; cam.position[1] = G / 8.f; cam.position[2] = 0.8f * G;
	orc_camera_direction(0.8, -0.5, cam.direction);
	cam.up[2] = 1.f; cam.focal = 1.f;
	memcpy(g_cam, cam.position, 12);
	OrcFrame fr{};
	fr.width = W; fr.height = H; fr.spp = 1; fr.max_bounces = 3; fr.base_frame = 1; fr.band_rows = H; fr.shard_count = 1; fr.sun_x = 0.05f; fr.sun_y = 0.1f;
	std::vector<float> accum(size_t(W) * H * 4);
	orc_set_ray_probe(ray_probe);
	orc_render(ow, &cam, &fr, accum.data(), nullptr, nullptr, 1);
	orc_set_ray_probe(nullptr);
	const int campos[3] = {int(cam.position[0] / 8.f), int(cam.position[1] / 8.f), int(cam.position[2] / 8.f)};
	for (RayRec& r : g_rays) {
		float nrm[3] = {0, 0, 0}, dist = r.kind == 2 ? 0.f : 1e20f;
		int out4[4];
		orc_intersect_voxel(ow, r.o, r.d, nrm, &dist, campos, out4, &r.loads);
	}
	bm::World world;
	world.dims.set(G, G);
	world.generate(8);
	world.build_cube_field(g_w.field, 8);
	g_w.cells = world.dims.cells; g_w.cells_h = world.dims.cells_height; g_w.cfx = g_w.cells + 2; g_w.plane = g_w.field.size() / 8;
	g_w.gs = float(G); g_w.gh = float(G);

	const char* names[3] = {"primary", "bounce", "shadow"};
	std::vector<const RayRec*> by_kind[3];
	for (const RayRec& r : g_rays) if (r.loads) by_kind[r.kind].push_back(&r);
	printf("config 2 at %d x %d, 1 spp, 4 segments: %zu rays that enter the grid: %zu primary, %zu bounce, %zu shadow (octant planes; no view / sun plane, no escape rule)\n", W, H,
		   by_kind[0].size() + by_kind[1].size() + by_kind[2].size(), by_kind[0].size(), by_kind[1].size(), by_kind[2].size());

	// ---- part 1: the parent's jumps by binade
	printf("\n== 1. jumps of the parent's rule by the binade [2^e, 2^(e+1)) of their smallest tmax: per ray; cells per jump; share ended by the binade end\n");
	for (int k = 0; k < 3; ++k) {
		JumpHist h;
		for (const RayRec* r : by_kind[k]) {
			Lane s;
			int st = setup(s, *r, kRules[0]);
			while (st != S_DONE) st = st == S_CAND ? candidate(s) : (st == S_JUMP ? jump(s, kRules[0], &h) : single_step(s, kRules[0]));
		}
		const double n = double(std::max<size_t>(by_kind[k].size(), 1));
		printf("%-8s", names[k]);
		for (int e = 0; e < 40; ++e) if (h.n[e]) printf("  e=%d: %.2f/ray %.1f cells %.0f%%", e - 12, h.n[e] / n, double(h.cells[e]) / h.n[e], 100.0 * h.binade[e] / h.n[e]);
		printf("\n");
	}

	// ---- part 2: stops per ray, a lane on its own
	printf("\n== 2. stops per ray by rule, a lane on its own (ST_JUMP jumps, ST_OUTER takes a single move): single moves + jumps + candidates; cost = jumps x %.0f + single moves x %.0f\n", COST_J, COST_S);
	for (int k = 0; k < 3; ++k)
		for (int ri = 0; ri < kNRules; ++ri) {
			uint64_t ns = 0, nj = 0, nc = 0;
			for (const RayRec* r : by_kind[k]) {
				Lane s;
				int st = setup(s, *r, kRules[ri]);
				while (st != S_DONE) st = st == S_CAND ? candidate(s) : (st == S_JUMP ? jump(s, kRules[ri], nullptr) : single_step(s, kRules[ri]));
				ns += s.n_single; nj += s.n_jump; nc += s.n_cand;
			}
			const double n = double(std::max<size_t>(by_kind[k].size(), 1));
			printf("%-8s %-15s %6.2f single + %5.2f jumps + %4.2f candidates = %6.2f stops, cost %7.1f\n", names[k], kRules[ri].name, ns / n, nj / n, nc / n, (ns + nj + nc) / n,
				   (nj * COST_J + ns * COST_S) / n);
		}

	// ---- part 3: waves of 64 rays that start in step
	printf("\n== 3. waves of 64 consecutive rays of one kind, started together, under the kernel's pass choice: passes (lanes per pass), cost = J x %.0f + S x %.0f per wave\n", COST_J, COST_S);
	for (int k = 0; k < 3; ++k) {
		double base = 0;
		for (int ri = 0; ri < kNRules; ++ri) {
			const Rule& R = kRules[ri];
			uint64_t J = 0, lJ = 0, S = 0, lS = 0, B = 0, lB = 0, waves = 0;
			for (size_t first = 0; first + 64 <= by_kind[k].size(); first += 64, ++waves) {
				Lane L[64];
				for (int l = 0; l < 64; ++l) L[l].st = setup(L[l], *by_kind[k][first + l], R);
				for (int guard = 0; guard < 100000; ++guard) {
					int nJ = 0, nO = 0, nB = 0;
					for (int l = 0; l < 64; ++l) { nJ += L[l].st == S_JUMP; nO += L[l].st == S_OUTER; nB += L[l].st == S_CAND; }
					const int live = nJ + nO + nB;
					if (!live) break;
					if (nB >= (live + 1) / 2 || nJ + nO == 0) {
						B++; lB += nB;
						for (int l = 0; l < 64; ++l) if (L[l].st == S_CAND) L[l].st = candidate(L[l]);
					} else if (nJ * JUMP_RATIO >= nO) {
						int walkers = nJ + nO;
						for (int pass = 0; pass < JUMP_PASSES; ++pass) {
							J++; lJ += walkers;
							int still = 0;
							for (int l = 0; l < 64; ++l) {
								if (L[l].st == S_JUMP || L[l].st == S_OUTER) L[l].st = jump(L[l], R, nullptr);
								still += L[l].st == S_JUMP || L[l].st == S_OUTER;
							}
							if (still * KEEP_DIV < walkers || still == 0) break;
							walkers = still;
						}
					} else {
						for (int step = 0; step < STEPS; ++step) {
							int n = 0;
							for (int l = 0; l < 64; ++l) if (L[l].st == S_OUTER) { L[l].st = single_step(L[l], R); n++; }
							S++; lS += n;
						}
					}
				}
			}
			const double w = double(std::max<uint64_t>(waves, 1)), cost = (J * COST_J + S * COST_S) / w;
			if (ri == 0) base = cost;
			printf("%-8s %-15s J %6.2f (%4.1f lanes)  S %6.2f (%4.1f)  B %5.2f (%4.1f)  cost %7.0f  %+5.1f %%\n", names[k], R.name, J / w, J ? double(lJ) / J : 0.0, S / w, S ? double(lS) / S : 0.0,
				   B / w, B ? double(lB) / B : 0.0, cost, 100.0 * (cost / base - 1.0));
		}
	}
	return 0;
}
