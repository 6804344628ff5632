// mesh_check.cpp -- a program with its own main around csrc/mesh_host.cpp and csrc/mesh.h alone (no HIP, no scene), built plain and with
// -fsanitize=address,undefined by tests/test_mesh_host.py:
//   1. the greedy cover of mesh.h on all 2^16 two-row masks (at three heights) and on random 64-bit masks against a brute-force painter:
//      every rectangle starts at the lowest bit left, lies inside what is left, cannot grow along u and then along v, and together they
//      paint every bit of the mask once, in at most 64 rounds;
//   2. the walk of mesh.hip, lane by lane on the host -- a cell's 100 rows of ten bits in an array where the kernel has its LDS, the drop
//      of cells that can have no face, the 48 lanes' masks from the rows, their quads one lane after the other -- against the plain
//      loops of bm_host_mesh_quads, on random volumes with random origins, pitches and flags, with a capacity that cuts the list;
//   3. the triangles of every quad: on the quad's plane, normals along its direction, the two areas summing to w h;
//   4. the refusals of the host routine.
// usage: mesh_check [rounds]; prints "name count" pairs and "failures N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../brickmap_amd/csrc/mesh.h"
#include "../include/brickmap.h"

namespace {

long failures = 0;
#define CHECK(cond)                                                                  \
	do {                                                                             \
		if (!(cond)) {                                                               \
			if (++failures <= 10) std::printf("line %d: %s\n", __LINE__, #cond);     \
		}                                                                            \
	} while (0)

bool bit(uint64_t m, int u, int v) { return (m >> (8 * v + u)) & 1u; }

// 1.
void check_cover(uint64_t mask, bool unit) {
	uint64_t left = mask;
	int rounds = 0;
	uint32_t quads = 0, faces = 0;
	bm::mesh_cover(mask, unit, [&](int u0, int v0, int w, int h) {
		++rounds;
		CHECK(left != 0 && 8 * v0 + u0 == __builtin_ctzll(left));
		CHECK(w >= 1 && h >= 1 && u0 + w <= 8 && v0 + h <= 8);
		if (unit) CHECK(w == 1 && h == 1);
		for (int v = v0; v < v0 + h && v < 8; ++v)
			for (int u = u0; u < u0 + w && u < 8; ++u) {
				CHECK(bit(left, u, v));
				left &= ~(uint64_t{1} << (8 * v + u));
			}
		if (!unit) {
			if (u0 + w < 8) CHECK(!bit(left, u0 + w, v0)); // the run ended at a clear bit (bits before it in the row were taken by earlier rectangles or are clear)
			if (v0 + h < 8) {
				bool whole = true;
				for (int u = u0; u < u0 + w; ++u) whole = whole && bit(left, u, v0 + h);
				CHECK(!whole);
			}
		}
		++quads;
		faces += static_cast<uint32_t>(w * h);
	});
	CHECK(left == 0 && rounds <= 64);
	CHECK(faces == static_cast<uint32_t>(__builtin_popcountll(mask)));
	CHECK(bm::mesh_cover_count(mask, unit) == (quads | faces << 16));
}

// 2.  the ten voxels of row (y, z) from x0 - 1 on, as the kernel stages them: 0 outside the volume
uint16_t stage_row(const uint8_t* volume, const bm::MeshDims& d, int x0, int y, int z) {
	uint16_t bits = 0;
	if (y < 0 || z < 0 || y >= d.extent[1] || z >= d.extent[2]) return 0;
	for (int j = 0; j < 10; ++j) {
		const int x = x0 - 1 + j;
		if (x >= 0 && x < d.extent[0] && volume[z * d.slice_pitch + y * d.row_pitch + x] != 0) bits |= static_cast<uint16_t>(1u << j);
	}
	return bits;
}

struct Walk {
	std::vector<bm_quad> quads;
	uint64_t faces = 0, dropped = 0, cells = 0;
};

Walk walk_lanes(const uint8_t* volume, const bm::MeshDims& d) {
	Walk out;
	for (uint32_t c = 0; c < d.cells; ++c) {
		uint16_t rows[bm::kMeshRows]; // the kernel's LDS
		int32_t i0[3];
		bm::mesh_cell_origin(d, c, i0);
		bool any = false, hole = false;
		for (int lane = 0; lane < 64; ++lane)
			for (int k = 0; k < 2; ++k) {
				const int r = lane + 64 * k;
				if (r >= bm::kMeshRows) continue;
				rows[r] = stage_row(volume, d, i0[0], i0[1] - 1 + r % 10, i0[2] - 1 + r / 10);
				any = any || rows[r] != 0;
				const uint32_t full = bm::mesh_row_full_mask(r);
				hole = hole || (rows[r] & full) != full;
			}
		uint32_t valid[3];
		int32_t w0[3];
		for (int a = 0; a < 3; ++a) {
			valid[a] = bm::mesh_valid8(d, a, i0[a]);
			w0[a] = i0[a] + d.lo[a];
		}
		++out.cells;
		const bool walk = any && hole;
		if (!walk) ++out.dropped;
		// a dropped cell has no face: walk it all the same and see that nothing comes out
		for (int lane = 0; lane < bm::kMeshLanes; ++lane) {
			const uint64_t mask = bm::mesh_lane_mask(rows, lane, valid);
			if (!walk) CHECK(mask == 0);
			bm::mesh_cover(mask, d.unit != 0, [&](int u0, int v0, int w, int h) {
				const bm::MeshQuad q = bm::mesh_quad(w0, lane, u0, v0, w, h);
				out.quads.push_back({q.x, q.y, q.z, q.shape});
				out.faces += static_cast<uint64_t>(w * h);
			});
		}
	}
	return out;
}

// 3.
void check_triangles(const bm_quad& q) {
	float t[18], host[18];
	bm::mesh_quad_triangles({q.x, q.y, q.z, q.shape}, t);
	CHECK(bm_host_mesh_triangles(&q, 1, host) == 0 && std::memcmp(t, host, sizeof t) == 0);
	const int d = static_cast<int>(q.shape & 15u), a = d >> 1, w = static_cast<int>((q.shape >> 4) & 15u), h = static_cast<int>((q.shape >> 8) & 15u);
	const int32_t c[3] = {q.x, q.y, q.z};
	double area = 0;
	for (int k = 0; k < 2; ++k) {
		const float* p = t + 9 * k;
		double e1[3], e2[3], n[3];
		for (int i = 0; i < 3; ++i) {
			e1[i] = static_cast<double>(p[3 + i]) - p[i];
			e2[i] = static_cast<double>(p[6 + i]) - p[i];
		}
		n[0] = e1[1] * e2[2] - e1[2] * e2[1];
		n[1] = e1[2] * e2[0] - e1[0] * e2[2];
		n[2] = e1[0] * e2[1] - e1[1] * e2[0];
		for (int i = 0; i < 3; ++i) CHECK(i == a ? ((d & 1) ? n[i] > 0 : n[i] < 0) : n[i] == 0); // counter-clockwise seen from outside
		area += (n[a] < 0 ? -n[a] : n[a]) / 2;
		for (int v = 0; v < 3; ++v) {
			CHECK(p[3 * v + a] == static_cast<float>(c[a] + (d & 1)));
			for (int i = 0; i < 3; ++i)
				if (i != a) CHECK(p[3 * v + i] >= static_cast<float>(c[i]) && p[3 * v + i] <= static_cast<float>(c[i] + 8));
		}
	}
	CHECK(area == static_cast<double>(w * h));
}

} // namespace

int main(int argc, char** argv) {
	const int rounds = argc > 1 ? std::atoi(argv[1]) : 40;
	std::mt19937_64 rng(12345);
	long masks = 0;
	for (uint64_t m = 0; m < 65536; ++m)
		for (int shift : {0, 24, 48})
			for (int unit = 0; unit < 2; ++unit) {
				check_cover(m << shift, unit != 0);
				++masks;
			}
	for (int i = 0; i < 100000; ++i) {
		uint64_t m = rng();
		if (i % 3 == 1) m |= rng(); // denser: larger rectangles
		if (i % 3 == 2) m |= rng() | rng();
		check_cover(m, false);
		check_cover(m, true);
		masks += 2;
	}
	check_cover(~uint64_t{0}, false);

	long cells = 0, dropped = 0, quads = 0, triangles = 0;
	for (int round = 0; round < rounds; ++round) {
		bm_mesh_params p{};
		for (int a = 0; a < 3; ++a) {
			p.extent[a] = round % 7 == 3 || round % 7 == 5 ? 26 + static_cast<int>(rng() % 8) : 3 + static_cast<int>(rng() % (round % 4 == 0 ? 30 : 14));
			p.lo[a] = static_cast<int>(rng() % 41) - 20;
		}
		if (round % 5 == 0) p.lo[0] = -(1 << 23), p.lo[1] = (1 << 23) - p.extent[1];
		p.flags = static_cast<uint32_t>(round % 4); // HALO, UNIT_FACES, both, none
		const int64_t row = p.extent[0] + static_cast<int>(rng() % 5), slice = row * (p.extent[1] + static_cast<int>(rng() % 3));
		if (round % 2) p.row_pitch = row, p.slice_pitch = slice;
		std::vector<uint8_t> volume(static_cast<size_t>(slice) * p.extent[2]);
		const unsigned density = round % 3 == 0 ? 20 : (round % 3 == 1 ? 128 : 245); // of 256: full cells and their facing slices do occur
		for (uint8_t& v : volume) v = (rng() & 255u) < density ? static_cast<uint8_t>(1 + rng() % 255) : 0;
		if (round % 7 == 3) std::fill(volume.begin(), volume.end(), uint8_t{9});                             // cells with no hole, and
		if (round % 7 == 5) std::fill(volume.begin() + static_cast<std::ptrdiff_t>(volume.size() / 2), volume.end(), uint8_t{0}); // cells with nothing
		const bm::MeshDims d = bm::mesh_dims(bm::mesh_params_view(p));
		const Walk walk = walk_lanes(volume.data(), d);
		bm_mesh_result res{~uint64_t{0}, ~uint64_t{0}};
		CHECK(bm_host_mesh_quads(&p, volume.data(), nullptr, 0, &res) == 0);
		CHECK(res.quads == walk.quads.size() && res.faces == walk.faces);
		const uint64_t capacity = round % 3 == 0 ? res.quads / 2 : res.quads;
		std::vector<bm_quad> host(capacity + 1, bm_quad{-7, -7, -7, 0xFFFFFFFFu});
		CHECK(bm_host_mesh_quads(&p, volume.data(), host.data(), capacity, &res) == 0);
		CHECK(res.quads == walk.quads.size() && res.faces == walk.faces);
		CHECK(capacity <= walk.quads.size() && (capacity == 0 || std::memcmp(host.data(), walk.quads.data(), capacity * sizeof(bm_quad)) == 0));
		CHECK(host[capacity].shape == 0xFFFFFFFFu && host[capacity].x == -7);
		for (size_t i = 0; i < walk.quads.size(); i += 1 + walk.quads.size() / 200) {
			check_triangles(walk.quads[i]);
			++triangles;
		}
		cells += static_cast<long>(walk.cells);
		dropped += static_cast<long>(walk.dropped);
		quads += static_cast<long>(walk.quads.size());
	}

	// 4.
	long refused = 0;
	{
		std::vector<uint8_t> volume(8 * 8 * 8, 1);
		std::vector<bm_quad> out(64);
		bm_mesh_result res{};
		auto call = [&](auto change, const uint8_t* v, bm_quad* q, uint64_t cap, bm_mesh_result* r) {
			bm_mesh_params p{};
			p.extent[0] = p.extent[1] = p.extent[2] = 8;
			change(p);
			const int e = bm_host_mesh_quads(&p, v, q, cap, r);
			if (e == BM_EINVAL) ++refused;
			return e;
		};
		auto vol = volume.data();
		CHECK(call([](bm_mesh_params&) {}, vol, out.data(), 64, &res) == 0 && res.quads == 6 && res.faces == 6 * 64);
		CHECK(call([](bm_mesh_params& p) { p.extent[0] = 0; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params& p) { p.extent[2] = 16385; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params& p) { p.extent[1] = 2; p.flags = BM_MESH_HALO; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params& p) { p.extent[0] = p.extent[1] = 16384; p.extent[2] = 8; }, vol, out.data(), 64, &res) == BM_EINVAL); // 2^31 voxels
		CHECK(call([](bm_mesh_params& p) { p.row_pitch = 7; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params& p) { p.slice_pitch = 63; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params& p) { p.row_pitch = -8; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params& p) { p.flags = 4; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params& p) { p.reserved = 1; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params& p) { p.lo[0] = (1 << 23) - 7; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params& p) { p.lo[2] = -(1 << 23) - 1; }, vol, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params&) {}, nullptr, out.data(), 64, &res) == BM_EINVAL);
		CHECK(call([](bm_mesh_params&) {}, vol, out.data(), 64, nullptr) == BM_EINVAL);
		CHECK(call([](bm_mesh_params&) {}, vol, nullptr, 1, &res) == BM_EINVAL);
		CHECK(bm_host_mesh_quads(nullptr, vol, out.data(), 64, &res) == BM_EINVAL && ++refused);
		CHECK(bm_host_mesh_triangles(nullptr, 1, nullptr) == BM_EINVAL && ++refused);
		CHECK(bm_host_mesh_triangles(out.data(), -1, nullptr) == BM_EINVAL && ++refused);
		CHECK(bm_host_mesh_triangles(nullptr, 0, nullptr) == 0);
		CHECK(call([](bm_mesh_params& p) { p.lo[0] = (1 << 23) - 8; p.lo[1] = -(1 << 23); }, vol, out.data(), 64, &res) == 0);
	}
	std::printf("masks %ld cells %ld dropped %ld quads %ld triangles %ld refused %ld failures %ld\n", masks, cells, dropped, quads, triangles, refused, failures);
	return failures ? 1 : 0;
}
