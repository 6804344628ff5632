// mesh_host.cpp -- bm_host_mesh_quads and bm_host_mesh_triangles: surface extraction of host memory by the rules of mesh.h, as plain
// loops: every cell in (z, y, x) order, every direction, every slice; the slice's mask is filled voxel by voxel from the volume -- solid,
// inside the meshed range, the neighbour empty -- and the greedy cover of mesh.h emits its rectangles.
// Needs nothing else of the library (no HIP header, no scene): tests/mesh_check.cpp links this file alone.
#include <string>

#include "../../include/brickmap.h"
#include "mesh.h"

namespace bm {
// the library's error slot (error.h, defined in scene.cpp); absent -- a null address -- in a program that links this file alone
__attribute__((weak)) void set_error(const std::string& msg);
} // namespace bm

namespace {

int refuse(const char* who, const char* why) {
	if (bm::set_error) bm::set_error(std::string(who) + ": " + why);
	return BM_EINVAL;
}

} // namespace

extern "C" int bm_host_mesh_quads(const bm_mesh_params* params, const uint8_t* volume, bm_quad* quads, uint64_t capacity, bm_mesh_result* result) {
	using namespace bm;
	static_assert(sizeof(bm_quad) == sizeof(MeshQuad) && sizeof(bm_quad) == 16 && sizeof(bm_mesh_result) == 16, "the records are 16 bytes");
	const char* who = "bm_host_mesh_quads";
	if (!params) return refuse(who, "null params");
	const MeshParamsView pv = mesh_params_view(*params);
	if (const char* why = mesh_params_problem(pv)) return refuse(who, why);
	if (!volume || !result) return refuse(who, "null volume or result");
	if (!quads && capacity > 0) return refuse(who, "null quads with a capacity above 0");
	const MeshDims d = mesh_dims(pv);
	auto solid = [&](int x, int y, int z) {
		if (x < 0 || y < 0 || z < 0 || x >= d.extent[0] || y >= d.extent[1] || z >= d.extent[2]) return false;
		return volume[z * d.slice_pitch + y * d.row_pitch + x] != 0;
	};
	uint64_t total = 0, faces = 0;
	for (uint32_t c = 0; c < d.cells; ++c) {
		int32_t i0[3];
		mesh_cell_origin(d, c, i0);
		const int32_t w0[3] = {i0[0] + d.lo[0], i0[1] + d.lo[1], i0[2] + d.lo[2]};
		for (int dir = 0; dir < 6; ++dir) {
			const int a = dir >> 1, ua = mesh_axis_u(a), va = mesh_axis_v(a), step = (dir & 1) ? 1 : -1;
			for (int s = 0; s < 8; ++s) {
				uint64_t mask = 0;
				for (int v = 0; v < 8; ++v)
					for (int u = 0; u < 8; ++u) {
						int p[3];
						p[a] = i0[a] + s;
						p[ua] = i0[ua] + u;
						p[va] = i0[va] + v;
						bool meshed = true;
						for (int k = 0; k < 3; ++k) meshed = meshed && p[k] >= d.m0[k] && p[k] < d.m1[k];
						if (!meshed || !solid(p[0], p[1], p[2])) continue;
						int n[3] = {p[0], p[1], p[2]};
						n[a] += step;
						if (!solid(n[0], n[1], n[2])) mask |= uint64_t{1} << (8 * v + u);
					}
				mesh_cover(mask, d.unit != 0, [&](int u0, int v0, int w, int h) {
					if (total < capacity) {
						const MeshQuad q = mesh_quad(w0, 8 * dir + s, u0, v0, w, h);
						quads[total] = {q.x, q.y, q.z, q.shape};
					}
					++total;
					faces += static_cast<uint64_t>(w * h);
				});
			}
		}
	}
	result->quads = total;
	result->faces = faces;
	return 0;
}

extern "C" int bm_host_mesh_triangles(const bm_quad* quads, int64_t n, float* triangles) {
	using namespace bm;
	const char* who = "bm_host_mesh_triangles";
	if (n < 0 || n > (int64_t{1} << 32)) return refuse(who, "a quad count below 0 or above 2^32");
	if (n > 0 && (!quads || !triangles)) return refuse(who, "null buffer");
	for (int64_t i = 0; i < n; ++i) {
		const MeshQuad q = {quads[i].x, quads[i].y, quads[i].z, quads[i].shape};
		mesh_quad_triangles(q, triangles + 18 * i);
	}
	return 0;
}
