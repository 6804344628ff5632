// voxelize_host.cpp -- bm_host_voxelize: mesh voxelization of host memory by the rules of voxelize.h, as plain loops: every triangle marks
// the voxels of its clipped bounds that pass the surface tests in one bit plane and toggles its crossing of every covered column in
// another; then every row takes the running parity of its crossings and is written out.
// Needs nothing else of the library (no HIP header, no scene): tests/voxelize_check.cpp links this file alone.
#include <string>
#include <vector>

#include "../../include/brickmap.h"
#include "voxelize.h"

namespace bm {
// the library's error slot (error.h, defined in scene.cpp); absent -- a null address -- in a program that links this file alone
__attribute__((weak)) void set_error(const std::string& msg);
} // namespace bm

namespace {

int refuse(const char* why) {
	if (bm::set_error) bm::set_error(std::string("bm_host_voxelize: ") + why);
	return BM_EINVAL;
}

} // namespace

extern "C" int bm_host_voxelize(const bm_voxelize_params* params, int64_t n, const float* triangles, uint8_t* volume, bm_voxelize_result* result) {
	using namespace bm;
	if (!params) return refuse("null params");
	const VxParamsView pv = voxelize_params_view(*params);
	if (const char* why = voxelize_params_problem(pv, n)) return refuse(why);
	if (!volume || (n > 0 && !triangles)) return refuse("null buffer");
	const int nx = pv.extent[0], ny = pv.extent[1], nz = pv.extent[2];
	const int64_t row_pitch = voxelize_row_pitch(pv), slice_pitch = voxelize_slice_pitch(pv);
	const size_t words = voxelize_row_words(nx), rows = static_cast<size_t>(ny) * static_cast<size_t>(nz);
	const bool surface = (pv.mode & kVxSurface) != 0, solid = (pv.mode & kVxSolid) != 0;
	std::vector<uint32_t> marked(surface ? rows * words : 0), crossings(solid ? rows * words : 0);
	bm_voxelize_result res = {0, 0, 0};

	for (int64_t i = 0; i < n; ++i) {
		VxTri t;
		const int kind = vx_snap(triangles + 9 * i, pv.lo, t);
		if (kind == kVxRejected) { ++res.rejected; continue; }
		if (kind == kVxDegenerate) { ++res.degenerate; continue; }
		if (surface) {
			int x0, x1, y0, y1, z0, z1;
			vx_surface_range(t, 0, nx, x0, x1);
			vx_surface_range(t, 1, ny, y0, y1);
			vx_surface_range(t, 2, nz, z0, z1);
			for (int z = z0; z <= z1; ++z)
				for (int y = y0; y <= y1; ++y)
					for (int x = x0; x <= x1; ++x)
						if (vx_surface_voxel(t, x, y, z)) marked[(static_cast<size_t>(z) * ny + y) * words + (x >> 5)] |= 1u << (x & 31);
		}
		if (solid && t.n[0] != 0) {
			int y0, y1, z0, z1;
			vx_solid_range(t, 1, ny, y0, y1);
			vx_solid_range(t, 2, nz, z0, z1);
			for (int z = z0; z <= z1; ++z)
				for (int y = y0; y <= y1; ++y) {
					int k;
					if (vx_solid_crossing(t, y, z, nx, &k)) crossings[(static_cast<size_t>(z) * ny + y) * words + (k >> 5)] ^= 1u << (k & 31);
				}
		}
	}

	const bool keep = (pv.flags & kVxKeep) != 0;
	for (int z = 0; z < nz; ++z)
		for (int y = 0; y < ny; ++y) {
			const size_t row = (static_cast<size_t>(z) * ny + y) * words;
			uint8_t* out = volume + z * slice_pitch + y * row_pitch;
			uint32_t carry = 0; // all ones while the crossings so far are odd
			for (size_t w = 0; w < words; ++w) {
				uint32_t bits = surface ? marked[row + w] : 0u;
				if (solid) {
					const uint32_t inside = vx_prefix_xor(crossings[row + w]) ^ carry;
					carry = (inside >> 31) ? 0xFFFFFFFFu : 0u;
					bits |= inside;
				}
				for (int b = 0; b < 32 && static_cast<int>(32 * w) + b < nx; ++b) {
					const uint8_t v = (bits >> b) & 1u;
					out[32 * w + b] = keep ? static_cast<uint8_t>(out[32 * w + b] | v) : v;
				}
			}
			if (carry) ++res.open_columns;
		}
	if (result) *result = res;
	return 0;
}
