// viewfield.hip -- builds the view plane, the tenth plane of the cube field that primary rays read (viewfield.h: the plan of a camera
// position and the rule of a cell's byte), from the eight octant planes and the escape table: one lane per cell, which starts at its
// octant's cube and extends it shell by shell along the pencil of rays that reach the cell from the camera.  The octant planes carry
// the occupancy (byte 0) and the empty cube the extension starts from, so the index grid is not read at all.
// The whole plane is rebuilt when the world or the camera's position has changed and a resting camera's frame is about to use it
// (scene.cpp ensure_view_plane); the cost is in profiles/r12_view_plane.txt.
#include <hip/hip_runtime.h>

#include "escape.h"
#include "global_mem.h"
#include "kernels.h"
#include "viewfield.h"

namespace bm {
namespace {

// lane t = (z * cells + y) * cells + x
__global__ __launch_bounds__(256) void view_field_cells(const uint32_t* __restrict__ escape, uint8_t* __restrict__ field, const ViewBuild u) {
	const uint32_t cells = static_cast<uint32_t>(u.cells), total = cells * cells * static_cast<uint32_t>(u.cells_height);
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= total) return;
	const int c[3] = {static_cast<int>(t % cells), static_cast<int>(t / cells % cells), static_cast<int>(t / (cells * cells))};
	const int n[3] = {u.cells, u.cells, u.cells_height};
	auto at = [&](int o, int x, int y, int z) { // inside the grid: 0 <= x < cells ...
		return static_cast<size_t>(o) * u.cf_plane + static_cast<size_t>(z + 1) * u.cf_pxy + (static_cast<size_t>(y + 1) << u.cf_shift) + static_cast<size_t>(x + 1);
	};
	auto cube = [&](int o, int x, int y, int z) { return static_cast<int>(ld8(field, at(o, x, y, z))); };
	auto threshold = [&](int o) {
		return escape_height_of(o, ld32(escape, escape_index(o, u.cf_shift, u.cf_pxy, u.plan.cell[0], u.plan.cell[1])), u.cf_pxy, u.cf_plane);
	};
	st8(field, at(9, c[0], c[1], c[2]), static_cast<uint32_t>(view_cell_byte(u.plan, n, c, cube, threshold)));
}

} // namespace

void launch_view_build(const uint32_t* escape, uint8_t* field, const ViewBuild& u, hipStream_t stream) {
	const uint32_t total = static_cast<uint32_t>(u.cells) * static_cast<uint32_t>(u.cells) * static_cast<uint32_t>(u.cells_height);
	hipLaunchKernelGGL(view_field_cells, dim3((total + 255) / 256), dim3(256), 0, stream, escape, field, u);
}

} // namespace bm
