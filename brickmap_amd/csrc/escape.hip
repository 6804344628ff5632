// escape.hip -- builds the escape-height table of the walk (escape.h: the rule, the table's definition and its entries) from the
// index grid, on the GPU:
//   1. column scan: the highest and the lowest occupied cell of every column of an xy footprint (the whole grid, or the columns an
//      edit batch touched -- a removal is exact because the column is scanned again, not patched);
//   2. the running max / min of those over the four xy-quadrant directions, for the whole table: along y into the table (octant o
//      takes tops or bottoms by its z direction), then along x in place, where the threshold becomes the stored entry.
// They follow the cube-field update on the load stream (kernels.h launch_escape_update) and add 0.10 ms to an edit batch's 0.38 ms field step on
// a 1024^3 world, 0.39 ms to 33.8 ms on 4096^3 (profiles/r08_escape.txt 5): the quadrant passes are one lane per line, serial along it.
#include <hip/hip_runtime.h>

#include "escape.h"
#include "global_mem.h"
#include "kernels.h"

namespace bm {
namespace {

// one lane per column of the footprint: cols[y * cells + x] = top, cols[cells^2 + y * cells + x] = bottom
__global__ void escape_columns(const uint32_t* __restrict__ index_grid, int32_t* __restrict__ cols, const EscapeUpdate u) {
	const uint32_t nx = u.x1 - u.x0, ny = u.y1 - u.y0;
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= nx * ny) return;
	const int x = u.x0 + static_cast<int>(t % nx), y = u.y0 + static_cast<int>(t / nx);
	int top = escape_none(0, u.cells_height), bottom = escape_none(4, u.cells_height);
	for (int z = 0; z < u.cells_height; ++z) escape_column_fold(top, bottom, z, ld32(index_grid, index_word_at(u.sg_xy, u.sg_xy2, x, y, z)) != 0u);
	const size_t c = static_cast<size_t>(y) * u.cells + x, plane = static_cast<size_t>(u.cells) * u.cells;
	((g_i32*)cols)[c] = top;
	((g_i32*)cols)[plane + c] = bottom;
}

// along y: one lane per (octant, x), from the quadrant's far row to its near one; the table holds plain thresholds afterwards
__global__ void escape_pass_y(const int32_t* __restrict__ cols, uint32_t* __restrict__ table, const EscapeUpdate u) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= 8u * u.cells) return;
	const int o = static_cast<int>(t / u.cells), x = static_cast<int>(t % u.cells);
	const size_t plane = static_cast<size_t>(u.cells) * u.cells;
	const int step = (o & 2) ? 1 : -1; // the quadrant of a ray that moves down in y lies at smaller y: scan upwards from row 0
	int acc = escape_none(o, u.cells_height);
	for (int k = 0, y = (o & 2) ? 0 : u.cells - 1; k < u.cells; ++k, y += step) {
		const size_t c = static_cast<size_t>(y) * u.cells + x;
		acc = escape_fold(o, acc, ldi32(cols, c), ldi32(cols, plane + c));
		st32(table, escape_index(o, u.cf_shift, u.cf_pxy, x, y), static_cast<uint32_t>(acc));
	}
}

// along x, in place: one lane per (octant, y); writes the entries the walk reads
__global__ void escape_pass_x(uint32_t* __restrict__ table, const EscapeUpdate u) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= 8u * u.cells) return;
	const int o = static_cast<int>(t / u.cells), y = static_cast<int>(t % u.cells);
	const int step = (o & 1) ? 1 : -1;
	int acc = escape_none(o, u.cells_height);
	for (int k = 0, x = (o & 1) ? 0 : u.cells - 1; k < u.cells; ++k, x += step) {
		const size_t i = escape_index(o, u.cf_shift, u.cf_pxy, x, y);
		const int v = static_cast<int>(ld32(table, i));
		acc = escape_fold(o, acc, v, v);
		st32(table, i, escape_entry(o, acc, u.cf_pxy, u.cf_plane));
	}
}

} // namespace

size_t escape_columns_bytes(int cells) { return 2 * static_cast<size_t>(cells) * cells * sizeof(int32_t); }

void launch_escape_update(const uint32_t* index_grid, int32_t* cols, uint32_t* table, const EscapeUpdate& u, hipStream_t stream) {
	const uint32_t columns = static_cast<uint32_t>(u.x1 - u.x0) * static_cast<uint32_t>(u.y1 - u.y0), lines = 8u * u.cells;
	if (columns) hipLaunchKernelGGL(escape_columns, dim3((columns + 63) / 64), dim3(64), 0, stream, index_grid, cols, u);
	hipLaunchKernelGGL(escape_pass_y, dim3((lines + 63) / 64), dim3(64), 0, stream, cols, table, u);
	hipLaunchKernelGGL(escape_pass_x, dim3((lines + 63) / 64), dim3(64), 0, stream, table, u);
}

} // namespace bm
