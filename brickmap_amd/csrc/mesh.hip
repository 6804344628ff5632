// mesh.hip -- voxels -> the quads of their surface on the device (bm_mesh_quads, bm_mesh_triangles), by the rules of mesh.h.
//
// The quads of a cell follow those of the cells before it, so the work is counted, scanned and done again:
//
//   count     : one wave64 (one workgroup) per 8^3 cell.  The cell's 10^3 neighbourhood is staged as bits -- a lane takes two of its 100
//               (y, z) rows, ten voxels each: aligned words where all four bytes are voxels of the row, single bytes otherwise -- into
//               200 bytes of LDS.  A ballot drops the cell when nothing is set or when the cell and its six facing slices are all set.
//               Lanes 0 ... 47 (8 d + s) build their 8 x 8 face mask from the rows and run the greedy cover, counting; a wave reduction
//               leaves the cell's quads in the workspace and one 64-bit add per wave sums the faces in the result.
//   scan      : a workgroup turns 256 cell counts into their exclusive prefixes in place and leaves their sum; voxelize.hip's scan of
//               workgroup sums (launch_offsets_scan) turns those into 64-bit offsets and the total, which becomes result.quads.
//   emit      : the walk of count again (recomputing is cheaper than keeping 48 masks per cell); a lane's first quad goes to the cell's
//               offset + the exclusive prefix of the lanes' counts over the wave, and every quad below the capacity is one 16-byte store.
//               Cells without quads end after two loads.
//   triangles : one lane per quad, 16 bytes in, 72 bytes out.
//
// Every loop is bounded (two rows, 64 rounds of the cover, the scan); nothing waits for another workgroup; the one atomic is the face
// total; nothing is read in the kernel that wrote it.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "global_mem.h"
#include "kernels.h"
#include "mesh.h"

namespace bm {

namespace {

constexpr int kThreads = 256;

typedef __attribute__((address_space(1))) unsigned long long g_ull;
typedef u32x4 QuadWords __attribute__((aligned(4))); // a bm_quad: 16 bytes at a 4-byte aligned place
typedef __attribute__((address_space(1))) QuadWords g_quad;
typedef __attribute__((address_space(1))) float g_f32;

// the four bytes of a word -> bit k: byte k is not 0
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) {
	const uint32_t nz = ((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u) >> 7;
	return ((nz * 0x00204081u) >> 21) & 15u;
}

// the ten voxels x0 - 1 ... x0 + 8 of row (y, z) as bits; voxels outside the volume are 0
__device__ __forceinline__ uint32_t stage_row(const uint8_t* __restrict__ volume, const MeshDims& d, int32_t x0, int32_t y, int32_t z) {
	if (y < 0 || z < 0 || y >= d.extent[1] || z >= d.extent[2]) return 0;
	const int64_t at = static_cast<int64_t>(z) * d.slice_pitch + static_cast<int64_t>(y) * d.row_pitch; // the row's voxel 0
	const int32_t first = x0 - 1, nx = d.extent[0];
	// the aligned words that hold bytes first ... first + 9: at most four
	const int32_t lead = static_cast<int32_t>((reinterpret_cast<uintptr_t>(volume) + static_cast<uintptr_t>(at + first)) & 3u);
	uint32_t bits = 0;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const int32_t xw = first - lead + 4 * k; // the voxel of the word's first byte
		const int32_t j = xw - first;            // its place in the ten bits, -3 ... 12
		if (j >= 10) continue;
		uint32_t four = 0;
		if (xw >= 0 && xw + 4 <= nx) {
			four = nonzero_bytes(*(const g_u32*)((const g_u8*)volume + (at + xw)));
		} else {
#pragma unroll
			for (int b = 0; b < 4; ++b) {
				const int32_t x = xw + b;
				if (x >= 0 && x < nx && x >= first && x < first + 10 && ld8(volume, static_cast<size_t>(at + x)) != 0) four |= 1u << b;
			}
		}
		bits |= j >= 0 ? four << j : four >> -j;
	}
	return bits & 0x3FFu;
}

// Stages the cell's rows into `rows` and tells whether the cell can have a face; then `valid` and `w0` are set.
__device__ __forceinline__ bool stage_cell(const uint8_t* __restrict__ volume, const MeshDims& d, uint32_t cell, uint16_t* rows, uint32_t valid[3], int32_t w0[3]) {
	const int lane = static_cast<int>(threadIdx.x);
	int32_t i0[3];
	mesh_cell_origin(d, cell, i0);
	bool any = false, hole = false;
#pragma unroll
	for (int k = 0; k < 2; ++k) {
		const int r = lane + 64 * k;
		if (r < kMeshRows) {
			const uint32_t bits = stage_row(volume, d, i0[0], i0[1] - 1 + r % 10, i0[2] - 1 + r / 10);
			rows[r] = static_cast<uint16_t>(bits);
			any = any || bits != 0;
			const uint32_t full = mesh_row_full_mask(r);
			hole = hole || (bits & full) != full;
		}
	}
	const bool faces = __ballot(any) != 0 && __ballot(hole) != 0;
	__syncthreads(); // (one wave: the rows are in LDS before any lane reads another's)
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		valid[a] = mesh_valid8(d, a, i0[a]);
		w0[a] = i0[a] + d.lo[a];
	}
	return faces;
}

} // namespace

// counts[c] = the quads of cell c; *faces += the faces of all cells
__global__ __launch_bounds__(64) void mesh_count(const uint8_t* __restrict__ volume, uint32_t* __restrict__ counts, unsigned long long* __restrict__ faces, const MeshDims d) {
	__shared__ uint16_t rows[kMeshRows];
	const uint32_t cell = blockIdx.x, lane = threadIdx.x;
	uint32_t valid[3];
	int32_t w0[3];
	uint32_t n = 0;
	if (stage_cell(volume, d, cell, rows, valid, w0) && lane < kMeshLanes) n = mesh_cover_count(mesh_lane_mask(rows, static_cast<int>(lane), valid), d.unit != 0);
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) n += __shfl_xor(n, s, 64); // quads below 2^11 and faces below 2^12 in the two halves
	if (lane == 0) {
		st32(counts, cell, n & 0xFFFFu);
		if (n >> 16) __hip_atomic_fetch_add((g_ull*)faces, static_cast<unsigned long long>(n >> 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// counts[256 b ... 256 b + 255] -> their exclusive prefixes, in place; block_off[b] = their sum
__global__ __launch_bounds__(kThreads) void mesh_scan(uint32_t* __restrict__ counts, uint64_t* __restrict__ block_off, uint32_t cells) {
	__shared__ uint64_t lds[kThreads];
	const uint32_t i = blockIdx.x * kMeshScanBlock + threadIdx.x;
	const uint32_t v = i < cells ? ld32(counts, i) : 0u;
	uint64_t total;
	const uint64_t before = block_scan(v, lds, &total);
	if (i < cells) st32(counts, i, static_cast<uint32_t>(before));
	if (threadIdx.x == 0) st64(block_off, blockIdx.x, total);
}

// prefix: the cells' prefixes within their scan block; block_off: the blocks' offsets, entry nblocks = the total
__global__ __launch_bounds__(64) void mesh_emit(const uint8_t* __restrict__ volume, const uint32_t* __restrict__ prefix, const uint64_t* __restrict__ block_off,
												 void* __restrict__ quads, const uint64_t capacity, const MeshDims d) {
	__shared__ uint16_t rows[kMeshRows];
	const uint32_t cell = blockIdx.x, lane = threadIdx.x;
	const uint32_t b = cell / kMeshScanBlock;
	const uint64_t off = ld64(block_off, b);
	const uint64_t begin = off + ld32(prefix, cell);
	const uint64_t end = ((cell + 1) % kMeshScanBlock == 0 || cell + 1 == d.cells) ? ld64(block_off, b + 1) : off + ld32(prefix, cell + 1);
	if (begin == end || begin >= capacity) return; // (the same for every lane)
	uint32_t valid[3];
	int32_t w0[3];
	(void)stage_cell(volume, d, cell, rows, valid, w0);
	const uint64_t mask = lane < kMeshLanes ? mesh_lane_mask(rows, static_cast<int>(lane), valid) : 0;
	const uint32_t mine = mesh_cover_count(mask, d.unit != 0) & 0xFFFFu;
	uint32_t upto = mine; // inclusive prefix over the wave
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) {
		const uint32_t other = __shfl_up(upto, s, 64);
		if (lane >= static_cast<uint32_t>(s)) upto += other;
	}
	uint64_t at = begin + (upto - mine);
	mesh_cover(mask, d.unit != 0, [&](int u0, int v0, int w, int h) {
		if (at < capacity) {
			const MeshQuad q = mesh_quad(w0, static_cast<int>(lane), u0, v0, w, h);
			u32x4 rec;
			rec.x = static_cast<uint32_t>(q.x);
			rec.y = static_cast<uint32_t>(q.y);
			rec.z = static_cast<uint32_t>(q.z);
			rec.w = q.shape;
			((g_quad*)quads)[at] = rec;
		}
		++at;
	});
}

__global__ __launch_bounds__(kThreads) void mesh_triangles(const void* __restrict__ quads, float* __restrict__ triangles, const uint64_t n) {
	const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) return;
	const u32x4 rec = ((const g_quad*)quads)[i];
	const MeshQuad q = {static_cast<int32_t>(rec.x), static_cast<int32_t>(rec.y), static_cast<int32_t>(rec.z), rec.w};
	float out[18];
	mesh_quad_triangles(q, out);
#pragma unroll
	for (int k = 0; k < 18; ++k) ((g_f32*)triangles)[i * 18 + k] = out[k];
}

// ---- host-callable launchers (kernels.h)
void launch_mesh_quads(const MeshDims& d, const uint8_t* volume, void* quads, uint64_t capacity, void* result, void* workspace, hipStream_t stream, hipEvent_t* marks) {
	int mark = 0;
	auto stamp = [&]() { if (marks) (void)hipEventRecord(marks[mark++], stream); };
	uint32_t* counts = static_cast<uint32_t*>(workspace);
	uint64_t* block_off = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(workspace) + mesh_cells_bytes(d));
	const uint32_t nblocks = mesh_scan_blocks(d);
	stamp();
	(void)hipMemsetAsync(result, 0, 16, stream);
	hipLaunchKernelGGL(mesh_count, dim3(d.cells), dim3(64), 0, stream, volume, counts, reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(result) + 8), d);
	stamp();
	hipLaunchKernelGGL(mesh_scan, dim3(nblocks), dim3(kThreads), 0, stream, counts, block_off, d.cells);
	launch_offsets_scan(block_off, nblocks, 1, stream);
	(void)hipMemcpyAsync(result, block_off + nblocks, 8, hipMemcpyDeviceToDevice, stream);
	stamp();
	if (capacity > 0) hipLaunchKernelGGL(mesh_emit, dim3(d.cells), dim3(64), 0, stream, volume, counts, block_off, quads, capacity, d);
	stamp();
}

void launch_mesh_triangles(const void* quads, uint64_t n, float* triangles, hipStream_t stream) {
	if (n == 0) return;
	hipLaunchKernelGGL(mesh_triangles, dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, quads, triangles, n);
}

} // namespace bm
