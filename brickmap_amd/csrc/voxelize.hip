// voxelize.hip -- triangle meshes -> voxels on the device (bm_voxelize), by the rules of voxelize.h.
//
// A triangle covers anything from a fraction of a voxel to 2048 voxels per axis and its size is only known on the device, so the work is
// laid out there, as volume.hip lays out its shapes:
//
//   plan    : one lane per triangle snaps it, counts the rejected and degenerate ones, and writes two item counts -- the 8^3 cells of its
//             clipped bounds (surface) and the 8 x 8 tiles of columns of its clipped (y, z) bounds (solid); a workgroup scans its 256
//             counts (64-bit) and leaves their sums
//   scan    : one workgroup per kind turns the workgroups' sums into exclusive offsets and the total
//   surface : persistent wave64 kernel, one item per wave at a time and a run of consecutive items per wave: the wave finds its first
//             item's triangle by binary search (workgroup offsets, then the 256 counts inside) and the later ones by stepping to the next
//             triangle, snaps it again, and drops the cell as a whole when the triangle's plane misses it; otherwise a lane takes one
//             x-row of 8 voxels and ORs its 8 bits into the surface plane with one atomic
//   solid   : the same for a tile of 8 x 8 columns: a lane tests one column and toggles the bit of its crossing in the crossings plane
//   dense   : one wave per row (y, z): the running parity of the crossings along the row (per word by shifts, across the words of the
//             wave by a ballot), OR the surface bits, the row's open end counted, and every byte of the row written once -- 16 aligned
//             bytes per lane, the ragged ends of a row byte by byte
//
// No lane's loop grows with a triangle: an item is 8 voxels or one column per lane.  The planes are written by integer atomics alone
// (OR, XOR of one bit: any order, one result) and read by the dense pass after the kernel boundary; nothing waits for another workgroup.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "global_mem.h"
#include "kernels.h"
#include "voxelize.h"

namespace bm {

namespace {

constexpr int kThreads = 256;
constexpr int kRowWordsMax = (kVxMaxExtent + 32) / 32; // 513

__device__ __forceinline__ int load_tri(const float* __restrict__ triangles, uint32_t i, const VoxelizeDims& d, VxTri& t) {
	float v[9];
#pragma unroll
	for (int k = 0; k < 9; ++k) v[k] = triangles[static_cast<size_t>(i) * 9 + k];
	return vx_snap(v, d.lo, t);
}

// the 8^3 cells of a triangle's clipped surface bounds: first cell and count per axis (count 0: nothing inside the volume)
struct CellBox {
	int c0[3];
	uint32_t nc[3];
	__device__ __forceinline__ uint64_t items() const { return static_cast<uint64_t>(nc[0]) * nc[1] * nc[2]; }
};
__device__ __forceinline__ CellBox surface_cells(const VxTri& t, const VoxelizeDims& d) {
	CellBox b;
	bool any = true;
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		int k0, k1;
		vx_surface_range(t, a, d.extent[a], k0, k1);
		any = any && k0 <= k1;
		b.c0[a] = k0 >> 3;
		b.nc[a] = static_cast<uint32_t>((k1 >> 3) - (k0 >> 3) + 1);
	}
	if (!any) b.nc[0] = b.nc[1] = b.nc[2] = 0;
	return b;
}
// the 8 x 8 tiles of a triangle's clipped columns; axis 0 is not used (c0 0, count 1)
__device__ __forceinline__ CellBox solid_tiles(const VxTri& t, const VoxelizeDims& d) {
	CellBox b;
	bool any = t.n[0] != 0;
	b.c0[0] = 0;
	b.nc[0] = 1;
#pragma unroll
	for (int a = 1; a < 3; ++a) {
		int k0, k1;
		vx_solid_range(t, a, d.extent[a], k0, k1);
		any = any && k0 <= k1;
		b.c0[a] = k0 >> 3;
		b.nc[a] = static_cast<uint32_t>((k1 >> 3) - (k0 >> 3) + 1);
	}
	if (!any) b.nc[0] = b.nc[1] = b.nc[2] = 0;
	return b;
}

} // namespace

// local[kind * n + i] = items of the triangles before i in i's workgroup; block_off[kind * (nblocks + 1) + b] = items of workgroup b
// (kind 0 = surface, 1 = solid); result: null, or the zeroed record
__global__ __launch_bounds__(kThreads) void voxelize_plan(const float* __restrict__ triangles, uint64_t* __restrict__ local, uint64_t* __restrict__ block_off,
														  uint32_t* __restrict__ result, uint32_t n, uint32_t nblocks, const VoxelizeDims d) {
	__shared__ uint64_t lds[kThreads];
	const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
	uint64_t items[2] = {0, 0};
	int kind = kVxOk;
	if (i < n) {
		VxTri t;
		kind = load_tri(triangles, i, d, t);
		if (kind == kVxOk) {
			if (d.mode & kVxSurface) items[0] = surface_cells(t, d).items();
			if (d.mode & kVxSolid) items[1] = solid_tiles(t, d).items();
		}
	}
	if (result) { // one add per wave and counter
		const uint32_t rejected = static_cast<uint32_t>(__popcll(__ballot(kind == kVxRejected))), degenerate = static_cast<uint32_t>(__popcll(__ballot(kind == kVxDegenerate)));
		if ((threadIdx.x & 63) == 0) {
			if (rejected) atomicAdd(result, rejected);
			if (degenerate) atomicAdd(result + 1, degenerate);
		}
	}
#pragma unroll
	for (int k = 0; k < 2; ++k) {
		uint64_t total;
		const uint64_t before = block_scan(items[k], lds, &total);
		if (i < n) st64(local, static_cast<size_t>(k) * n + i, before);
		if (threadIdx.x == 0) st64(block_off, static_cast<size_t>(k) * (nblocks + 1) + blockIdx.x, total);
	}
}

// workgroup k: block_off[k * (nblocks + 1) + (0 ... nblocks)): sums -> exclusive offsets; entry nblocks = the total
__global__ __launch_bounds__(kThreads) void voxelize_scan(uint64_t* __restrict__ block_off_both, uint32_t nblocks) {
	__shared__ uint64_t lds[kThreads];
	uint64_t* block_off = block_off_both + static_cast<size_t>(blockIdx.x) * (nblocks + 1);
	const uint32_t per = (nblocks + 255) / 256, first = threadIdx.x * per;
	uint64_t sum = 0;
	for (uint32_t j = first; j < first + per && j < nblocks; ++j) sum += ld64(block_off, j);
	uint64_t total;
	uint64_t run = block_scan(sum, lds, &total);
	for (uint32_t j = first; j < first + per && j < nblocks; ++j) {
		const uint64_t v = ld64(block_off, j);
		st64(block_off, j, run);
		run += v;
	}
	if (threadIdx.x == 0) st64(block_off, nblocks, total);
}

namespace {

// the triangle of item t: the last workgroup whose offset is <= t, then the last triangle in it whose offset is <= the rest; *begin =
// the triangle's first item.  t < the total, so the triangle has items.
__device__ __forceinline__ uint32_t item_triangle(uint64_t t, const uint64_t* __restrict__ local, const uint64_t* __restrict__ block_off, uint32_t n, uint32_t nblocks,
												   uint64_t* begin) {
	uint32_t a = 0, b = nblocks;
	while (b - a > 1) {
		const uint32_t mid = (a + b) >> 1;
		if (ld64(block_off, mid) <= t) a = mid; else b = mid;
	}
	const uint64_t off = ld64(block_off, a), rest = t - off;
	const uint32_t first = a * 256;
	a = 0;
	b = n - first < 256u ? n - first : 256u;
	while (b - a > 1) {
		const uint32_t mid = (a + b) >> 1;
		if (ld64(local, first + mid) <= rest) a = mid; else b = mid;
	}
	*begin = off + ld64(local, first + a);
	return first + a;
}

} // namespace

// SOLID = false: an item is an 8^3 cell, a lane ORs the 8 bits of one x-row into `plane`; true: an item is a tile of 8 x 8 columns, a lane
// toggles its column's crossing
template <bool SOLID>
__global__ __launch_bounds__(kThreads) void voxelize_items(const float* __restrict__ triangles, const uint64_t* __restrict__ local, const uint64_t* __restrict__ block_off,
														   uint32_t* __restrict__ plane, const uint32_t n, const uint32_t nblocks, const VoxelizeDims d) {
	const uint64_t total = ld64(block_off, nblocks);
	const uint32_t lane = threadIdx.x & 63;
	// (every lane keeps the wave's triangle itself: told that it is the same for all of them -- the wave's number through readfirstlane --
	// the compiler moves it and the edge functions into scalar registers, more than there are, and spills them)
	const uint64_t waves = static_cast<uint64_t>(gridDim.x) * 4, wave = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
	// a wave takes a run of consecutive items, so that the triangle of its next item is the one it has or one of the next few: the search
	// (some twenty dependent loads) is for a wave's first item and for what follows a stretch of triangles without items
	const uint64_t per = (total + waves - 1) / waves;
	const uint64_t first = wave * per, last = first + per < total ? first + per : total;
	uint32_t r = 0;
	uint32_t j = 0, cnt = 0; // the item's place among the items of triangle r and their number (below 257^3); 0: no triangle yet
	VxTri t;
	CellBox box;
	box.c0[0] = box.c0[1] = box.c0[2] = 0;
	box.nc[0] = box.nc[1] = box.nc[2] = 1;
	for (uint64_t item = first; item < last; ++item, ++j) {
		if (j >= cnt) { // triangle r has no more items: this one is the first of the next triangle that has any
			bool found = false;
			if (cnt != 0) {
				for (int tries = 0; tries < 4 && !found && r + 1 < n; ++tries) {
					++r;
					if (load_tri(triangles, r, d, t) != kVxOk) continue;
					box = SOLID ? solid_tiles(t, d) : surface_cells(t, d);
					found = box.items() != 0;
				}
				j = 0;
			}
			if (!found) {
				uint64_t begin;
				r = item_triangle(item, local, block_off, n, nblocks, &begin);
				(void)load_tri(triangles, r, d, t);
				box = SOLID ? solid_tiles(t, d) : surface_cells(t, d);
				j = static_cast<uint32_t>(item - begin);
			}
			cnt = static_cast<uint32_t>(box.items());
		}
		const uint32_t q = j / box.nc[0];
		const int cx = box.c0[0] + static_cast<int>(j - q * box.nc[0]);
		const int cy = box.c0[1] + static_cast<int>(q % box.nc[1]), cz = box.c0[2] + static_cast<int>(q / box.nc[1]);
		const int y = 8 * cy + static_cast<int>(lane & 7), z = 8 * cz + static_cast<int>(lane >> 3);
		if (y >= d.extent[1] || z >= d.extent[2]) continue; // (a lane's own rows: nothing below is shared between lanes)
		const size_t row = (static_cast<size_t>(z) * static_cast<size_t>(d.extent[1]) + static_cast<size_t>(y)) * d.words;
		if (SOLID) {
			int k;
			if (vx_solid_crossing(t, y, z, d.extent[0], &k)) atomicXor(plane + row + (k >> 5), 1u << (k & 31));
		} else {
			if (!vx_plane_meets(t, 8 * cx, 8 * cy, 8 * cz, 8)) continue; // the same for every lane of the wave
			const uint32_t m = vx_surface_row8(t, 8 * cx, y, z);
			if (m) atomicOr(plane + row + (cx >> 2), m << (8 * (cx & 3)));
		}
	}
}

// one wave per row (y, z), four rows per workgroup.  marked / crossings: the planes (null: the mode does not ask for it)
__global__ __launch_bounds__(kThreads) void voxelize_dense(const uint32_t* __restrict__ marked, const uint32_t* __restrict__ crossings, uint8_t* __restrict__ volume,
														   unsigned long long* __restrict__ open_columns, const VoxelizeDims d) {
	__shared__ uint32_t s_bits[4][kRowWordsMax + 3];
	const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const uint64_t rows = static_cast<uint64_t>(d.extent[1]) * static_cast<uint64_t>(d.extent[2]);
	const uint64_t r = static_cast<uint64_t>(blockIdx.x) * 4 + wv;
	const bool active = r < rows;
	const uint32_t words = d.words;
	uint32_t* bits = s_bits[wv];
	if (active) {
		uint32_t carry = 0; // 1 while the crossings before this round's words are odd
		for (uint32_t w0 = 0; w0 < words; w0 += 64) {
			const uint32_t w = w0 + lane;
			const bool has = w < words;
			uint32_t inside = 0;
			if (crossings) {
				const uint32_t p = vx_prefix_xor(has ? ld32(crossings, r * words + w) : 0u);
				const uint64_t odd = __ballot(p >> 31);
				const uint32_t before = (static_cast<uint32_t>(__popcll(odd & ((uint64_t{1} << lane) - 1))) & 1u) ^ carry;
				inside = p ^ (before ? 0xFFFFFFFFu : 0u);
				carry ^= static_cast<uint32_t>(__popcll(odd)) & 1u;
			}
			if (has) bits[w] = inside | (marked ? ld32(marked, r * words + w) : 0u);
		}
		if (lane == 0) {
			bits[words] = 0; // (the upper half of the last 64-bit window)
			if (carry && open_columns) atomicAdd(open_columns, 1ull);
		}
	}
	__syncthreads();
	if (!active) return;
	const int nx = d.extent[0];
	const uint32_t y = static_cast<uint32_t>(r % static_cast<uint32_t>(d.extent[1])), z = static_cast<uint32_t>(r / static_cast<uint32_t>(d.extent[1]));
	const int64_t at = static_cast<int64_t>(z) * d.slice_pitch + static_cast<int64_t>(y) * d.row_pitch; // the row's first byte
	const int64_t lead = static_cast<int64_t>((reinterpret_cast<uintptr_t>(volume) + static_cast<uintptr_t>(at)) & 15u); // bytes of its first 16-byte line before it
	const int chunks = static_cast<int>((lead + nx + 15) >> 4);
	for (int c = static_cast<int>(lane); c < chunks; c += 64) {
		const int x0 = 16 * c - static_cast<int>(lead); // the voxel of the chunk's first byte
		if (x0 >= 0 && x0 + 16 <= nx) {
			const uint32_t w = static_cast<uint32_t>(x0) >> 5, s = static_cast<uint32_t>(x0) & 31u;
			const uint32_t b16 = static_cast<uint32_t>((static_cast<uint64_t>(bits[w]) | static_cast<uint64_t>(bits[w + 1]) << 32) >> s) & 0xFFFFu;
			u32x4 v;
			v.x = ((b16 & 15u) * 0x00204081u) & 0x01010101u; // bit i of four -> byte i
			v.y = (((b16 >> 4) & 15u) * 0x00204081u) & 0x01010101u;
			v.z = (((b16 >> 8) & 15u) * 0x00204081u) & 0x01010101u;
			v.w = (((b16 >> 12) & 15u) * 0x00204081u) & 0x01010101u;
			if (d.keep) {
				const u32x4 old = ld128(volume, at + x0);
				v.x |= old.x; v.y |= old.y; v.z |= old.z; v.w |= old.w;
			}
			st128(volume, at + x0, v);
		} else {
			for (int b = 0; b < 16; ++b) {
				const int x = x0 + b;
				if (x < 0 || x >= nx) continue;
				uint32_t v = (bits[static_cast<uint32_t>(x) >> 5] >> (static_cast<uint32_t>(x) & 31u)) & 1u;
				if (d.keep) v |= ld8(volume, static_cast<size_t>(at + x));
				st8(volume, static_cast<size_t>(at + x), v);
			}
		}
	}
}

// ---- host-callable launchers (kernels.h)
void launch_offsets_scan(uint64_t* block_off, uint32_t nblocks, uint32_t groups, hipStream_t stream) {
	hipLaunchKernelGGL(voxelize_scan, dim3(groups), dim3(kThreads), 0, stream, block_off, nblocks);
}

size_t voxelize_plane_bytes(const VoxelizeDims& d) {
	const size_t bytes = static_cast<size_t>(d.extent[1]) * static_cast<size_t>(d.extent[2]) * d.words * sizeof(uint32_t);
	return (bytes + 15) & ~static_cast<size_t>(15);
}

size_t voxelize_workspace_bytes(const VoxelizeDims& d, uint32_t n) {
	const size_t nblocks = (static_cast<size_t>(n) + 255) / 256;
	return 2 * voxelize_plane_bytes(d) + (2 * static_cast<size_t>(n) + 2 * (nblocks + 1)) * sizeof(uint64_t);
}

int voxelize_blocks_per_cu(bool solid) { return solid ? resident_blocks_per_cu(voxelize_items<true>) : resident_blocks_per_cu(voxelize_items<false>); }

void launch_voxelize(const VoxelizeDims& d, const float* triangles, uint32_t n, uint8_t* volume, void* result, void* workspace, const int resident_blocks[2],
					 hipStream_t stream, hipEvent_t* marks) {
	int mark = 0;
	auto stamp = [&]() { if (marks) (void)hipEventRecord(marks[mark++], stream); };
	const size_t plane = voxelize_plane_bytes(d);
	const uint32_t nblocks = (n + 255) / 256;
	uint32_t* marked = static_cast<uint32_t*>(workspace);
	uint32_t* crossings = marked + plane / sizeof(uint32_t);
	uint64_t* local = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(workspace) + 2 * plane);
	uint64_t* block_off = local + 2 * static_cast<size_t>(n);
	const bool surface = (d.mode & kVxSurface) != 0, solid = (d.mode & kVxSolid) != 0;
	stamp();
	(void)hipMemsetAsync(workspace, 0, 2 * plane, stream);
	if (result) (void)hipMemsetAsync(result, 0, 16, stream);
	stamp();
	if (n > 0) {
		hipLaunchKernelGGL(voxelize_plan, dim3(nblocks), dim3(kThreads), 0, stream, triangles, local, block_off, static_cast<uint32_t*>(result), n, nblocks, d);
		launch_offsets_scan(block_off, nblocks, 2, stream);
	}
	stamp();
	if (n > 0 && surface)
		hipLaunchKernelGGL(voxelize_items<false>, dim3(static_cast<unsigned>(resident_blocks[0])), dim3(kThreads), 0, stream, triangles, local, block_off, marked, n, nblocks, d);
	stamp();
	if (n > 0 && solid)
		hipLaunchKernelGGL(voxelize_items<true>, dim3(static_cast<unsigned>(resident_blocks[1])), dim3(kThreads), 0, stream, triangles, local + n,
						   block_off + (nblocks + 1), crossings, n, nblocks, d);
	stamp();
	const uint64_t rows = static_cast<uint64_t>(d.extent[1]) * static_cast<uint64_t>(d.extent[2]);
	unsigned long long* open_columns = result ? reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(result) + 8) : nullptr;
	hipLaunchKernelGGL(voxelize_dense, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(kThreads), 0, stream, surface ? marked : nullptr, solid ? crossings : nullptr, volume,
					   open_columns, d);
	stamp();
}

} // namespace bm
