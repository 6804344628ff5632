// label.hip -- connected components of a box of the live scene (bm_scene_label_region, bm_scene_label_components, bm_scene_label_mask;
// scene.cpp "connected components").  The caller's label volume L[z][y][x] (tight, int32) is the only per-voxel memory: it is the parent
// array of a union-find forest while the call runs (label.h has the rules) and holds 1 + index(first voxel of the component) at its end.
//
//   local   : one wave per brick cell of the clipped box, one x-row of 8 voxels per lane.  The index word and -- when it is loaded --
//             the brick at arena[pool_base + slot] (or a listed brick: the cells a streaming scene does not hold), masked with the box's
//             cover, is labelled in registers: every row takes the minimum over the overlapping voxels of its four neighbouring rows
//             (lane shuffles) and spreads it along its runs, until a wave ballot says nothing changed.  The brick's (z, y, x) order is
//             the box's, so the smallest brick-local index is the smallest box index: 8 words per lane are stored, 0 for empty voxels.
//   merge   : one wave per brick cell, its three lower faces inside the box in turn, one lane per voxel pair across the face; a pair
//             with both sides solid is joined (label_union)
//   flatten : every solid voxel takes its root's label; the roots (label == index + 1) are counted and added to *count
//   components : roots per 1024 voxels -> exclusive scan -> records of the first `capacity` roots in index order, which is ascending
//             label; then every voxel finds its record by binary search and is added to it with integer atomics -- reduced over the wave
//             and the workgroup first where they share a record; then max -> max + 1
//   mask    : the same search, then chosen[slot] as one byte
//
// Between workgroups of merge.  The L2s of the eight XCDs are not coherent with each other and a CU's L1 is never refreshed by another
// CU's stores, so inside merge every read of a word is a relaxed agent-scope atomic load and every write is an atomic minimum.  No
// fence is needed: the algorithm is correct with values read late (label.h), the link itself is decided by what the atomic returns,
// and between kernels the stream's order makes everything visible.  Nothing here waits for another workgroup: no spin, no flag, no
// persistent hand-off.  Every loop is bounded by construction; the bounds stand next to the loops (label.h).
#include <hip/hip_runtime.h>

#include <climits>

#include "global_mem.h"
#include "kernels.h"
#include "label.h"

namespace bm {
namespace {

constexpr int kRecordWords = 10;           // bm_component
constexpr uint32_t kVoxelsPerBlock = 1024; // of flatten and the component kernels: 4 per thread

// the words of the label volume as merge and flatten see them
struct DeviceWords {
	g_u32* p;
	__device__ __forceinline__ uint32_t load(uint32_t i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	__device__ __forceinline__ uint32_t fetch_min(uint32_t i, uint32_t v) { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

__device__ __forceinline__ uint32_t bit_range(int a, int b) { return ((1u << b) - 1u) & ~((1u << a) - 1u); } // bits [a, b), 0 <= a <= b <= 8

// the wave's cell: PATCH = entry `id` of the list, else cell `id` of the clipped box, x fastest
template <bool PATCH>
__device__ __forceinline__ void cell_of(const LabelDims& d, const int* __restrict__ cells, uint32_t id, int c[3]) {
	if (PATCH) {
		c[0] = ldi32(cells, 3 * static_cast<size_t>(id));
		c[1] = ldi32(cells, 3 * static_cast<size_t>(id) + 1);
		c[2] = ldi32(cells, 3 * static_cast<size_t>(id) + 2);
	} else {
		const uint32_t q = id / static_cast<uint32_t>(d.nc[0]);
		c[0] = d.c0[0] + static_cast<int>(id - q * static_cast<uint32_t>(d.nc[0]));
		c[1] = d.c0[1] + static_cast<int>(q % static_cast<uint32_t>(d.nc[1]));
		c[2] = d.c0[2] + static_cast<int>(q / static_cast<uint32_t>(d.nc[1]));
	}
}

// index in the box of world voxel (x, y, z) of the clipped box
__device__ __forceinline__ uint32_t box_index(const LabelDims& d, int x, int y, int z) {
	return label_index(static_cast<uint32_t>(x - d.org[0]), static_cast<uint32_t>(y - d.org[1]), static_cast<uint32_t>(z - d.org[2]), d.nx, d.ny);
}

template <bool PATCH>
__global__ __launch_bounds__(256) void label_local(uint32_t* __restrict__ labels, const uint32_t* __restrict__ index_grid, const uint32_t* __restrict__ pool_base,
												   const uint32_t* __restrict__ arena, const int* __restrict__ cells, const uint32_t* __restrict__ bricks, const uint32_t count,
												   const LabelDims d) {
	const uint32_t id = blockIdx.x * 4 + (threadIdx.x >> 6), r = threadIdx.x & 63;
	if (id >= count) return; // (the whole wave)
	int c[3];
	cell_of<PATCH>(d, cells, id, c);
	uint32_t word = 0;
	if (PATCH) {
		word = ld32(bricks, static_cast<size_t>(id) * 16 + (r >> 2));
	} else {
		const uint32_t sc = supercell_of(static_cast<int>(d.sg_xy), static_cast<int>(d.sg_xy2), c[0], c[1], c[2]);
		const uint32_t iw = ld32(index_grid, static_cast<size_t>(sc) * 4096 + cell_local_index(c[0], c[1], c[2]));
		if (iw & kLoadedBit) word = ld32(arena, brick_first_word(ld32(pool_base, sc), iw) + (r >> 2));
	}
	// the box's cover of the lane's row
	const int y = c[1] * 8 + static_cast<int>(r & 7), z = c[2] * 8 + static_cast<int>(r >> 3);
	const bool row_in = y >= d.lo[1] && y < d.hi[1] && z >= d.lo[2] && z < d.hi[2];
	const int x0 = d.lo[0] - 8 * c[0] > 0 ? d.lo[0] - 8 * c[0] : 0, x1 = d.hi[0] - 8 * c[0] < 8 ? d.hi[0] - 8 * c[0] : 8;
	const uint32_t cover = row_in && x0 < x1 ? bit_range(x0, x1) : 0u;
	const uint32_t bits = (word >> (8 * (r & 3))) & cover;

	LabelRow row = label_row_init(bits, r);
	if (__ballot(bits != 0) != 0) {
		// the neighbouring rows: y - 1, y + 1, z - 1, z + 1 inside the brick
		const int src[4] = {static_cast<int>(r) - 1, static_cast<int>(r) + 1, static_cast<int>(r) - 8, static_cast<int>(r) + 8};
		const bool have[4] = {(r & 7) != 0, (r & 7) != 7, (r >> 3) != 0, (r >> 3) != 7};
#pragma unroll 1
		for (int round = 0; round < kLabelBrickRounds; ++round) { // bounded (label.h); ends as soon as no lane's row changed
			LabelRow near = {{kLabelRowEmpty, kLabelRowEmpty, kLabelRowEmpty, kLabelRowEmpty}};
#pragma unroll
			for (int n = 0; n < 4; ++n)
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					const uint32_t v = __shfl(row.w[k], src[n] & 63, 64);
					near.w[k] = label_min16x2(near.w[k], have[n] ? v : kLabelRowEmpty);
				}
			const bool changed = label_row_settle(row, bits, near);
			if (__ballot(changed) == 0) break;
		}
	}
#pragma unroll
	for (int x = 0; x < 8; ++x) {
		if (!((cover >> x) & 1u)) continue;
		const uint32_t l = label_row_get(row, x);
		const uint32_t v = l == 0xFFFFu ? 0u : 1u + box_index(d, c[0] * 8 + static_cast<int>(l & 7), c[1] * 8 + static_cast<int>((l >> 3) & 7), c[2] * 8 + static_cast<int>(l >> 6));
		st32(labels, box_index(d, c[0] * 8 + x, y, z), v);
	}
}

__global__ __launch_bounds__(256) void label_merge(uint32_t* labels, const uint32_t count, const LabelDims d) {
	const uint32_t id = blockIdx.x * 4 + (threadIdx.x >> 6), r = threadIdx.x & 63;
	if (id >= count) return;
	int c[3];
	cell_of<false>(d, nullptr, id, c);
	DeviceWords w{(g_u32*)labels};
	const uint32_t step[3] = {1u, d.nx, d.nx * d.ny};
#pragma unroll
	for (int f = 0; f < 3; ++f) {
		if (c[f] * 8 <= d.lo[f]) continue; // the voxels below this face lie outside the box
		// the lane's voxel on the cell's low face of axis f: the other two axes take r & 7 and r >> 3, in (x, y, z) order
		int v[3];
		v[f] = c[f] * 8;
		v[f == 0 ? 1 : 0] = c[f == 0 ? 1 : 0] * 8 + static_cast<int>(r & 7);
		v[f == 2 ? 1 : 2] = c[f == 2 ? 1 : 2] * 8 + static_cast<int>(r >> 3);
		const bool inside = v[0] >= d.lo[0] && v[0] < d.hi[0] && v[1] >= d.lo[1] && v[1] < d.hi[1] && v[2] >= d.lo[2] && v[2] < d.hi[2];
		const uint32_t a = inside ? box_index(d, v[0], v[1], v[2]) : 0u, b = inside ? a - step[f] : 0u;
		const uint32_t wa = inside ? w.load(a) : 0u, wb = inside ? w.load(b) : 0u;
		// A lane whose pair hangs under the same two parents as the pair of the lane before it leaves the join to that lane (and that one
		// to the one before it ...): the first lane of such a run joins the two trees, which are these lanes' trees as well.  On a flat
		// face of a large solid that is one union per face instead of 64 on one root.
		const uint32_t pa = __shfl_up(wa, 1, 64), pb = __shfl_up(wb, 1, 64);
		const bool left_to_neighbour = r != 0 && pa == wa && pb == wb;
		if (wa != 0 && wb != 0 && !left_to_neighbour) label_union(w, a, b); // bounded (label.h)
	}
}

// sum of one value per thread over a 256-thread workgroup, in every thread
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* lds4) {
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
	if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
	__syncthreads();
	return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

__global__ __launch_bounds__(256) void label_flatten(uint32_t* labels, const uint32_t n, unsigned long long* __restrict__ count) {
	__shared__ uint32_t lds4[4];
	DeviceWords w{(g_u32*)labels};
	uint32_t roots = 0;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const uint32_t i = blockIdx.x * kVoxelsPerBlock + 256 * k + threadIdx.x;
		if (i >= n) continue;
		const uint32_t word = w.load(i);
		if (word == 0) continue;
		if (word == i + 1) { ++roots; continue; }
		// another thread may have flattened a word of the chain already: it then names the root, still an ancestor.  Bounded as label_find.
		const uint32_t root = label_find(w, word - 1);
		__hip_atomic_store(w.p + i, root + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	const uint32_t total = block_sum(roots, lds4);
	if (threadIdx.x == 0 && total != 0) atomicAdd(count, static_cast<unsigned long long>(total));
}

// ---- components
// a thread's four consecutive voxels: which of them are roots
__device__ __forceinline__ uint32_t thread_roots(const uint32_t* __restrict__ labels, uint32_t n, uint32_t first) {
	uint32_t m = 0;
#pragma unroll
	for (uint32_t k = 0; k < 4; ++k)
		if (first + k < n && ld32(labels, first + k) == first + k + 1) m |= 1u << k;
	return m;
}

__global__ __launch_bounds__(256) void label_roots_count(const uint32_t* __restrict__ labels, const uint32_t n, uint64_t* __restrict__ block_off) {
	__shared__ uint32_t lds4[4];
	const uint32_t total = block_sum(__popc(thread_roots(labels, n, blockIdx.x * kVoxelsPerBlock + 4 * threadIdx.x)), lds4);
	if (threadIdx.x == 0) st64(block_off, blockIdx.x, total);
}

// exclusive scan of one value per thread of a 256-thread workgroup; *total = the sum
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* lds, uint64_t* total) {
	const uint32_t t = threadIdx.x;
	lds[t] = v;
	__syncthreads();
	uint64_t sum = v;
#pragma unroll
	for (uint32_t s = 1; s < 256; s <<= 1) {
		const uint64_t other = t >= s ? lds[t - s] : 0;
		__syncthreads();
		sum += other;
		lds[t] = sum;
		__syncthreads();
	}
	*total = lds[255];
	return sum - v;
}

// block_off[0 ... nblocks): sums -> exclusive offsets; block_off[nblocks] = the total (one workgroup, as volume_scan)
__global__ __launch_bounds__(256) void label_scan(uint64_t* __restrict__ block_off, const uint32_t nblocks) {
	__shared__ uint64_t lds[256];
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

// the records of the first `capacity` roots, in index order: label, no faces, no voxels, empty bounds
__global__ __launch_bounds__(256) void label_roots_write(const uint32_t* __restrict__ labels, const uint32_t n, const uint64_t* __restrict__ block_off,
														 uint32_t* __restrict__ comps, const uint64_t capacity) {
	__shared__ uint64_t lds[256];
	const uint32_t first = blockIdx.x * kVoxelsPerBlock + 4 * threadIdx.x;
	const uint32_t m = thread_roots(labels, n, first);
	uint64_t total;
	uint64_t rank = ld64(block_off, blockIdx.x) + block_scan(__popc(m), lds, &total);
#pragma unroll
	for (uint32_t k = 0; k < 4; ++k) {
		if (!((m >> k) & 1u)) continue;
		if (rank < capacity) {
			const size_t at = static_cast<size_t>(rank) * kRecordWords;
			st32(comps, at, first + k + 1);
			st32(comps, at + 1, 0u);
			st32(comps, at + 2, 0u);
			st32(comps, at + 3, 0u);
#pragma unroll
			for (int a = 0; a < 3; ++a) {
				st32(comps, at + 4 + a, static_cast<uint32_t>(INT_MAX));
				st32(comps, at + 7 + a, static_cast<uint32_t>(INT_MIN));
			}
		}
		++rank;
	}
}

// the record among comps[0 ... records) that carries `label`, or -1.  Bounded: the range halves.
__device__ __forceinline__ int64_t find_record(const uint32_t* __restrict__ comps, uint64_t records, uint32_t label) {
	uint64_t a = 0, b = records; // the last record whose label is <= `label`
	if (records == 0) return -1;
	while (b - a > 1) {
		const uint64_t mid = (a + b) >> 1;
		if (ld32(comps, static_cast<size_t>(mid) * kRecordWords) <= label) a = mid; else b = mid;
	}
	return ld32(comps, static_cast<size_t>(a) * kRecordWords) == label ? static_cast<int64_t>(a) : -1;
}

// what a wave (and then a workgroup) has gathered for one record and not yet added to it
struct Pending {
	int64_t slot; // -1: nothing
	uint32_t cnt, faces;
	int mn[3], mx[3];
};
__device__ __forceinline__ void pending_add(uint32_t* comps, const Pending& p) {
	uint32_t* rec = comps + static_cast<size_t>(p.slot) * kRecordWords;
	if (p.faces != 0) atomicOr(rec + 1, p.faces);
	atomicAdd(reinterpret_cast<unsigned long long*>(rec + 2), static_cast<unsigned long long>(p.cnt));
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		atomicMin(reinterpret_cast<int*>(rec) + 4 + a, p.mn[a]);
		atomicMax(reinterpret_cast<int*>(rec) + 7 + a, p.mx[a]); // the last voxel; finish makes it half-open
	}
}
__device__ __forceinline__ void pending_merge(Pending& p, const Pending& q) {
	p.cnt += q.cnt;
	p.faces |= q.faces;
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		p.mn[a] = q.mn[a] < p.mn[a] ? q.mn[a] : p.mn[a];
		p.mx[a] = q.mx[a] > p.mx[a] ? q.mx[a] : p.mx[a];
	}
}

// A workgroup takes kAccumulateRounds * 256 consecutive voxels, 64 consecutive ones per wave and round.  A wave whose voxels that have a
// record all share it reduces them by shuffles and keeps the sum while the next rounds bring the same record; the four waves' sums meet in
// LDS at the end.  So a giant component costs one set of atomics per workgroup, not one per voxel: every one of them lands on the same
// few words.  Waves with several records among their 64 voxels add lane by lane.
constexpr int kAccumulateRounds = 16;
__global__ __launch_bounds__(256) void label_accumulate(const uint32_t* __restrict__ labels, const uint32_t n, const uint64_t* __restrict__ total, uint32_t* comps,
														const uint64_t capacity, const LabelDims d) {
	__shared__ Pending lds[4];
	const uint64_t count = ld64(total, 0), records = count < capacity ? count : capacity;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	Pending kept; // wave-uniform
	kept.slot = -1;
#pragma unroll 1
	for (int k = 0; k < kAccumulateRounds; ++k) {
		const uint64_t i64 = (static_cast<uint64_t>(blockIdx.x) * kAccumulateRounds + k) * 256 + threadIdx.x;
		const uint32_t i = static_cast<uint32_t>(i64 < n ? i64 : n);
		const uint32_t label = i < n ? ld32(labels, i) : 0u;
		Pending mine;
		mine.slot = label != 0 ? find_record(comps, records, label) : -1;
		// the voxel and the faces of (box and world) it lies on
		const uint32_t row = i / d.nx, zz = row / d.ny;
		const int v[3] = {d.org[0] + static_cast<int>(i - row * d.nx), d.org[1] + static_cast<int>(row - zz * d.ny), d.org[2] + static_cast<int>(zz)};
		mine.cnt = mine.slot >= 0 ? 1u : 0u;
		mine.faces = 0;
#pragma unroll
		for (int a = 0; a < 3; ++a) {
			if (mine.slot >= 0) mine.faces |= (v[a] == d.lo[a] ? 1u : 0u) << (2 * a) | (v[a] == d.hi[a] - 1 ? 1u : 0u) << (2 * a + 1);
			mine.mn[a] = mine.slot >= 0 ? v[a] : INT_MAX;
			mine.mx[a] = mine.slot >= 0 ? v[a] : INT_MIN;
		}
		const unsigned long long with = __ballot(mine.slot >= 0);
		if (with == 0) continue; // (the whole wave)
		const int64_t slot0 = __shfl(mine.slot, __builtin_ctzll(with), 64);
		if (__ballot(mine.slot >= 0 && mine.slot != slot0) != 0) { // several records: lane by lane
			if (mine.slot >= 0) pending_add(comps, mine);
			continue;
		}
		// one record: the wave's sum in every lane (lanes without a record hold the neutral values)
#pragma unroll
		for (int s = 1; s < 64; s <<= 1) {
			Pending other;
			other.cnt = __shfl_xor(mine.cnt, s, 64);
			other.faces = __shfl_xor(mine.faces, s, 64);
#pragma unroll
			for (int a = 0; a < 3; ++a) { other.mn[a] = __shfl_xor(mine.mn[a], s, 64); other.mx[a] = __shfl_xor(mine.mx[a], s, 64); }
			pending_merge(mine, other);
		}
		mine.slot = slot0;
		if (kept.slot == slot0) pending_merge(kept, mine);
		else {
			if (kept.slot >= 0 && lane == 0) pending_add(comps, kept);
			kept = mine;
		}
	}
	if (lane == 0) lds[wave] = kept;
	__syncthreads();
	const bool together = lds[0].slot >= 0 && lds[1].slot == lds[0].slot && lds[2].slot == lds[0].slot && lds[3].slot == lds[0].slot;
	if (together) {
		if (threadIdx.x == 0) {
			Pending sum = lds[0];
			pending_merge(sum, lds[1]);
			pending_merge(sum, lds[2]);
			pending_merge(sum, lds[3]);
			pending_add(comps, sum);
		}
	} else if (lane == 0 && kept.slot >= 0) pending_add(comps, kept);
}

__global__ __launch_bounds__(256) void label_finish(const uint64_t* __restrict__ total, uint32_t* __restrict__ comps, const uint64_t capacity) {
	const uint64_t count = ld64(total, 0), records = count < capacity ? count : capacity;
	for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < records; i += static_cast<uint64_t>(gridDim.x) * 256)
#pragma unroll
		for (int a = 0; a < 3; ++a) st32(comps, static_cast<size_t>(i) * kRecordWords + 7 + a, ld32(comps, static_cast<size_t>(i) * kRecordWords + 7 + a) + 1u);
}

__global__ __launch_bounds__(256) void label_mask(const uint32_t* __restrict__ labels, const uint32_t n, const uint32_t* __restrict__ comps, const uint64_t records,
												  const uint8_t* __restrict__ chosen, uint8_t* __restrict__ mask) {
#pragma unroll 1
	for (int k = 0; k < 4; ++k) {
		const uint32_t i = blockIdx.x * kVoxelsPerBlock + 256 * k + threadIdx.x;
		if (i >= n) continue;
		const uint32_t label = ld32(labels, i);
		const int64_t slot = label != 0 ? find_record(comps, records, label) : -1;
		st8(mask, i, slot >= 0 ? ld8(chosen, static_cast<size_t>(slot)) : 0u);
	}
}

unsigned blocks_of(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

} // namespace

void launch_label_region(const DeviceScene& sc, uint32_t* labels, uint64_t* count, const LabelDims& d, const int* patch_cells, const uint32_t* patch_bricks,
						 uint32_t patches, hipStream_t stream, hipEvent_t* marks) {
	const uint32_t cells = static_cast<uint32_t>(d.nc[0]) * static_cast<uint32_t>(d.nc[1]) * static_cast<uint32_t>(d.nc[2]);
	const uint32_t n = d.nx * d.ny * d.nz;
	if (marks) (void)hipEventRecord(marks[0], stream);
	hipLaunchKernelGGL(label_local<false>, dim3(blocks_of(cells, 4)), dim3(256), 0, stream, labels, sc.index_grid, sc.pool_base, sc.brick_arena, nullptr, nullptr, cells, d);
	if (patches) hipLaunchKernelGGL(label_local<true>, dim3(blocks_of(patches, 4)), dim3(256), 0, stream, labels, nullptr, nullptr, nullptr, patch_cells, patch_bricks, patches, d);
	if (marks) (void)hipEventRecord(marks[1], stream);
	hipLaunchKernelGGL(label_merge, dim3(blocks_of(cells, 4)), dim3(256), 0, stream, labels, cells, d);
	if (marks) (void)hipEventRecord(marks[2], stream);
	hipLaunchKernelGGL(label_flatten, dim3(blocks_of(n, kVoxelsPerBlock)), dim3(256), 0, stream, labels, n, reinterpret_cast<unsigned long long*>(count));
	if (marks) (void)hipEventRecord(marks[3], stream);
}

size_t label_tmp_bytes(uint32_t voxels) { return (static_cast<size_t>(blocks_of(voxels, kVoxelsPerBlock)) + 1) * sizeof(uint64_t); }

void launch_label_components(const uint32_t* labels, void* comps, uint64_t capacity, const LabelDims& d, uint64_t* tmp, hipStream_t stream) {
	const uint32_t n = d.nx * d.ny * d.nz, nblocks = blocks_of(n, kVoxelsPerBlock);
	uint32_t* out = static_cast<uint32_t*>(comps);
	hipLaunchKernelGGL(label_roots_count, dim3(nblocks), dim3(256), 0, stream, labels, n, tmp);
	hipLaunchKernelGGL(label_scan, dim3(1), dim3(256), 0, stream, tmp, nblocks);
	if (capacity == 0) return;
	hipLaunchKernelGGL(label_roots_write, dim3(nblocks), dim3(256), 0, stream, labels, n, tmp, out, capacity);
	hipLaunchKernelGGL(label_accumulate, dim3(blocks_of(n, kAccumulateRounds * 256)), dim3(256), 0, stream, labels, n, tmp + nblocks, out, capacity, d);
	const uint64_t most = capacity < n ? capacity : n;
	hipLaunchKernelGGL(label_finish, dim3(static_cast<unsigned>((most + 255) / 256 < 65536 ? (most + 255) / 256 : 65536)), dim3(256), 0, stream, tmp + nblocks, out, capacity);
}

void launch_label_mask(const uint32_t* labels, uint32_t voxels, const void* comps, uint64_t records, const uint8_t* chosen, uint8_t* mask, hipStream_t stream) {
	hipLaunchKernelGGL(label_mask, dim3(blocks_of(voxels, kVoxelsPerBlock)), dim3(256), 0, stream, labels, voxels, static_cast<const uint32_t*>(comps), records, chosen, mask);
}

} // namespace bm
