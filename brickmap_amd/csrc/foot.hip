// foot.hip -- ground navigation on the device (bm_foot_room, bm_foot_field, bm_foot_paths), by the rules of foot.h.
//
//   room   : one lane per column (x, y), x fastest across the lanes: a wave walks 64 consecutive columns downwards, the loads of
//            kFootSlices slices in flight per wait, with the running count of free voxels, and stores one byte per voxel.  A voxel's byte
//            needs the voxel below it, so it is stored one step later.  The only kernel that reads the caller's byte volume.
//   setup  : fills the field with kFootNone and counts the stands from the room bytes, one add per wave.
//   seed   : one lane per seed.  An accepted seed takes 0 by an atomic min; the lane to which the atomic returns kFootNone appends it to
//            the queue as level 0.  The rejected seeds are counted, one add per wave.
//   level  : a round.  Round k reads level k - 1, a segment of the queue whose bounds lie in the tail, and a capped grid of waves strides
//            over it, sixteen nodes per wave: one lane handles one pair (node, direction).  It loads the room bytes of the up + down + 1
//            heights of the neighbouring column, kFootHeights per wait, tests stand and move from the bytes alone, and touches the field
//            only at a legal target, with an atomic min of k.  The returned value says who came first: kFootNone means this lane appends
//            the target, by a ballot and one add per wave on the count of level k.  No plain read of the field decides anything.
//   finish : the largest value and the lowest index that holds it, as the maximum of a key over the queue; then one thread turns the
//            tail into the record.  paths: one lane per start walks down the field (foot_walk).
//
// Between workgroups.  Every store to the field is an atomic min of the round's number at a voxel that held kFootNone or, from another
// lane of the same round, the same number: a value never changes once it is finite, and it does not matter which lane wins.  What a
// round reads with plain loads -- the room bytes, the front's entries, its bounds -- was written by earlier kernels, so the stream's order
// makes it visible.  Entries appended in round k are read in round k + 1.  Nothing waits for another workgroup: no spin, no flag poll,
// no grid barrier, no LDS.  Every loop is bounded by an extent, a front's length, up + down + 1, W(start) or the capacity.  The atomics:
// the min on W (seed, level), the counts of the levels (seed, level), the stands (setup), the rejected seeds (seed) and the key (finish);
// the tail is zeroed by launch_foot_setup on the stream.  Stores into the queue are compared with its size whatever the tail held.
#include <hip/hip_runtime.h>

#include "foot.h"
#include "global_mem.h"
#include "kernels.h"

namespace bm {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kStreamBlocks = 2048; // the grid of setup, seed and finish at most: eight workgroups for each of 256 compute units

typedef __attribute__((address_space(1))) unsigned long long g_ull;

__device__ __forceinline__ uint32_t word_add(uint32_t* words, uint32_t i, uint32_t v) {
	return __hip_atomic_fetch_add((g_u32*)words + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t field_min(uint32_t* field, uint32_t i, uint32_t v) {
	return __hip_atomic_fetch_min((g_u32*)field + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) v += static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), s, 64));
	return v;
}

// The lanes with `take` append their `index` behind `first` under the count word `word`: one add per wave.  (Called by whole waves.)
__device__ __forceinline__ void append(uint32_t* queue, uint32_t* tail, uint32_t word, uint32_t first, uint32_t size, bool take, uint32_t index) {
	const uint64_t takers = __ballot(take);
	if (takers == 0) return;
	const uint32_t lane = threadIdx.x & 63u, leader = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(takers))) - 1u;
	uint32_t base = 0;
	if (lane == leader) base = word_add(tail, word, static_cast<uint32_t>(__popcll(takers)));
	base = static_cast<uint32_t>(__shfl(static_cast<int>(base), static_cast<int>(leader), 64));
	const uint32_t slot = first + base + static_cast<uint32_t>(__popcll(takers & ((uint64_t{1} << lane) - 1u)));
	if (take && slot < size) st32(queue, slot, index);
}

// the bounds of level `level` as the tail holds them, kept inside the queue whatever the tail held
struct Segment {
	uint32_t begin, count;
};
__device__ __forceinline__ Segment segment_of(const uint32_t* tail, uint32_t level, uint32_t size) {
	const uint32_t b = ld32(tail, kFootTailBeginWord + level % 3u), c = ld32(tail, kFootTailCountWord + level % 3u);
	const uint32_t begin = b < size ? b : size;
	return {begin, c < size - begin ? c : size - begin};
}

} // namespace

__global__ __launch_bounds__(kThreads) void foot_room(const uint8_t* __restrict__ volume, uint8_t* __restrict__ room, const FootDims d) {
	const uint32_t col = blockIdx.x * kThreads + threadIdx.x;
	if (col >= d.columns) return;
	const uint32_t nx = static_cast<uint32_t>(d.extent[0]), y = col / nx, x = col - y * nx;
	const int32_t nz = d.extent[2];
	const int64_t at = static_cast<int64_t>(y) * d.row_pitch + x;
	uint32_t run = kFootRoomCap; // of the voxel above: everything above the volume is free
	for (int32_t z0 = nz - 1; z0 >= 0; z0 -= kFootSlices) {
		uint32_t v[kFootSlices];
#pragma unroll
		for (int i = 0; i < kFootSlices; ++i) v[i] = z0 - i >= 0 ? ld8(volume, static_cast<size_t>(static_cast<int64_t>(z0 - i) * d.slice_pitch + at)) : 0u;
#pragma unroll
		for (int i = 0; i < kFootSlices; ++i) {
			const int32_t z = z0 - i;
			if (z < 0) continue;
			const bool blocked = v[i] != 0;
			if (z + 1 < nz) st8(room, static_cast<size_t>(z + 1) * d.columns + col, foot_room_byte(run, blocked));
			run = foot_room_run(run, blocked);
		}
	}
	st8(room, col, foot_room_byte(run, d.floor != 0));
}

__global__ __launch_bounds__(kThreads) void foot_setup(const uint8_t* __restrict__ room, uint32_t* __restrict__ field, uint32_t* tail, const FootDims d) {
	uint32_t stands = 0;
	for (uint32_t base = blockIdx.x * kThreads; base < d.voxels; base += gridDim.x * kThreads) {
		const uint32_t i = base + threadIdx.x;
		if (i < d.voxels) {
			st32(field, i, kFootNone);
			stands += foot_stand(ld8(room, i), d.height) ? 1u : 0u;
		}
	}
	stands = wave_sum(stands);
	if ((threadIdx.x & 63u) == 0 && stands != 0) word_add(tail, kFootTailStandableWord, stands);
}

__global__ __launch_bounds__(kThreads) void foot_seed(const uint8_t* __restrict__ room, const int32_t* __restrict__ seeds, const uint32_t n, uint32_t* field,
													   uint32_t* __restrict__ queue, uint32_t* tail, const FootDims d) {
	uint32_t rejected = 0; // (ballots: the same in every lane)
	for (uint32_t base = blockIdx.x * kThreads; base < n; base += gridDim.x * kThreads) {
		const uint32_t s = base + threadIdx.x;
		const bool live = s < n;
		bool ok = false, first = false;
		uint32_t index = 0;
		if (live) {
			const int32_t x = ldi32(seeds, 3 * static_cast<size_t>(s)), y = ldi32(seeds, 3 * static_cast<size_t>(s) + 1), z = ldi32(seeds, 3 * static_cast<size_t>(s) + 2);
			if (x >= 0 && y >= 0 && z >= 0 && x < d.extent[0] && y < d.extent[1] && z < d.extent[2]) {
				index = foot_voxel_index(d, x, y, z);
				if (foot_stand(ld8(room, index), d.height)) {
					ok = true;
					first = field_min(field, index, 0u) == kFootNone;
				}
			}
		}
		append(queue, tail, kFootTailCountWord, 0u, d.queue, first, index);
		rejected += static_cast<uint32_t>(__popcll(__ballot(live && !ok)));
	}
	if ((threadIdx.x & 63u) == 0 && rejected != 0) word_add(tail, kFootTailRejectedWord, rejected);
}

// round `round` (1, 2, ...): the stands of level round - 1 give their legal targets the value `round`
__global__ __launch_bounds__(kThreads) void foot_level(const uint8_t* __restrict__ room, uint32_t* field, uint32_t* queue, uint32_t* tail, const uint32_t round, const FootDims d) {
	const Segment front = segment_of(tail, round + 2u, d.queue); // level round - 1
	const uint32_t behind = front.begin + front.count, word = kFootTailCountWord + round % 3u;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		st32(tail, kFootTailBeginWord + round % 3u, behind);          // read by the next round
		st32(tail, kFootTailCountWord + (round + 1u) % 3u, 0u);        // read by the round before, appended under by the next one
	}
	if (front.count == 0 || round > d.limit) return;
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (kThreads / 64);
	const int dir = static_cast<int>(lane & 3u);
	const int32_t nx = d.extent[0], ny = d.extent[1], nz = d.extent[2], heights = d.up + d.down + 1;
	for (uint32_t node0 = (blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * 16u; node0 < front.count; node0 += waves * 16u) {
		const uint32_t node = node0 + (lane >> 2);
		bool live = node < front.count;
		uint32_t p = live ? ld32(queue, front.begin + node) : 0u;
		live = live && p < d.voxels; // (always: the queue holds voxels)
		p = live ? p : 0u;
		const int32_t z = static_cast<int32_t>(p / d.columns), c = static_cast<int32_t>(p - static_cast<uint32_t>(z) * d.columns), y = c / nx, x = c - y * nx;
		const int32_t qx = x + foot_dir_x(dir), qy = y + foot_dir_y(dir);
		live = live && qx >= 0 && qy >= 0 && qx < nx && qy < ny;
		const uint32_t rp = live ? ld8(room, p) : 0u;
		const uint32_t qcol = live ? static_cast<uint32_t>(qy) * static_cast<uint32_t>(nx) + static_cast<uint32_t>(qx) : 0u;
		for (int32_t j0 = 0; j0 < heights; j0 += kFootHeights) { // (the same trips in every lane: the ballots below meet whole waves)
			uint32_t r[kFootHeights];
#pragma unroll
			for (int i = 0; i < kFootHeights; ++i) {
				const int32_t dz = j0 + i - d.down, qz = z + dz;
				r[i] = live && dz <= d.up && qz >= 0 && qz < nz ? ld8(room, static_cast<size_t>(qz) * d.columns + qcol) : 0u; // 0: blocked, no stand
			}
#pragma unroll
			for (int i = 0; i < kFootHeights; ++i) {
				const int32_t dz = j0 + i - d.down;
				const uint32_t q = static_cast<uint32_t>(z + dz) * d.columns + qcol;
				bool first = false;
				if (foot_move(rp, r[i], dz, d.height)) first = field_min(field, q, round) == kFootNone;
				append(queue, tail, word, behind, d.queue, first, q);
			}
		}
	}
}

// `done` rounds have run: the key of the largest value over everything the queue holds
__global__ __launch_bounds__(kThreads) void foot_finish(const uint32_t* __restrict__ field, const uint32_t* __restrict__ queue, unsigned long long* tail, const uint32_t done,
														 const FootDims d) {
	const Segment last = segment_of(reinterpret_cast<const uint32_t*>(tail), done, d.queue);
	const uint32_t n = last.begin + last.count;
	uint64_t best = 0;
	for (uint32_t base = blockIdx.x * kThreads; base < n; base += gridDim.x * kThreads) {
		const uint32_t i = base + threadIdx.x;
		if (i < n) {
			const uint32_t q = ld32(queue, i);
			const uint64_t k = q < d.voxels ? foot_max_key(ld32(field, q), q) : 0u;
			best = k > best ? k : best;
		}
	}
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) {
		const uint64_t other = static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(best), s, 64));
		best = other > best ? other : best;
	}
	if ((threadIdx.x & 63u) == 0 && best != 0) __hip_atomic_fetch_max((g_ull*)tail, static_cast<unsigned long long>(best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the tail -> the 32 bytes of the result
__global__ __launch_bounds__(64) void foot_record_out(const uint64_t* __restrict__ tail, uint64_t* __restrict__ result, const uint32_t done, const uint32_t size) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const uint32_t* words = reinterpret_cast<const uint32_t*>(tail);
	const Segment last = segment_of(words, done, size);
	const FootRecord rec = foot_record(ld64(tail, 0), last.begin + last.count, ld32(words, kFootTailRejectedWord), ld32(words, kFootTailStandableWord));
	st64(result, 0, rec.reached);
	st64(result, 1, static_cast<uint64_t>(rec.farthest) | static_cast<uint64_t>(rec.seeds_rejected) << 32);
	st64(result, 2, rec.farthest_at);
	st64(result, 3, rec.standable);
}

__global__ __launch_bounds__(kThreads) void foot_paths(const uint8_t* __restrict__ room, const uint32_t* __restrict__ field, const int32_t* __restrict__ starts, const uint32_t n,
														const int32_t capacity, int32_t* __restrict__ path, int32_t* __restrict__ lengths, const FootDims d) {
	const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
	if (q >= n) return;
	g_i32* out = (g_i32*)path + static_cast<size_t>(q) * static_cast<size_t>(capacity) * 3;
	const int32_t length = foot_walk(
		d, ldi32(starts, 3 * static_cast<size_t>(q)), ldi32(starts, 3 * static_cast<size_t>(q) + 1), ldi32(starts, 3 * static_cast<size_t>(q) + 2), capacity,
		[&](uint32_t i) { return ld32(field, i); }, [&](uint32_t i) { return ld8(room, i); },
		[&](int32_t k, int32_t x, int32_t y, int32_t z) {
			out[3 * static_cast<size_t>(k)] = x;
			out[3 * static_cast<size_t>(k) + 1] = y;
			out[3 * static_cast<size_t>(k) + 2] = z;
		});
	((g_i32*)lengths)[q] = length;
}

// ---- host-callable launchers (kernels.h)
namespace {
unsigned blocks_for(uint64_t items, uint64_t per_block, uint64_t most) {
	const uint64_t b = (items + per_block - 1) / per_block;
	return static_cast<unsigned>(b < most ? (b ? b : 1) : most);
}
uint32_t* foot_tail(const FootDims& d, void* workspace) { return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(workspace) + foot_tail_offset(d)); }
} // namespace

void launch_foot_room(const FootDims& d, const uint8_t* volume, uint8_t* room, hipStream_t stream) {
	hipLaunchKernelGGL(foot_room, dim3((d.columns + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, volume, room, d); // at most 2^20 blocks: 16384^2 columns
}

void launch_foot_setup(const FootDims& d, const uint8_t* room, const int32_t* seeds, uint32_t n, uint32_t* field, void* workspace, hipStream_t stream) {
	uint32_t* tail = foot_tail(d, workspace);
	(void)hipMemsetAsync(tail, 0, kFootTailBytes, stream); // every byte an atomic of this call lives in, but the field's
	hipLaunchKernelGGL(foot_setup, dim3(blocks_for(d.voxels, kThreads, kStreamBlocks)), dim3(kThreads), 0, stream, room, field, tail, d);
	if (n > 0) hipLaunchKernelGGL(foot_seed, dim3(blocks_for(n, kThreads, kStreamBlocks)), dim3(kThreads), 0, stream, room, seeds, n, field, static_cast<uint32_t*>(workspace), tail, d);
}

void launch_foot_rounds(const FootDims& d, const uint8_t* room, uint32_t* field, void* workspace, uint32_t first_round, uint32_t rounds, hipStream_t stream) {
	const unsigned blocks = blocks_for(d.queue, (kThreads / 64) * 16, kFootMaxWaves / (kThreads / 64));
	for (uint32_t k = first_round; k < first_round + rounds; ++k)
		hipLaunchKernelGGL(foot_level, dim3(blocks), dim3(kThreads), 0, stream, room, field, static_cast<uint32_t*>(workspace), foot_tail(d, workspace), k, d);
}

void launch_foot_finish(const FootDims& d, const uint32_t* field, void* result, void* workspace, uint32_t done, hipStream_t stream) {
	unsigned long long* tail = reinterpret_cast<unsigned long long*>(foot_tail(d, workspace));
	hipLaunchKernelGGL(foot_finish, dim3(blocks_for(d.queue, kThreads, kStreamBlocks)), dim3(kThreads), 0, stream, field, static_cast<const uint32_t*>(workspace), tail, done, d);
	hipLaunchKernelGGL(foot_record_out, dim3(1), dim3(64), 0, stream, reinterpret_cast<const uint64_t*>(tail), static_cast<uint64_t*>(result), done, d.queue);
}

void launch_foot_paths(const FootDims& d, const uint8_t* room, const uint32_t* field, const int32_t* starts, uint32_t n, int32_t capacity, int32_t* path, int32_t* lengths,
					   hipStream_t stream) {
	hipLaunchKernelGGL(foot_paths, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, room, field, starts, n, capacity, path, lengths, d);
}

} // namespace bm
