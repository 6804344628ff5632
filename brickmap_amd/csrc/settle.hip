// settle.hip -- rigid settling of a label volume on the device (bm_settle), by the rules of settle.h.  One lane per column (x, y), x
// fastest across the lanes: a wave walks 64 consecutive columns upwards and reads 256 contiguous bytes of every slice.
//
//   setup  : one lane per record: D[slot] = chosen ? kSettleUnknown : 0; the chosen records are counted, one add per wave.
//   relax  : a round.  A lane walks its column upwards, kSettleSlices slices' loads in flight per wait, and keeps the label, the height
//            and the moving slot of the solid voxel below it (settle_step); it searches the table only where the label changes.  At a
//            contact it takes D[upper] = min(D[upper], D[lower] + g) with an atomic min -- only where a plain read of D[upper] is above the
//            candidate -- and counts a change when the value the atomic returns was above it.  The changes are reduced over the wave,
//            one add per wave under this round's count.  Round 1 also counts the contacts (one 64-bit add per wave) and notes in the
//            wave's group word whether any of its 64 columns holds one: contacts never change, so in every later round a group
//            without one returns at once.  A round whose predecessor changed nothing returns at once.
//   move   : out is zeroed on the stream; then the same walk stores 1 or 2 at z - drop.  The 2s are counted, one 64-bit add per wave.
//   finish : one lane per record writes drops; moved pieces and the largest drop are reduced over the wave, one add and one max per
//            wave.  Then one thread turns the tail into the record.
//
// Between workgroups.  D only ever falls, and every value ever stored is the length of a real chain of contacts down to something
// static (settle.h).  A lane reads D[lower] with a plain load while other waves of the same round may be lowering it: whatever it sees
// is such a length and at worst larger than the final value, never wrong.  The plain read of D[upper] that guards the atomic can only
// be too large as well, so it never hides a candidate that would lower the true value; what counts as a change is decided by the
// atomic's return alone.  A value that fell in round k is seen by round k + 1: a later kernel, so the stream's order makes it visible
// (the L2s of the XCDs are not coherent and L1 is never refreshed: nothing here relies on either).  A round without a change leaves D at
// a fixed point read in full, which is the answer.  Nothing waits for another workgroup: no spin, no flag poll, no grid barrier.  Every
// loop is bounded by nz, n or log2 n.  The atomics: the min on D, the changes and the contacts (relax), the chosen count (setup), the 2s
// (move), moved pieces and the largest drop (finish); the bytes of the sums are zeroed by launch_settle_setup on the stream.
#include <hip/hip_runtime.h>

#include "global_mem.h"
#include "kernels.h"
#include "settle.h"

namespace bm {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kRecordBlocks = 2048; // the grid of setup and finish at most; their lanes stride over the records

typedef __attribute__((address_space(1))) unsigned long long g_ull;

__device__ __forceinline__ uint32_t word_add(uint32_t* words, uint32_t i, uint32_t v) {
	return __hip_atomic_fetch_add((g_u32*)words + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wide_add(uint32_t* tail, uint32_t i64, uint64_t v) {
	__hip_atomic_fetch_add((g_ull*)tail + i64, static_cast<unsigned long long>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) v += static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), s, 64));
	return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) {
		const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), s, 64));
		v = o > v ? o : v;
	}
	return v;
}

// the table as the search reads it: a record's label is its first word
struct Table {
	const int32_t* records;
	const uint8_t* chosen;
	uint32_t n;
	__device__ __forceinline__ int32_t moving_slot(int32_t label) const {
		return settle_moving_slot([&](uint32_t slot) { return ldi32(records, static_cast<size_t>(slot) * (kSettleRecordBytes / 4)); },
								  [&](uint32_t slot) { return ld8(chosen, slot); }, n, label);
	}
};

// kSettleSlices labels of column `col` from slice z0 on; 0 (empty) past the top
__device__ __forceinline__ void load_slices(const int32_t* labels, const SettleDims& d, uint32_t col, int32_t z0, int32_t (&l)[kSettleSlices]) {
#pragma unroll
	for (int i = 0; i < kSettleSlices; ++i) l[i] = z0 + i < d.nz ? ldi32(labels, static_cast<size_t>(z0 + i) * d.columns + col) : 0;
}

} // namespace

__global__ __launch_bounds__(kThreads) void settle_setup(const uint8_t* __restrict__ chosen, uint32_t* __restrict__ D, uint32_t* tail, const uint32_t n) {
	uint32_t count = 0;
	for (uint32_t base = blockIdx.x * kThreads; base < n; base += gridDim.x * kThreads) {
		const uint32_t s = base + threadIdx.x;
		if (s < n) {
			const bool c = ld8(chosen, s) != 0;
			st32(D, s, c ? kSettleUnknown : 0u);
			count += c ? 1u : 0u;
		}
	}
	count = wave_sum(count);
	if ((threadIdx.x & 63u) == 0 && count != 0) word_add(tail, kSettleTailChosenWord, count);
}

// round `round` (1, 2, ...)
__global__ __launch_bounds__(kThreads) void settle_relax(const int32_t* __restrict__ labels, const int32_t* __restrict__ records, const uint8_t* __restrict__ chosen, uint32_t* D,
														  uint32_t* groups, uint32_t* tail, const uint32_t round, const SettleDims d) {
	if (blockIdx.x == 0 && threadIdx.x == 0) st32(tail, kSettleTailCountWord + (round + 1u) % 3u, 0u); // read by the round before, added under by the next one
	const bool first = round == 1u;
	if (!first && ld32(tail, kSettleTailCountWord + (round - 1u) % 3u) == 0u) return;
	const uint32_t col = blockIdx.x * kThreads + threadIdx.x, group = col >> 6;
	if (group >= d.groups) return; // (wave-uniform: a group is a wave's columns)
	if (!first && ld32(groups, group) == 0u) return;
	const Table table = {records, chosen, d.n};
	uint32_t changes = 0, contacts = 0;
	if (col < d.columns) {
		SettleBelow below = settle_floor();
		for (int32_t z0 = 0; z0 < d.nz; z0 += kSettleSlices) {
			int32_t l[kSettleSlices];
			load_slices(labels, d, col, z0, l);
#pragma unroll
			for (int i = 0; i < kSettleSlices; ++i) {
				if (l[i] == 0) continue;
				SettleContact c;
				if (!settle_step(below, l[i], z0 + i, [&](int32_t label) { return table.moving_slot(label); }, c)) continue;
				++contacts;
				const uint32_t cand = settle_candidate(c.lower >= 0 ? ld32(D, static_cast<uint32_t>(c.lower)) : 0u, c.gap);
				if (cand < ld32(D, static_cast<uint32_t>(c.upper))) {
					const uint32_t old = __hip_atomic_fetch_min((g_u32*)D + c.upper, cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					changes += cand < old ? 1u : 0u;
				}
			}
		}
	}
	const uint32_t lane = threadIdx.x & 63u;
	changes = wave_sum(changes);
	if (lane == 0 && changes != 0) word_add(tail, kSettleTailCountWord + round % 3u, changes);
	if (first) {
		contacts = wave_sum(contacts);
		if (lane == 0) {
			st32(groups, group, contacts != 0 ? 1u : 0u);
			if (contacts != 0) wide_add(tail, 1, contacts);
		}
	}
}

__global__ __launch_bounds__(kThreads) void settle_move(const int32_t* __restrict__ labels, const int32_t* __restrict__ records, const uint8_t* __restrict__ chosen,
														 const uint32_t* __restrict__ D, uint8_t* __restrict__ out, uint32_t* tail, const SettleDims d) {
	const uint32_t col = blockIdx.x * kThreads + threadIdx.x;
	const Table table = {records, chosen, d.n};
	uint32_t moved = 0;
	if (col < d.columns) {
		SettleBelow below = settle_floor();
		uint32_t by = 0; // the drop of below's piece
		for (int32_t z0 = 0; z0 < d.nz; z0 += kSettleSlices) {
			int32_t l[kSettleSlices];
			load_slices(labels, d, col, z0, l);
#pragma unroll
			for (int i = 0; i < kSettleSlices; ++i) {
				if (l[i] == 0) continue;
				const int32_t z = z0 + i;
				const bool same = l[i] == below.label;
				SettleContact c;
				settle_step(below, l[i], z, [&](int32_t label) { return table.moving_slot(label); }, c);
				if (!same) by = below.slot >= 0 ? settle_final_drop(ld32(D, static_cast<uint32_t>(below.slot))) : 0u;
				if (by > static_cast<uint32_t>(z)) continue; // (never, settle.h: the store stays inside the volume whatever D held)
				st8(out, static_cast<size_t>(z - static_cast<int32_t>(by)) * d.columns + col, settle_byte(by));
				moved += by != 0 ? 1u : 0u;
			}
		}
	}
	moved = wave_sum(moved);
	if ((threadIdx.x & 63u) == 0 && moved != 0) wide_add(tail, 0, moved);
}

__global__ __launch_bounds__(kThreads) void settle_finish(const uint8_t* __restrict__ chosen, const uint32_t* __restrict__ D, int32_t* __restrict__ drops, uint32_t* tail,
														   const uint32_t n) {
	uint32_t moved = 0, largest = 0;
	for (uint32_t base = blockIdx.x * kThreads; base < n; base += gridDim.x * kThreads) {
		const uint32_t s = base + threadIdx.x;
		if (s < n) {
			const uint32_t by = ld8(chosen, s) != 0 ? settle_final_drop(ld32(D, s)) : 0u;
			((g_i32*)drops)[s] = static_cast<int32_t>(by);
			moved += by != 0 ? 1u : 0u;
			largest = by > largest ? by : largest;
		}
	}
	moved = wave_sum(moved);
	largest = wave_max(largest);
	if ((threadIdx.x & 63u) == 0 && moved != 0) {
		word_add(tail, kSettleTailMovedWord, moved);
		__hip_atomic_fetch_max((g_u32*)tail + kSettleTailLargestWord, largest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// the tail -> the 32 bytes of the result
__global__ __launch_bounds__(64) void settle_record_out(const uint32_t* __restrict__ tail, uint64_t* __restrict__ result) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const uint64_t* wide = reinterpret_cast<const uint64_t*>(tail);
	st64(result, 0, ld64(wide, 0));
	st64(result, 1, static_cast<uint64_t>(ld32(tail, kSettleTailChosenWord)) | static_cast<uint64_t>(ld32(tail, kSettleTailMovedWord)) << 32);
	st64(result, 2, static_cast<uint64_t>(ld32(tail, kSettleTailLargestWord)));
	st64(result, 3, ld64(wide, 1));
}

// ---- host-callable launchers (kernels.h)
namespace {
unsigned blocks_for(uint64_t items, uint64_t per_block, uint64_t most) {
	const uint64_t b = (items + per_block - 1) / per_block;
	return static_cast<unsigned>(b < most ? (b ? b : 1) : most);
}
uint32_t* settle_groups(const SettleDims& d, void* workspace) { return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(workspace) + settle_groups_offset(d)); }
} // namespace

void launch_settle_setup(const SettleDims& d, const uint8_t* chosen, void* workspace, hipStream_t stream) {
	(void)hipMemsetAsync(settle_tail_at(d, workspace), 0, kSettleTailBytes, stream); // every sum of this call
	if (d.n > 0)
		hipLaunchKernelGGL(settle_setup, dim3(blocks_for(d.n, kThreads, kRecordBlocks)), dim3(kThreads), 0, stream, chosen, static_cast<uint32_t*>(workspace), settle_tail_at(d, workspace),
						   d.n);
}

void launch_settle_rounds(const SettleDims& d, const int32_t* labels, const void* records, const uint8_t* chosen, void* workspace, uint32_t first_round, uint32_t rounds,
						  hipStream_t stream) {
	const unsigned blocks = (d.columns + kThreads - 1) / kThreads; // at most 2^20: 16384^2 columns
	for (uint32_t k = first_round; k < first_round + rounds; ++k)
		hipLaunchKernelGGL(settle_relax, dim3(blocks), dim3(kThreads), 0, stream, labels, static_cast<const int32_t*>(records), chosen, static_cast<uint32_t*>(workspace),
						   settle_groups(d, workspace), settle_tail_at(d, workspace), k, d);
}

void launch_settle_move(const SettleDims& d, const int32_t* labels, const void* records, const uint8_t* chosen, uint8_t* out, int32_t* drops, void* result, void* workspace,
						hipStream_t stream) {
	(void)hipMemsetAsync(out, 0, d.voxels, stream);
	hipLaunchKernelGGL(settle_move, dim3((d.columns + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, labels, static_cast<const int32_t*>(records), chosen,
					   static_cast<const uint32_t*>(workspace), out, settle_tail_at(d, workspace), d);
	if (d.n > 0)
		hipLaunchKernelGGL(settle_finish, dim3(blocks_for(d.n, kThreads, kRecordBlocks)), dim3(kThreads), 0, stream, chosen, static_cast<const uint32_t*>(workspace), drops,
						   settle_tail_at(d, workspace), d.n);
	hipLaunchKernelGGL(settle_record_out, dim3(1), dim3(64), 0, stream, static_cast<const uint32_t*>(settle_tail_at(d, workspace)), static_cast<uint64_t*>(result));
}

} // namespace bm
