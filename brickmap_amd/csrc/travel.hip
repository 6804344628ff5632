// travel.hip -- exact shortest face-step distances of a byte volume from a set of seeds on the device, and paths down the field
// (bm_travel_field, bm_travel_paths), by the rules of travel.h.  The volume is cut into 8^3 tiles.
//
//   setup  : one wave per tile, one x-row of eight voxels per lane (the layout of label_local): the row's bytes become the row's byte of
//            the tile's 64-byte bit brick of blocked voxels in the workspace (voxels outside the volume are blocked), and its voxels of
//            the field become BM_TRAVEL_NONE.  No later kernel reads the byte volume.
//   seed   : one lane per seed: inside the volume and not blocked -> 0 into the field and the seed's tile onto the list of round 1,
//            once (the stamp); the others are counted, one add per wave.
//   relax  : a round.  One wave per listed tile -- the grid is bounded, the waves stride over the list, whose count is read from the
//            tail, so a round with an empty list ends at once.  The wave loads its 512 values (open voxels only) and takes the values
//            across its six faces once: they are constants of the round.  Then it settles in registers (travel_row_sweep; the four
//            neighbouring rows by lane shuffles) until a ballot says no row changed, 512 sweeps at most.  It stores the values that fell
//            and, for each face on which one fell, puts the tile across it on the next round's list: an atomic max of the tile's stamp
//            with the next round's number says by its return whether this wave is the first to do so.  Nothing is ever cleared.
//   finish : one pass over the field: the finite values' count and the max key, reduced over the wave, one add and one max per wave; then
//            one thread turns the tail into the record.
//   paths  : one lane per start walks down the field (travel_walk).
//
// Between workgroups.  A wave reads values of neighbouring tiles that other waves of the same round may be rewriting, with plain loads:
// whatever it sees is the length of a real path and at worst larger than the final value (travel.h), and the tile whose face value fell
// lists this one for the next round -- a later kernel, so the stream's order makes the value visible then (the L2s of the XCDs are not
// coherent and L1 is never refreshed: nothing here relies on either).  No tile is on a list twice, so no tile is written by two waves of
// a round.  Nothing waits for another workgroup: no spin, no flag poll, no grid barrier, no persistent hand-off.  Every loop is bounded
// by an extent, the list's length, kTravelTileSweeps, T(start) or capacity.  The atomics: the stamp and the list append (seed, relax),
// the reject count (seed), the count and the key (finish); the bytes they live in are zeroed by launch_travel_setup on the stream.
#include <hip/hip_runtime.h>

#include "global_mem.h"
#include "kernels.h"
#include "tile_lists.h"
#include "travel.h"
#include "voxel_bits.h"

namespace bm {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kStreamBlocks = 2048; // the grid of setup, seed and finish at most: eight workgroups for each of 256 compute units

typedef __attribute__((address_space(1))) unsigned long long g_ull;

} // namespace

__global__ __launch_bounds__(kThreads) void travel_setup(const uint8_t* __restrict__ volume, uint32_t* __restrict__ field, uint8_t* __restrict__ bricks, const TravelDims d) {
	const uint32_t r = threadIdx.x & 63u;
	const int32_t nx = d.extent[0], ny = d.extent[1], nz = d.extent[2];
	for (uint32_t tile = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); tile < d.tile_count; tile += gridDim.x * (kThreads / 64)) {
		const TilePlace p = tile_place(d, tile);
		const int32_t x0 = static_cast<int32_t>(p.tx * 8u), y = static_cast<int32_t>(p.ty * 8u + (r & 7u)), z = static_cast<int32_t>(p.tz * 8u + (r >> 3));
		uint32_t blocked = 0xFFu;
		if (y < ny && z < nz) {
			const int64_t at = static_cast<int64_t>(z) * d.slice_pitch + static_cast<int64_t>(y) * d.row_pitch + x0;
			const size_t out = travel_voxel_index(d, static_cast<uint32_t>(x0), static_cast<uint32_t>(y), static_cast<uint32_t>(z));
			uint32_t lo = 0, hi = 0, outside = 0;
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				if (x0 + i < nx) {
					const uint32_t b = ld8(volume, static_cast<size_t>(at + i));
					if (i < 4) lo |= b << (8 * i); else hi |= b << (8 * (i - 4));
					st32(field, out + i, kTravelNone);
				} else {
					outside |= 1u << i;
				}
			}
			blocked = brick_row_bits(lo, hi) | outside;
		}
		st8(bricks, static_cast<size_t>(tile) * 64 + r, blocked);
	}
}

__global__ __launch_bounds__(kThreads) void travel_seed(const int32_t* __restrict__ seeds, const uint32_t n, uint32_t* __restrict__ field, const uint8_t* __restrict__ bricks,
														 uint32_t* stamps, uint32_t* __restrict__ list, uint32_t* tail, const TravelDims d) {
	uint32_t rejected = 0; // (ballots: the same in every lane)
	for (uint32_t base = blockIdx.x * kThreads; base < n; base += gridDim.x * kThreads) {
		const uint32_t s = base + threadIdx.x;
		const bool live = s < n;
		bool ok = false;
		if (live) {
			const int32_t x = ldi32(seeds, 3 * static_cast<size_t>(s)), y = ldi32(seeds, 3 * static_cast<size_t>(s) + 1), z = ldi32(seeds, 3 * static_cast<size_t>(s) + 2);
			if (x >= 0 && y >= 0 && z >= 0 && x < d.extent[0] && y < d.extent[1] && z < d.extent[2]) {
				const uint32_t ux = static_cast<uint32_t>(x), uy = static_cast<uint32_t>(y), uz = static_cast<uint32_t>(z);
				const uint32_t tile = travel_tile_index(d, ux >> 3, uy >> 3, uz >> 3);
				const uint32_t row = ld8(bricks, static_cast<size_t>(tile) * 64 + (uy & 7u) + 8u * (uz & 7u));
				if (!((row >> (ux & 7u)) & 1u)) {
					ok = true;
					st32(field, travel_voxel_index(d, ux, uy, uz), 0u);
					list_tile(stamps, list, tail, kTravelTailCountWord + 1u, tile, 1u, d.tile_count);
				}
			}
		}
		rejected += static_cast<uint32_t>(__popcll(__ballot(live && !ok)));
	}
	if ((threadIdx.x & 63u) == 0 && rejected != 0) word_add(tail, kTravelTailRejectedWord, rejected);
}

// round `round` (1, 2, ...): the tiles of `list` (count: word round % 3 of the tail's counts) are settled; `next` takes the tiles across
// the faces on which a value fell
__global__ __launch_bounds__(kThreads) void travel_relax(uint32_t* field, const uint8_t* __restrict__ bricks, uint32_t* stamps, const uint32_t* __restrict__ list,
														  uint32_t* __restrict__ next, uint32_t* tail, const uint32_t round, const TravelDims d) {
	const uint32_t count = ld32(tail, kTravelTailCountWord + round % 3u), listed = count < d.tile_count ? count : d.tile_count;
	if (blockIdx.x == 0 && threadIdx.x == 0) st32(tail, kTravelTailCountWord + (round + 2u) % 3u, 0u); // read by the round before, appended under by the next one
	const uint32_t r = threadIdx.x & 63u;
	const uint32_t nx = static_cast<uint32_t>(d.extent[0]), ny = static_cast<uint32_t>(d.extent[1]), nz = static_cast<uint32_t>(d.extent[2]);
	const uint32_t limit = d.limit, next_word = kTravelTailCountWord + (round + 1u) % 3u;
	const int src[4] = {static_cast<int>(r) - 1, static_cast<int>(r) + 1, static_cast<int>(r) - 8, static_cast<int>(r) + 8};
	// kTravelNone where the tile has no such row: a value | kTravelNone is kTravelNone
	const uint32_t lack[4] = {(r & 7u) != 0 ? 0u : kTravelNone, (r & 7u) != 7 ? 0u : kTravelNone, (r >> 3) != 0 ? 0u : kTravelNone, (r >> 3) != 7 ? 0u : kTravelNone};
	for (uint32_t at = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); at < listed; at += gridDim.x * (kThreads / 64)) {
		const uint32_t tile = ld32(list, at);
		if (tile >= d.tile_count) continue; // (never: the lists hold tiles)
		const TilePlace p = tile_place(d, tile);
		// (a voxel outside the volume is blocked: an open bit says that its voxel, and with it the row, lies inside)
		const uint32_t open = ~ld8(bricks, static_cast<size_t>(tile) * 64 + r) & 0xFFu;
		if (__ballot(open != 0) == 0) continue;
		const uint32_t x0 = p.tx * 8u, y = p.ty * 8u + (r & 7u), z = p.tz * 8u + (r >> 3);
		const size_t base = open ? travel_voxel_index(d, x0, y, z) : 0u;
		uint32_t t[8], was[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			t[i] = ((open >> i) & 1u) ? ld32(field, base + i) : kTravelNone;
			was[i] = round == 1u && t[i] == 0u ? kTravelNone : t[i]; // a seed counts as fallen in the first round: its neighbours across a face hear of it
		}
		// the six faces' values, once
		if ((open & 1u) && x0 > 0) t[0] = travel_take(t[0], ld32(field, base - 1), true, limit);
		if ((open & 0x80u) && x0 + 8u < nx) t[7] = travel_take(t[7], ld32(field, base + 8), true, limit);
		if (open != 0 && (r & 7u) == 0 && y > 0) {
#pragma unroll
			for (int i = 0; i < 8; ++i)
				if ((open >> i) & 1u) t[i] = travel_take(t[i], ld32(field, base - nx + i), true, limit);
		}
		if (open != 0 && (r & 7u) == 7 && y + 1u < ny) {
#pragma unroll
			for (int i = 0; i < 8; ++i)
				if ((open >> i) & 1u) t[i] = travel_take(t[i], ld32(field, base + nx + i), true, limit);
		}
		const size_t slice = static_cast<size_t>(nx) * ny;
		if (open != 0 && (r >> 3) == 0 && z > 0) {
#pragma unroll
			for (int i = 0; i < 8; ++i)
				if ((open >> i) & 1u) t[i] = travel_take(t[i], ld32(field, base - slice + i), true, limit);
		}
		if (open != 0 && (r >> 3) == 7 && z + 1u < nz) {
#pragma unroll
			for (int i = 0; i < 8; ++i)
				if ((open >> i) & 1u) t[i] = travel_take(t[i], ld32(field, base + slice + i), true, limit);
		}
#pragma unroll 1
		for (int sweep = 0; sweep < kTravelTileSweeps; ++sweep) { // bounded (travel.h); ends as soon as no lane's row changed
			uint32_t near[8];
#pragma unroll
			for (int i = 0; i < 8; ++i) near[i] = kTravelNone;
#pragma unroll
			for (int k = 0; k < 4; ++k)
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					const uint32_t v = static_cast<uint32_t>(__shfl(static_cast<int>(t[i]), src[k] & 63, 64));
					const uint32_t w = v | lack[k];
					near[i] = w < near[i] ? w : near[i];
				}
			const bool changed = travel_row_sweep(t, open, near, limit);
			if (__ballot(changed) == 0) break;
		}
		bool fell = false;
#pragma unroll
		for (int i = 0; i < 8; ++i)
			if (t[i] < was[i]) {
				st32(field, base + i, t[i]);
				fell = true;
			}
		// the faces on which a value fell, and the tiles across them
		const bool faces[6] = {t[0] < was[0] && p.tx > 0,
							   t[7] < was[7] && p.tx + 1u < d.tiles[0],
							   fell && (r & 7u) == 0 && p.ty > 0,
							   fell && (r & 7u) == 7 && p.ty + 1u < d.tiles[1],
							   fell && (r >> 3) == 0 && p.tz > 0,
							   fell && (r >> 3) == 7 && p.tz + 1u < d.tiles[2]};
		const uint32_t step[3] = {1u, d.tiles[0], d.tiles[0] * d.tiles[1]};
#pragma unroll
		for (int f = 0; f < 6; ++f) {
			const bool any = __ballot(faces[f]) != 0;
			if (any && r == 0) list_tile(stamps, next, tail, next_word, (f & 1) ? tile + step[f >> 1] : tile - step[f >> 1], round + 1u, d.tile_count);
		}
	}
}

__global__ __launch_bounds__(kThreads) void travel_finish(const uint32_t* __restrict__ field, const uint32_t n, unsigned long long* __restrict__ tail) {
	uint64_t best = 0;
	uint32_t count = 0;
	for (uint32_t base = blockIdx.x * kThreads; base < n; base += gridDim.x * kThreads) {
		const uint32_t i = base + threadIdx.x;
		if (i < n) {
			const uint32_t v = ld32(field, i);
			count += v != kTravelNone ? 1u : 0u;
			const uint64_t k = travel_max_key(v, i);
			best = k > best ? k : best;
		}
	}
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) {
		const uint64_t other = static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(best), s, 64));
		best = other > best ? other : best;
		count += static_cast<uint32_t>(__shfl_xor(static_cast<int>(count), s, 64));
	}
	if ((threadIdx.x & 63u) == 0 && count != 0) {
		__hip_atomic_fetch_add((g_ull*)tail + 1, static_cast<unsigned long long>(count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_max((g_ull*)tail, static_cast<unsigned long long>(best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// the tail -> the 32 bytes of the result
__global__ __launch_bounds__(64) void travel_record_out(const uint64_t* __restrict__ tail, uint64_t* __restrict__ result) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const TravelRecord rec = travel_record(ld64(tail, 0), ld64(tail, 1), static_cast<uint32_t>(ld64(tail, 2)));
	st64(result, 0, rec.reached);
	st64(result, 1, static_cast<uint64_t>(rec.farthest) | static_cast<uint64_t>(rec.seeds_rejected) << 32);
	st64(result, 2, rec.farthest_at);
	st64(result, 3, 0);
}

__global__ __launch_bounds__(kThreads) void travel_paths(const uint32_t* __restrict__ field, const int32_t* __restrict__ starts, const uint32_t n, const int32_t capacity,
														  int32_t* __restrict__ path, int32_t* __restrict__ lengths, const TravelDims d) {
	const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
	if (q >= n) return;
	const int32_t extent[3] = {d.extent[0], d.extent[1], d.extent[2]};
	g_i32* out = (g_i32*)path + static_cast<size_t>(q) * static_cast<size_t>(capacity) * 3;
	const int32_t length = travel_walk(
		extent, ldi32(starts, 3 * static_cast<size_t>(q)), ldi32(starts, 3 * static_cast<size_t>(q) + 1), ldi32(starts, 3 * static_cast<size_t>(q) + 2), capacity,
		[&](int32_t x, int32_t y, int32_t z) { return ld32(field, travel_voxel_index(d, static_cast<uint32_t>(x), static_cast<uint32_t>(y), static_cast<uint32_t>(z))); },
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
} // namespace

void launch_travel_setup(const TravelDims& d, const uint8_t* volume, const int32_t* seeds, uint32_t n, uint32_t* field, void* workspace, hipStream_t stream) {
	uint8_t* ws = static_cast<uint8_t*>(workspace);
	uint32_t* stamps = reinterpret_cast<uint32_t*>(ws + travel_stamps_offset(d));
	uint32_t* tail = reinterpret_cast<uint32_t*>(ws + travel_tail_offset(d));
	(void)hipMemsetAsync(stamps, 0, travel_words_bytes(d) + kTravelTailBytes, stream); // every byte an atomic of this call lives in
	hipLaunchKernelGGL(travel_setup, dim3(blocks_for(d.tile_count, kThreads / 64, 4 * kStreamBlocks)), dim3(kThreads), 0, stream, volume, field, ws, d);
	if (n > 0)
		hipLaunchKernelGGL(travel_seed, dim3(blocks_for(n, kThreads, kStreamBlocks)), dim3(kThreads), 0, stream, seeds, n, field, static_cast<const uint8_t*>(ws), stamps,
						   reinterpret_cast<uint32_t*>(ws + travel_list_offset(d, 1)), tail, d);
}

void launch_travel_rounds(const TravelDims& d, uint32_t* field, void* workspace, uint32_t first_round, uint32_t rounds, hipStream_t stream) {
	uint8_t* ws = static_cast<uint8_t*>(workspace);
	uint32_t* stamps = reinterpret_cast<uint32_t*>(ws + travel_stamps_offset(d));
	uint32_t* tail = reinterpret_cast<uint32_t*>(ws + travel_tail_offset(d));
	const unsigned blocks = blocks_for(d.tile_count, kThreads / 64, kTravelMaxWaves / (kThreads / 64));
	for (uint32_t k = first_round; k < first_round + rounds; ++k)
		hipLaunchKernelGGL(travel_relax, dim3(blocks), dim3(kThreads), 0, stream, field, static_cast<const uint8_t*>(ws), stamps,
						   reinterpret_cast<const uint32_t*>(ws + travel_list_offset(d, k & 1u)), reinterpret_cast<uint32_t*>(ws + travel_list_offset(d, (k + 1u) & 1u)), tail, k, d);
}

void launch_travel_finish(const TravelDims& d, const uint32_t* field, void* result, void* workspace, hipStream_t stream) {
	unsigned long long* tail = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(workspace) + travel_tail_offset(d));
	hipLaunchKernelGGL(travel_finish, dim3(blocks_for(d.voxels, kThreads, kStreamBlocks)), dim3(kThreads), 0, stream, field, d.voxels, tail);
	hipLaunchKernelGGL(travel_record_out, dim3(1), dim3(64), 0, stream, reinterpret_cast<const uint64_t*>(tail), static_cast<uint64_t*>(result));
}

void launch_travel_paths(const TravelDims& d, const uint32_t* field, const int32_t* starts, uint32_t n, int32_t capacity, int32_t* path, int32_t* lengths, hipStream_t stream) {
	hipLaunchKernelGGL(travel_paths, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, field, starts, n, capacity, path, lengths, d);
}

} // namespace bm
