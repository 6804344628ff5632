// water.hip -- exact spill levels of a byte volume on the device and the mask of its pools (bm_water_field, bm_water_mask), by the rules
// of water.h.  The volume is cut into 8^3 tiles; the tiles, the workspace and the rounds are those of travel.hip (travel.h, tile_lists.h).
//
//   setup  : one wave per tile, one x-row of eight voxels per lane: the row's bytes become the row's byte of the tile's 64-byte bit brick
//            of solid voxels in the workspace (voxels outside the volume are solid), and its voxels of the field become max(z, sea_level)
//            where the voxel is free and lies on an open face of the box, BM_WATER_NONE elsewhere.  A tile that holds such an outlet goes
//            onto the list of round 1 (the stamp).  No later kernel of the field reads the byte volume.
//   drain  : one lane per drain: inside the volume and free -> max(z, sea_level) into the field and the drain's tile onto the list of
//            round 1, once; the others are counted, one add per wave.
//   relax  : a round, with the structure of travel_relax.  One wave per listed tile -- the grid is bounded, the waves stride over the
//            list, whose count is read from the tail, so a round with an empty list ends at once.  The wave loads its 512 values (free
//            voxels only) and takes the values across its six faces once: they are constants of the round.  Then it settles in registers
//            (water_row_sweep; the four neighbouring rows by lane shuffles) until a ballot says no row changed, 512 sweeps at most.  It
//            stores the values that fell -- in round 1 every finite value counts as fallen, so that an outlet's neighbours across a face
//            hear of it -- and, for each face on which one fell, puts the tile across it on the next round's list.
//   finish : one pass, tile by tile: the wet and the closed voxels' counts and the depth key, reduced over the wave, one add per count
//            and one max per wave (free or solid: the brick's bit); then one thread turns the tail into the record.
//   mask   : one voxel per lane.
//
// Between workgroups: as in travel.hip.  A wave reads values of neighbouring tiles that other waves of the same round may be rewriting,
// with plain loads: whatever it sees is a real path's bottleneck and at worst larger than the final value (water.h), and the tile whose
// face value fell lists this one for the next round -- a later kernel, so the stream's order makes the value visible then.  No tile is on
// a list twice, so no tile is written by two waves of a round.  Nothing waits for another workgroup: no spin, no flag poll, no grid
// barrier.  Every loop is bounded by an extent, the list's length or kTravelTileSweeps.  The atomics: the stamp and the list append
// (setup, drain, relax), the reject count (drain), the counts and the key (finish); the bytes they live in are zeroed by
// launch_water_setup on the stream.  The visits word of the tail is written by one thread per round, in stream order.
#include <hip/hip_runtime.h>

#include "global_mem.h"
#include "kernels.h"
#include "tile_lists.h"
#include "voxel_bits.h"
#include "water.h"

namespace bm {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kStreamBlocks = 2048; // the grid of setup, drain, finish and mask at most: eight workgroups for each of 256 compute units

typedef __attribute__((address_space(1))) unsigned long long g_ull;

} // namespace

__global__ __launch_bounds__(kThreads) void water_setup(const uint8_t* __restrict__ volume, uint32_t* __restrict__ field, uint8_t* __restrict__ bricks, uint32_t* stamps,
														uint32_t* __restrict__ list, uint32_t* tail, const uint32_t sea, const uint32_t faces, const TravelDims d) {
	const uint32_t r = threadIdx.x & 63u;
	const int32_t nx = d.extent[0], ny = d.extent[1], nz = d.extent[2];
	const int32_t extent[3] = {nx, ny, nz};
	for (uint32_t tile = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); tile < d.tile_count; tile += gridDim.x * (kThreads / 64)) {
		const TilePlace p = tile_place(d, tile);
		const int32_t x0 = static_cast<int32_t>(p.tx * 8u), y = static_cast<int32_t>(p.ty * 8u + (r & 7u)), z = static_cast<int32_t>(p.tz * 8u + (r >> 3));
		uint32_t solid = 0xFFu;
		bool outlet = false;
		if (y < ny && z < nz) {
			const int64_t at = static_cast<int64_t>(z) * d.slice_pitch + static_cast<int64_t>(y) * d.row_pitch + x0;
			const size_t out = travel_voxel_index(d, static_cast<uint32_t>(x0), static_cast<uint32_t>(y), static_cast<uint32_t>(z));
			const uint32_t start = water_start(static_cast<uint32_t>(z), sea);
			uint32_t lo = 0, hi = 0, outside = 0;
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				if (x0 + i < nx) {
					const uint32_t b = ld8(volume, static_cast<size_t>(at + i));
					if (i < 4) lo |= b << (8 * i); else hi |= b << (8 * (i - 4));
					const bool here = b == 0 && (water_faces_of(extent, x0 + i, y, z) & faces) != 0;
					st32(field, out + i, here ? start : kWaterNone);
					outlet |= here;
				} else {
					outside |= 1u << i;
				}
			}
			solid = brick_row_bits(lo, hi) | outside;
		}
		st8(bricks, static_cast<size_t>(tile) * 64 + r, solid);
		const bool any = __ballot(outlet) != 0;
		if (any && r == 0) list_tile(stamps, list, tail, kTravelTailCountWord + 1u, tile, 1u, d.tile_count);
	}
}

__global__ __launch_bounds__(kThreads) void water_drain(const int32_t* __restrict__ drains, const uint32_t n, uint32_t* __restrict__ field, const uint8_t* __restrict__ bricks,
														uint32_t* stamps, uint32_t* __restrict__ list, uint32_t* tail, const uint32_t sea, const TravelDims d) {
	uint32_t rejected = 0; // (ballots: the same in every lane)
	for (uint32_t base = blockIdx.x * kThreads; base < n; base += gridDim.x * kThreads) {
		const uint32_t s = base + threadIdx.x;
		const bool live = s < n;
		bool ok = false;
		if (live) {
			const int32_t x = ldi32(drains, 3 * static_cast<size_t>(s)), y = ldi32(drains, 3 * static_cast<size_t>(s) + 1), z = ldi32(drains, 3 * static_cast<size_t>(s) + 2);
			if (x >= 0 && y >= 0 && z >= 0 && x < d.extent[0] && y < d.extent[1] && z < d.extent[2]) {
				const uint32_t ux = static_cast<uint32_t>(x), uy = static_cast<uint32_t>(y), uz = static_cast<uint32_t>(z);
				const uint32_t tile = travel_tile_index(d, ux >> 3, uy >> 3, uz >> 3);
				const uint32_t row = ld8(bricks, static_cast<size_t>(tile) * 64 + (uy & 7u) + 8u * (uz & 7u));
				if (!((row >> (ux & 7u)) & 1u)) {
					ok = true;
					st32(field, travel_voxel_index(d, ux, uy, uz), water_start(uz, sea));
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
__global__ __launch_bounds__(kThreads) void water_relax(uint32_t* field, const uint8_t* __restrict__ bricks, uint32_t* stamps, const uint32_t* __restrict__ list,
														uint32_t* __restrict__ next, uint32_t* tail, const uint32_t round, const TravelDims d) {
	const uint32_t count = ld32(tail, kTravelTailCountWord + round % 3u), listed = count < d.tile_count ? count : d.tile_count;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		st32(tail, kTravelTailCountWord + (round + 2u) % 3u, 0u); // read by the round before, appended under by the next one
		st32(tail, kWaterTailVisitsWord, ld32(tail, kWaterTailVisitsWord) + listed); // (this thread alone writes the word, one round after the other)
	}
	const uint32_t r = threadIdx.x & 63u;
	const uint32_t nx = static_cast<uint32_t>(d.extent[0]), ny = static_cast<uint32_t>(d.extent[1]), nz = static_cast<uint32_t>(d.extent[2]);
	const uint32_t next_word = kTravelTailCountWord + (round + 1u) % 3u;
	const int src[4] = {static_cast<int>(r) - 1, static_cast<int>(r) + 1, static_cast<int>(r) - 8, static_cast<int>(r) + 8};
	// kWaterNone where the tile has no such row: a value | kWaterNone is kWaterNone
	const uint32_t lack[4] = {(r & 7u) != 0 ? 0u : kWaterNone, (r & 7u) != 7 ? 0u : kWaterNone, (r >> 3) != 0 ? 0u : kWaterNone, (r >> 3) != 7 ? 0u : kWaterNone};
	for (uint32_t at = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); at < listed; at += gridDim.x * (kThreads / 64)) {
		const uint32_t tile = ld32(list, at);
		if (tile >= d.tile_count) continue; // (never: the lists hold tiles)
		const TilePlace p = tile_place(d, tile);
		// (a voxel outside the volume is solid: an open bit says that its voxel, and with it the row, lies inside)
		const uint32_t open = ~ld8(bricks, static_cast<size_t>(tile) * 64 + r) & 0xFFu;
		if (__ballot(open != 0) == 0) continue;
		const uint32_t x0 = p.tx * 8u, y = p.ty * 8u + (r & 7u), z = p.tz * 8u + (r >> 3);
		const size_t base = open ? travel_voxel_index(d, x0, y, z) : 0u;
		uint32_t t[8], was[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			t[i] = ((open >> i) & 1u) ? ld32(field, base + i) : kWaterNone;
			was[i] = round == 1u ? kWaterNone : t[i]; // every finite value counts as fallen in the first round: an outlet's neighbours across a face hear of it
		}
		// the six faces' values, once; across a z face the neighbour's value is raised to this row's height like any other
		if ((open & 1u) && x0 > 0) t[0] = water_step(t[0], ld32(field, base - 1), z, true);
		if ((open & 0x80u) && x0 + 8u < nx) t[7] = water_step(t[7], ld32(field, base + 8), z, true);
		if (open != 0 && (r & 7u) == 0 && y > 0) {
#pragma unroll
			for (int i = 0; i < 8; ++i)
				if ((open >> i) & 1u) t[i] = water_step(t[i], ld32(field, base - nx + i), z, true);
		}
		if (open != 0 && (r & 7u) == 7 && y + 1u < ny) {
#pragma unroll
			for (int i = 0; i < 8; ++i)
				if ((open >> i) & 1u) t[i] = water_step(t[i], ld32(field, base + nx + i), z, true);
		}
		const size_t slice = static_cast<size_t>(nx) * ny;
		if (open != 0 && (r >> 3) == 0 && z > 0) {
#pragma unroll
			for (int i = 0; i < 8; ++i)
				if ((open >> i) & 1u) t[i] = water_step(t[i], ld32(field, base - slice + i), z, true);
		}
		if (open != 0 && (r >> 3) == 7 && z + 1u < nz) {
#pragma unroll
			for (int i = 0; i < 8; ++i)
				if ((open >> i) & 1u) t[i] = water_step(t[i], ld32(field, base + slice + i), z, true);
		}
#pragma unroll 1
		for (int sweep = 0; sweep < kTravelTileSweeps; ++sweep) { // bounded (water.h); ends as soon as no lane's row changed
			uint32_t near[8];
#pragma unroll
			for (int i = 0; i < 8; ++i) near[i] = kWaterNone;
#pragma unroll
			for (int k = 0; k < 4; ++k)
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					const uint32_t v = static_cast<uint32_t>(__shfl(static_cast<int>(t[i]), src[k] & 63, 64));
					const uint32_t w = v | lack[k];
					near[i] = w < near[i] ? w : near[i];
				}
			const bool changed = water_row_sweep(t, open, near, z);
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

// the tail as 64-bit words: the key at 0, the wet count at 1, the closed count at kWaterTailClosedWord64
__global__ __launch_bounds__(kThreads) void water_finish(const uint32_t* __restrict__ field, const uint8_t* __restrict__ bricks, unsigned long long* __restrict__ tail,
														 const TravelDims d) {
	const uint32_t r = threadIdx.x & 63u;
	uint64_t best = 0;
	uint32_t wet = 0, closed = 0;
	for (uint32_t tile = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); tile < d.tile_count; tile += gridDim.x * (kThreads / 64)) {
		const TilePlace p = tile_place(d, tile);
		const uint32_t open = ~ld8(bricks, static_cast<size_t>(tile) * 64 + r) & 0xFFu;
		if (open == 0) continue; // (an open bit says that its voxel, and with it the row, lies inside the volume)
		const uint32_t z = p.tz * 8u + (r >> 3);
		const uint32_t base = travel_voxel_index(d, p.tx * 8u, p.ty * 8u + (r & 7u), z);
#pragma unroll
		for (int i = 0; i < 8; ++i)
			if ((open >> i) & 1u) {
				const uint32_t v = ld32(field, base + i);
				wet += water_wet(v, z) ? 1u : 0u;
				closed += v == kWaterNone ? 1u : 0u;
				const uint64_t k = water_depth_key(v, z, base + static_cast<uint32_t>(i));
				best = k > best ? k : best;
			}
	}
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) {
		const uint64_t other = static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(best), s, 64));
		best = other > best ? other : best;
		wet += static_cast<uint32_t>(__shfl_xor(static_cast<int>(wet), s, 64));
		closed += static_cast<uint32_t>(__shfl_xor(static_cast<int>(closed), s, 64));
	}
	if ((threadIdx.x & 63u) == 0) {
		if (closed != 0) __hip_atomic_fetch_add((g_ull*)tail + kWaterTailClosedWord64, static_cast<unsigned long long>(closed), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (wet != 0) {
			__hip_atomic_fetch_add((g_ull*)tail + 1, static_cast<unsigned long long>(wet), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__hip_atomic_fetch_max((g_ull*)tail, static_cast<unsigned long long>(best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}

// the tail -> the 32 bytes of the result
__global__ __launch_bounds__(64) void water_record_out(const uint64_t* __restrict__ tail, uint64_t* __restrict__ result) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const WaterRecord rec = water_record(ld64(tail, 0), ld64(tail, 1), static_cast<uint32_t>(ld64(tail, 2)), ld64(tail, kWaterTailClosedWord64));
	st64(result, 0, rec.wet);
	st64(result, 1, static_cast<uint64_t>(rec.deepest) | static_cast<uint64_t>(rec.drains_rejected) << 32);
	st64(result, 2, rec.deepest_at);
	st64(result, 3, rec.closed);
}

// slice blockIdx.y of the field -> the slice's bytes of the mask
__global__ __launch_bounds__(kThreads) void water_mask(const uint32_t* __restrict__ field, const uint32_t slice, const uint32_t min_depth, uint8_t* __restrict__ mask) {
	const uint32_t z = blockIdx.y;
	const size_t at = static_cast<size_t>(z) * slice;
	for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < slice; i += gridDim.x * kThreads) st8(mask, at + i, water_mask_byte(ld32(field, at + i), z, min_depth));
}

// ---- host-callable launchers (kernels.h)
namespace {
unsigned blocks_for(uint64_t items, uint64_t per_block, uint64_t most) {
	const uint64_t b = (items + per_block - 1) / per_block;
	return static_cast<unsigned>(b < most ? (b ? b : 1) : most);
}
} // namespace

void launch_water_setup(const TravelDims& d, uint32_t sea, uint32_t faces, const uint8_t* volume, const int32_t* drains, uint32_t n, uint32_t* field, void* workspace,
						hipStream_t stream) {
	uint8_t* ws = static_cast<uint8_t*>(workspace);
	uint32_t* stamps = reinterpret_cast<uint32_t*>(ws + travel_stamps_offset(d));
	uint32_t* tail = reinterpret_cast<uint32_t*>(ws + travel_tail_offset(d));
	uint32_t* first = reinterpret_cast<uint32_t*>(ws + travel_list_offset(d, 1));
	(void)hipMemsetAsync(stamps, 0, travel_words_bytes(d) + kTravelTailBytes, stream); // every byte an atomic of this call lives in
	hipLaunchKernelGGL(water_setup, dim3(blocks_for(d.tile_count, kThreads / 64, 4 * kStreamBlocks)), dim3(kThreads), 0, stream, volume, field, ws, stamps, first, tail, sea, faces, d);
	if (n > 0)
		hipLaunchKernelGGL(water_drain, dim3(blocks_for(n, kThreads, kStreamBlocks)), dim3(kThreads), 0, stream, drains, n, field, static_cast<const uint8_t*>(ws), stamps, first, tail,
						   sea, d);
}

void launch_water_rounds(const TravelDims& d, uint32_t* field, void* workspace, uint32_t first_round, uint32_t rounds, hipStream_t stream) {
	uint8_t* ws = static_cast<uint8_t*>(workspace);
	uint32_t* stamps = reinterpret_cast<uint32_t*>(ws + travel_stamps_offset(d));
	uint32_t* tail = reinterpret_cast<uint32_t*>(ws + travel_tail_offset(d));
	const unsigned blocks = blocks_for(d.tile_count, kThreads / 64, kTravelMaxWaves / (kThreads / 64));
	for (uint32_t k = first_round; k < first_round + rounds; ++k)
		hipLaunchKernelGGL(water_relax, dim3(blocks), dim3(kThreads), 0, stream, field, static_cast<const uint8_t*>(ws), stamps,
						   reinterpret_cast<const uint32_t*>(ws + travel_list_offset(d, k & 1u)), reinterpret_cast<uint32_t*>(ws + travel_list_offset(d, (k + 1u) & 1u)), tail, k, d);
}

void launch_water_finish(const TravelDims& d, const uint32_t* field, void* result, void* workspace, hipStream_t stream) {
	uint8_t* ws = static_cast<uint8_t*>(workspace);
	unsigned long long* tail = reinterpret_cast<unsigned long long*>(ws + travel_tail_offset(d));
	hipLaunchKernelGGL(water_finish, dim3(blocks_for(d.tile_count, kThreads / 64, kStreamBlocks)), dim3(kThreads), 0, stream, field, static_cast<const uint8_t*>(ws), tail, d);
	hipLaunchKernelGGL(water_record_out, dim3(1), dim3(64), 0, stream, reinterpret_cast<const uint64_t*>(tail), static_cast<uint64_t*>(result));
}

void launch_water_mask(const int32_t extent[3], const uint32_t* field, uint32_t min_depth, uint8_t* mask, hipStream_t stream) {
	const uint32_t slice = static_cast<uint32_t>(extent[0]) * static_cast<uint32_t>(extent[1]);
	hipLaunchKernelGGL(water_mask, dim3(blocks_for(slice, kThreads, 256), static_cast<unsigned>(extent[2])), dim3(kThreads), 0, stream, field, slice, min_depth, mask);
}

} // namespace bm
