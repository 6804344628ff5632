// tile_lists.h -- what the kernels of travel.hip and water.hip share on the device beside the rules of travel.h: the place of a tile,
// and how a tile gets onto a round's work list exactly once (the stamp rule).
#pragma once
#include <hip/hip_runtime.h>

#include "global_mem.h"
#include "travel.h"

namespace bm {

__device__ __forceinline__ uint32_t stamp_max(uint32_t* stamps, uint32_t tile, uint32_t v) {
	return __hip_atomic_fetch_max((g_u32*)stamps + tile, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t word_add(uint32_t* words, uint32_t i, uint32_t v) {
	return __hip_atomic_fetch_add((g_u32*)words + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// `tile` goes onto `list` (whose count is word `count_word` of the tail) unless its stamp says it is there already.  A tile is listed
// once per round, so the slot is below `tiles`, the list's size; the comparison keeps a store inside the list whatever the tail held.
__device__ __forceinline__ void list_tile(uint32_t* stamps, uint32_t* list, uint32_t* tail, uint32_t count_word, uint32_t tile, uint32_t round, uint32_t tiles) {
	if (stamp_max(stamps, tile, round) < round) {
		const uint32_t slot = word_add(tail, count_word, 1u);
		if (slot < tiles) st32(list, slot, tile);
	}
}

struct TilePlace {
	uint32_t tx, ty, tz;
};
__device__ __forceinline__ TilePlace tile_place(const TravelDims& d, uint32_t tile) {
	const uint32_t q = tile / d.tiles[0];
	return {tile - q * d.tiles[0], q % d.tiles[1], q / d.tiles[1]};
}

} // namespace bm
