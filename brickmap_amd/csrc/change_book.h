// change_book.h -- what a change of the host world sends to the device.  Host only, no HIP: world_changes.h owns the buffers, the events and
// the calls.  Here is every decision of a batch, once: which supercells a box reaches, which device word, arena slot and brick a touched cell
// sends and the two boxes the walk fields hear of (CellBatch), where the sections of the staging buffer lie (StagingLayout), a region's
// dimensions for region.hip, and which stages a call has clocked with what last_edit_ms / last_region_ms answer from them.
// tests/change_book_check.cpp scripts it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pool_book.h"
#include "world.h"

namespace bm {

// the cells a change of the world touched, collected while it is staged
struct FieldChange {
	int box_lo[3] = {1 << 30, 1 << 30, 1 << 30}, box_hi[3] = {-1, -1, -1}; // cells whose occupancy changed (unbordered, inclusive)
	int touch_lo[2] = {1 << 30, 1 << 30}, touch_hi[2] = {-1, -1};          // columns of every touched cell (x, y): what the shadow heights scan again
	bool occupancy() const { return box_hi[0] >= 0; }
	static FieldChange whole(const WorldDims& d) { // a new world
		FieldChange c;
		for (int k = 0; k < 3; ++k) { c.box_lo[k] = 0; c.box_hi[k] = (k == 2 ? d.cells_height : d.cells) - 1; }
		for (int k = 0; k < 2; ++k) { c.touch_lo[k] = 0; c.touch_hi[k] = d.cells - 1; }
		return c;
	}
};

// the supercells that hold a voxel of the box [lo, hi) (world voxels, inside the world, not empty), appended in ascending id order
inline void supercells_reached(const WorldDims& d, const int lo[3], const int hi[3], std::vector<int>* out) {
	for (int sz = lo[2] / kColumnSpan; sz <= (hi[2] - 1) / kColumnSpan; ++sz)
		for (int sy = lo[1] / kColumnSpan; sy <= (hi[1] - 1) / kColumnSpan; ++sy)
			for (int sx = lo[0] / kColumnSpan; sx <= (hi[0] - 1) / kColumnSpan; ++sx) out->push_back(d.supercell_id(sx, sy, sz));
}

// what region.hip is told about the region r whose box, clipped to the world, is [lo, hi)
inline RegionDims region_dims(const WorldDims& d, const bm_region& r, const int lo[3], const int hi[3]) {
	RegionDims rd{};
	for (int k = 0; k < 3; ++k) {
		rd.lo[k] = lo[k]; rd.hi[k] = hi[k]; rd.org[k] = r.lo[k];
		rd.c0[k] = lo[k] >> 3;
		rd.nc[k] = ((hi[k] - 1) >> 3) - rd.c0[k] + 1;
	}
	rd.g0 = rd.c0[0] >> 4;
	rd.sg_xy = static_cast<uint32_t>(d.supergrid_xy);
	rd.sg_xy2 = rd.sg_xy * rd.sg_xy;
	rd.row_pitch = r.row_pitch;
	rd.slice_pitch = r.slice_pitch;
	return rd;
}

// Stage clocks: the stages a call has recorded.  0 = the call has nothing to report.
enum : unsigned { kClockedCall = 1, kClockedPack = 2, kClockedScatter = 4, kClockedField = 8 };

// The touched cells of every supercell a change reached, as the scatter kernel of edit.hip takes them (the batch's pool moves: PoolBook::moves).
struct CellBatch {
	std::vector<uint32_t> cells, words, slots; // index of the cell's word in the index grid / its new device word / the arena slot of its brick, 0xFFFFFFFF: none is written
	std::vector<Brick> bricks;
	FieldChange change;
	unsigned clocked() const { return cells.empty() ? 0u : change.occupancy() ? kClockedScatter | kClockedField : kClockedScatter; } // the stages its submission records
	// The touched cells of supercell `sci`, whose host world has just changed (old_words = its index words before) and whose pool has been
	// rebound (PoolBook::rebind): slot | loaded | lod for a resident brick, which keeps its pool slot and gets its new content; unloaded | lod
	// for a brick that is not resident; 0 for an empty cell.
	void add_supercell(const WorldDims& d, int sci, const HostSupercell& c, const std::vector<uint32_t>& old_words, const uint8_t* touched, const PoolBook::Pool& pool) {
		int s[3];
		d.supercell_coords(sci, &s[0], &s[1], &s[2]);
		for (int j = 0; j < kCellsPerSupercell; ++j) {
			if (!touched[j]) continue;
			const uint32_t ow = old_words[j], nw = c.indices[j];
			const int g[3] = {s[0] * kSupercell + (j & 15), s[1] * kSupercell + ((j >> 4) & 15), s[2] * kSupercell + (j >> 8)};
			for (int k = 0; k < 2; ++k) { change.touch_lo[k] = std::min(change.touch_lo[k], g[k]); change.touch_hi[k] = std::max(change.touch_hi[k], g[k]); }
			if ((ow != 0) != (nw != 0))
				for (int k = 0; k < 3; ++k) { change.box_lo[k] = std::min(change.box_lo[k], g[k]); change.box_hi[k] = std::max(change.box_hi[k], g[k]); }
			const uint16_t ds = nw ? pool.dev_slot[nw & BM_BRICK_INDEX_BITS] : kNoDeviceSlot;
			cells.push_back(static_cast<uint32_t>(sci) * kCellsPerSupercell + static_cast<uint32_t>(j));
			words.push_back(PoolBook::device_word(nw, ds));
			slots.push_back(ds == kNoDeviceSlot ? 0xFFFFFFFFu : pool.base + ds);
			bricks.push_back(nw ? c.bricks[nw & BM_BRICK_INDEX_BITS] : Brick{});
		}
	}
};

// The staging buffer of a batch of n cells and `moves` pool moves: [pool moves][cells][words][slots][bricks], sections 64-byte aligned
struct StagingLayout {
	size_t o_cells, o_words, o_slots, o_bricks, bytes;
	StagingLayout(size_t moves, size_t n) {
		auto up = [](size_t v) { return (v + 63) / 64 * 64; };
		o_cells = up(moves * sizeof(PoolMove));
		o_words = o_cells + up(n * 4);
		o_slots = o_words + up(n * 4);
		o_bricks = o_slots + up(n * 4);
		bytes = o_bricks + n * sizeof(Brick);
	}
	static size_t grown(size_t bytes) { return std::max<size_t>(bytes * 2, 1 << 16); } // what a staging too small for `bytes` grows to
	void fill(char* dst, const std::vector<PoolMove>& moves, const CellBatch& b) const {
		const size_t n = b.cells.size();
		if (!moves.empty()) std::memcpy(dst, moves.data(), moves.size() * sizeof(PoolMove));
		if (n == 0) return;
		std::memcpy(dst + o_cells, b.cells.data(), n * 4);
		std::memcpy(dst + o_words, b.words.data(), n * 4);
		std::memcpy(dst + o_slots, b.slots.data(), n * 4);
		std::memcpy(dst + o_bricks, b.bricks.data(), n * sizeof(Brick));
	}
};

// ---- the stage-clock rules.  An edit records marks 0 ... 2 around scatter and field; a batch that scatters nothing leaves the last one's flags,
// and with them its times, readable.  A region write: marks 0 ... 2 around pack and copy (a device volume), 3 ... 5 around scatter and field.
inline unsigned edit_clocked(unsigned last, unsigned batch) { return batch ? batch : last; }
inline unsigned region_clocked(bool device_volume, unsigned batch) { return kClockedCall | (device_volume ? kClockedPack : 0u) | batch; }
// what last_edit_ms answers from the times between its marks (ms[2]) ...
inline void edit_ms(unsigned clocked, const float ms[2], float* scatter_ms, float* field_ms) {
	*scatter_ms = ms[0];
	*field_ms = (clocked & kClockedField) ? ms[1] : 0.0f;
}
// ... and last_region_ms (ms[0], ms[1]: marks 0 ... 2, read where kClockedPack is set; ms[2], ms[3]: marks 3 ... 5, read where kClockedScatter is)
inline void region_ms(unsigned clocked, const float ms[4], float* pack_ms, float* copy_ms, float* scatter_ms, float* field_ms) {
	*pack_ms = (clocked & kClockedPack) ? ms[0] : 0.0f;
	*copy_ms = (clocked & kClockedPack) ? ms[1] : 0.0f;
	*scatter_ms = (clocked & kClockedScatter) ? ms[2] : 0.0f;
	*field_ms = (clocked & kClockedField) ? ms[3] : 0.0f;
}

} // namespace bm
