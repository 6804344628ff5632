// read_book.h -- what a read of the world decides before it touches the device.  Host only, no HIP: world_reads.h owns the buffers, the events
// and the calls.  Here is every decision of the five calls that only read the world, once: the boxes of a box outside its clipped part and
// where they lie in the caller's volume, what the label calls refuse about their box and what label.hip is told about it, which bricks of a
// box the device does not hold and how they are listed for it (PatchList), what the two queries refuse and the LoD cell of an origin, what a
// scratch that is too small grows to, and what label_region has clocked.  tests/read_book_check.cpp scripts it on the CPU.
//
// Which read is a frame (FrameOrder::begin ... end around it, so that uploads and changes wait for it) and which Turn it takes:
//   read_region       a frame   the patch list's (when bricks are absent)
//   label_region      a frame   the labels', and the patch list's when bricks are absent
//   cast_rays         a frame   a slot of the ticket ring
//   query_volumes     a frame   the volume scratch's
//   label_components  --        the labels'   (they read the caller's label volume alone)
//   label_mask        --        the labels'
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "buffer_checks.h"
#include "change_book.h" // the kClocked* flags
#include "label.h"
#include "pool_book.h"
#include "world.h"

namespace bm {

// ---- outside slabs and offsets
// the parts of the box [blo, bhi) that lie outside its clipped part [lo, hi) (all of it when `inside` is false), as up to six boxes:
// f(x0, x1, y0, y1, z0, z1), none of them empty unless the box is
template <class F> void outside_slabs(const int32_t blo[3], const int32_t bhi[3], bool inside, const int lo[3], const int hi[3], F f) {
	if (!inside) { f(blo[0], bhi[0], blo[1], bhi[1], blo[2], bhi[2]); return; }
	if (blo[2] < lo[2]) f(blo[0], bhi[0], blo[1], bhi[1], blo[2], lo[2]);
	if (hi[2] < bhi[2]) f(blo[0], bhi[0], blo[1], bhi[1], hi[2], bhi[2]);
	if (blo[1] < lo[1]) f(blo[0], bhi[0], blo[1], lo[1], lo[2], hi[2]);
	if (hi[1] < bhi[1]) f(blo[0], bhi[0], hi[1], bhi[1], lo[2], hi[2]);
	if (blo[0] < lo[0]) f(blo[0], lo[0], lo[1], hi[1], lo[2], hi[2]);
	if (hi[0] < bhi[0]) f(hi[0], bhi[0], lo[1], hi[1], lo[2], hi[2]);
}
// the byte of world voxel (x, y, z) in the region's volume
inline int64_t region_offset(const bm_region& r, int64_t x, int64_t y, int64_t z) { return (z - r.lo[2]) * r.slice_pitch + (y - r.lo[1]) * r.row_pitch + (x - r.lo[0]); }
// ... and in the tight 4-byte volume of a label box: its pitches in bytes, and the first byte of the voxel's word
struct LabelPitch {
	int64_t row, slice;
	explicit LabelPitch(const LabelDims& d) : row(static_cast<int64_t>(d.nx) * 4), slice(row * d.ny) {}
	int64_t offset(const LabelDims& d, int64_t x, int64_t y, int64_t z) const { return (z - d.org[2]) * slice + (y - d.org[1]) * row + (x - d.org[0]) * 4; }
};

// ---- the label box
// What the three label calls refuse about their box, before anything is launched: the reason, or null -- then *d has the box's dimensions
// and *empty says whether it holds no voxel.
inline const char* check_label_box(const int32_t lo[3], const int32_t hi[3], int supergrid_xy, LabelDims* d, bool* empty) {
	if (!lo || !hi) return "null box";
	int64_t n[3];
	for (int k = 0; k < 3; ++k) {
		n[k] = static_cast<int64_t>(hi[k]) - lo[k];
		if (n[k] < 0) return "hi < lo";
	}
	*empty = n[0] == 0 || n[1] == 0 || n[2] == 0;
	// (64 bits: each factor is below 2^32, so the first product is below 2^63 once n[0] has passed, and the second is formed only below 2^31 * 2^32)
	if (!*empty && (n[0] > kLabelMaxVoxels || n[0] * n[1] > kLabelMaxVoxels || n[0] * n[1] * n[2] > kLabelMaxVoxels)) return "the box holds more than 2^31 - 2 voxels";
	*d = LabelDims{};
	for (int k = 0; k < 3; ++k) d->org[k] = lo[k];
	d->nx = static_cast<uint32_t>(n[0]); d->ny = static_cast<uint32_t>(n[1]); d->nz = static_cast<uint32_t>(n[2]);
	d->sg_xy = static_cast<uint32_t>(supergrid_xy);
	d->sg_xy2 = d->sg_xy * d->sg_xy;
	return nullptr;
}
// the box clipped to the world, as World::region_bounds gives it, and the cells it overlaps; false: nothing of it lies inside
inline bool label_clip(const WorldDims& wd, const int32_t lo[3], const int32_t hi[3], LabelDims* d) {
	bm_region r{};
	for (int k = 0; k < 3; ++k) { r.lo[k] = lo[k]; r.hi[k] = hi[k]; }
	int clo[3] = {0, 0, 0}, chi[3] = {0, 0, 0};
	const bool inside = World::region_bounds(wd, r, clo, chi);
	for (int k = 0; k < 3; ++k) {
		d->lo[k] = inside ? clo[k] : 0;
		d->hi[k] = inside ? chi[k] : 0;
		d->c0[k] = inside ? clo[k] >> 3 : 0;
		d->nc[k] = inside ? ((chi[k] - 1) >> 3) - d->c0[k] + 1 : 0;
	}
	return inside;
}

// ---- a scratch or staging buffer of these calls starts at 64 KiB; one that is too small for `bytes` grows to exactly that
constexpr size_t kScratchStart = size_t{1} << 16;
inline size_t scratch_grown(size_t bytes) { return std::max(bytes, kScratchStart); }

// ---- the patch list: the cells of a clipped box whose bricks the device does not hold (a streaming scene), with those bricks from the host
// world, as region.hip and label.hip take them: [cells: 3 ints each][bricks], the bricks on a 64-byte line.  76 bytes a brick: 862 fit 64 KiB.
struct PatchList {
	std::vector<int> cells;
	std::vector<Brick> bricks;
	// where the sections of a list of n bricks lie
	struct Layout {
		size_t n, o_bricks, bytes;
		explicit Layout(size_t n_) : n(n_), o_bricks((n_ * 3 * sizeof(int) + 63) / 64 * 64), bytes(o_bricks + n_ * sizeof(Brick)) {}
	};
	Layout layout() const { return Layout(bricks.size()); }
	// the box [lo, hi) (world voxels, inside the world, not empty; not read unless `inside`), cells in x-fastest order.  A preloaded scene
	// holds every brick: none.
	PatchList(const World& world, const PoolBook& book, bool inside, const int lo[3], const int hi[3]) {
		if (!inside || book.preloaded()) return;
		const WorldDims& d = world.dims;
		for (int cz = lo[2] >> 3; cz <= (hi[2] - 1) >> 3; ++cz)
			for (int cy = lo[1] >> 3; cy <= (hi[1] - 1) >> 3; ++cy)
				for (int cx = lo[0] >> 3; cx <= (hi[0] - 1) >> 3; ++cx) {
					const int sci = d.supercell_id(cx / kSupercell, cy / kSupercell, cz / kSupercell);
					const HostSupercell& c = world.supercells[sci];
					const uint32_t word = c.indices[cell_local_index(cx, cy, cz)];
					if (!book.absent(sci, word)) continue;
					cells.insert(cells.end(), {cx, cy, cz});
					bricks.push_back(c.bricks[word & BM_BRICK_INDEX_BITS]);
				}
	}
	void fill(char* dst) const { // layout().bytes bytes; the padding between the sections is left as it is
		const Layout at = layout();
		if (at.n == 0) return;
		std::memcpy(dst, cells.data(), at.n * 3 * sizeof(int));
		std::memcpy(dst + at.o_bricks, bricks.data(), at.n * sizeof(Brick));
	}
};

// ---- query arguments: what the two queries refuse before they touch the device, in this order -- the message, or null.  *nothing: n == 0,
// the call has succeeded and launches nothing (what follows n in the order is not looked at then).
inline bool lod_origin_ok(float v) { return std::fabs(v) < 16777216.f; } // finite and below 2^24: its cell is an int
inline int lod_cell(float v) { return static_cast<int>(v / 8.f); }       // as fill_frame_constants: ivec3(camera.position / 8.f) (no contraction: one division)
// campos: the LoD centre in brick cells, (0, 0, 0) without BM_QUERY_LOD
inline const char* check_cast_rays(int64_t n, const void* rays, const void* hits, uint32_t flags, const float* lod_origin, int campos[3], bool* nothing) {
	*nothing = false;
	if (flags & ~(BM_QUERY_LOD | BM_QUERY_NO_REQUESTS)) return "bm_scene_cast_rays: unknown flag";
	if (n < 0 || n > (int64_t{1} << 28)) return "bm_scene_cast_rays: n must be 0 ... 2^28";
	if (n == 0) { *nothing = true; return nullptr; }
	if (!rays || !hits) return "bm_scene_cast_rays: null ray or hit buffer";
	campos[0] = campos[1] = campos[2] = 0;
	if (flags & BM_QUERY_LOD) {
		if (!lod_origin) return "bm_scene_cast_rays: BM_QUERY_LOD needs lod_origin";
		for (int i = 0; i < 3; ++i) {
			if (!lod_origin_ok(lod_origin[i])) return "bm_scene_cast_rays: lod_origin must be finite and below 2^24";
			campos[i] = lod_cell(lod_origin[i]);
		}
	}
	return nullptr;
}
inline const char* check_query_volumes(int64_t n, const void* volumes, const void* results, uint32_t flags, bool* nothing) {
	*nothing = false;
	if (flags & ~BM_VOLUME_ANY) return "bm_scene_query_volumes: unknown flag";
	if (n < 0 || n > (int64_t{1} << 24)) return "bm_scene_query_volumes: n must be 0 ... 2^24";
	if (n == 0) { *nothing = true; return nullptr; }
	if (!volumes || !results) return "bm_scene_query_volumes: null volume or result buffer";
	if (!aligned(volumes, 4) || !aligned(results, 8)) return "bm_scene_query_volumes: volumes must be 4-byte aligned, results 8-byte aligned";
	return nullptr;
}

// ---- the stage clock of label_region (marks 0 ... 3 around local, merge and flatten; the flags: change_book.h).  A call that launches nothing
// -- an empty box, or one wholly outside the world -- records nothing, and the times of the call before it are not its own: nothing to report.
struct LabelClock {
	unsigned clocked = 0;
	void begun() { clocked = 0; }               // a call is being issued
	void launched() { clocked = kClockedCall; } // ... and part of its box lies inside the world: the kernels are queued
	const char* refused() const { return clocked ? nullptr : "the last bm_scene_label_region launched nothing, or there was none"; } // what last_label_ms answers: null = the times
};

} // namespace bm
