// distance.h -- the rules of the distance field (bm_distance_field, bm_distance_mask, include/brickmap.h), written once for the kernels
// of distance.hip and the plain loops of distance_host.cpp.  Needs no HIP header: tests/distance_check.cpp builds it with a host compiler.
//
// All integers.  D(p) = the minimum over the sources q of |p - q|^2 separates by axis: along x it is the square of the distance to the
// nearest source of the row (f), and along y and then z a line of values f(j) becomes min over j of f(j) + (u - j)^2 -- the lower envelope
// of the parabolas that stand on the sites j with f(j) != none.  The envelope is kept as a stack of (site, start) pairs: the parabola of
// `site` is the lowest one from `start` up to the start of the entry above it.  What the kernels add to that is the layout of a lane's
// stack in the workspace ([entry][line]) and keeping the top entry in registers; both are here (LineTop and the three accessors the
// functions take), so that the check program can walk a volume lane by lane without a device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "device_types.h"

namespace bm {

constexpr uint32_t kDistanceToEmpty = 1, kDistanceOutside = 2; // BM_DISTANCE_TO_EMPTY, BM_DISTANCE_OUTSIDE
constexpr uint32_t kDistanceMaskAbove = 1;                     // BM_DISTANCE_MASK_ABOVE
constexpr uint32_t kDistanceNone = 0x7FFFFFFFu;                // BM_DISTANCE_NONE
constexpr int kDistanceMaxExtent = 16384;                      // the limits of bm_mesh_params
constexpr int64_t kDistanceMaxVoxels = (int64_t{1} << 31) - 2;
constexpr size_t kDistanceTailBytes = 32;                      // the workspace's last bytes: the max key and the source count, 8 bytes each

struct DistanceParamsView {
	int32_t extent[3];
	int64_t row_pitch, slice_pitch;
	uint32_t flags, reserved;
};

// the view of a bm_distance_params (a template, so that this header needs no other)
template <class P>
inline DistanceParamsView distance_params_view(const P& p) {
	return {{p.extent[0], p.extent[1], p.extent[2]}, p.row_pitch, p.slice_pitch, p.flags, p.reserved};
}

// null, or why bm_distance_field and bm_host_distance_field refuse these parameters (pitches as given: 0 = tight)
inline const char* distance_params_problem(const DistanceParamsView& p) {
	if (p.flags & ~(kDistanceToEmpty | kDistanceOutside)) return "unknown flag";
	if (p.reserved != 0) return "reserved is not 0";
	for (int k = 0; k < 3; ++k)
		if (p.extent[k] < 1 || p.extent[k] > kDistanceMaxExtent) return "an extent below 1 or above 16384";
	if (static_cast<int64_t>(p.extent[0]) * p.extent[1] > kDistanceMaxVoxels / p.extent[2]) return "more than 2^31 - 2 voxels";
	if (p.row_pitch < 0 || p.slice_pitch < 0) return "negative pitch";
	if (p.row_pitch > (int64_t{1} << 40)) return "row_pitch above 2^40";
	const int64_t row = p.row_pitch ? p.row_pitch : p.extent[0];
	if (row < p.extent[0]) return "row_pitch below the extent along x";
	if (p.slice_pitch && p.slice_pitch / p.extent[1] < row) return "slice_pitch below row_pitch * the extent along y";
	if ((p.slice_pitch ? p.slice_pitch : row * p.extent[1]) > (int64_t{1} << 46) / p.extent[2]) return "a volume spanning more than 2^46 bytes";
	return nullptr;
}

// what the kernels and the loops need of the parameters
struct DistanceDims {
	int32_t extent[3];
	uint32_t to_empty, outside;
	uint32_t voxels;                // below 2^31 - 1
	int64_t row_pitch, slice_pitch; // resolved: never 0
};

inline DistanceDims distance_dims(const DistanceParamsView& p) {
	DistanceDims d;
	for (int k = 0; k < 3; ++k) d.extent[k] = p.extent[k];
	d.to_empty = (p.flags & kDistanceToEmpty) ? 1u : 0u;
	d.outside = (p.flags & kDistanceOutside) ? 1u : 0u;
	d.voxels = static_cast<uint32_t>(static_cast<int64_t>(p.extent[0]) * p.extent[1] * p.extent[2]);
	d.row_pitch = p.row_pitch ? p.row_pitch : p.extent[0];
	d.slice_pitch = p.slice_pitch ? p.slice_pitch : d.row_pitch * p.extent[1];
	return d;
}

// bytes from the volume's first byte to one past its last
inline uint64_t distance_span(const DistanceDims& d) {
	return static_cast<uint64_t>(d.extent[2] - 1) * static_cast<uint64_t>(d.slice_pitch) + static_cast<uint64_t>(d.extent[1] - 1) * static_cast<uint64_t>(d.row_pitch) +
		   static_cast<uint64_t>(d.extent[0]);
}

// workspace: the plane h between the two line passes, 4 bytes per voxel; the lanes' stacks, 4 bytes per voxel; each rounded up to 16
// bytes; then the tail (max key, source count, 16 bytes that stay 0)
inline size_t distance_plane_bytes(const DistanceDims& d) { return (static_cast<size_t>(d.voxels) * 4 + 15) & ~static_cast<size_t>(15); }
inline size_t distance_workspace_bytes(const DistanceDims& d) { return 2 * distance_plane_bytes(d) + kDistanceTailBytes; }

// ---- the x pass: a voxel's byte -> is it a source
BM_VHD bool distance_is_source(uint32_t byte, uint32_t to_empty) { return (byte != 0) != (to_empty != 0); }
// the square of a distance along one axis (at most 16383), or none
BM_VHD uint32_t distance_sq(int32_t g) { return static_cast<uint32_t>(g) * static_cast<uint32_t>(g); }

// A row is walked in chunks of 64 voxels (a row of 32 or fewer is one chunk of S = the power of two that holds it).  The lane at place
// l of a chunk whose sources are the bits of m, standing for voxel x: the distance to the nearest source -- inside the chunk the highest
// bit at or below l and the lowest at or above it, else `left`, the last source before the chunk, and `ahead`, the first one after it
// (-1: none) -- or kDistanceMaxExtent when the row has none.
BM_VHD int32_t distance_chunk_nearest(uint64_t m, uint32_t l, int32_t x, int32_t left, int32_t ahead) {
	const uint64_t upto = m & ((uint64_t{2} << l) - 1u), from = m >> l;
	int32_t g = kDistanceMaxExtent, r = kDistanceMaxExtent;
	if (upto != 0)
		g = static_cast<int32_t>(l) - (63 - __builtin_clzll(upto));
	else if (left >= 0)
		g = x - left;
	if (from != 0)
		r = __builtin_ctzll(from);
	else if (ahead >= 0)
		r = ahead - x;
	return r < g ? r : g;
}
// the lanes a row gets, as a shift: 6 for rows above 32 voxels
inline uint32_t distance_row_shift(int32_t nx) {
	uint32_t shift = 6;
	if (nx <= 32) {
		shift = 0;
		while ((1 << shift) < nx) ++shift;
	}
	return shift;
}

// ---- a line pass: values f(0 ... n - 1), each none or below 2^29 (one or two squares of at most 16383), n at most 16384
// the top entry of a line's stack, and how many entries the stack holds (the others are where the accessors keep them)
struct LineTop {
	uint32_t count, site, start, f;
};

// an entry as the stacks hold it: two 16-bit halves
BM_VHD uint32_t distance_line_pack(uint32_t site, uint32_t start) { return site | start << 16; }

// drops the top entry; the one below comes back from the stack (load_entry(k): entry k as packed) and its value from the line (f_at(site))
template <class LoadEntry, class FAt>
BM_VHD void distance_line_pop(LineTop& t, LoadEntry&& load_entry, FAt&& f_at) {
	--t.count;
	if (t.count > 0) {
		const uint32_t e = load_entry(t.count - 1);
		t.site = e & 0xFFFFu;
		t.start = e >> 16;
		t.f = f_at(t.site);
	}
}

// Site u (above every site so far) with value fu != none joins the envelope of a line of n values: the tops it beats at their own start
// go; against the top i that stays, it is the lower one from 1 + floor((u^2 - i^2 + f(u) - f(i)) / (2 (u - i))) on, and it is dropped
// when that is n or more.  (The top that stays is not beaten at its start t >= 0, which says numerator >= 2 t (u - i) >= 0; it is below
// 2^28 + 2^29, so the 64-bit numerator divides as a 32-bit one.  Sums of a value and a square stay below 2^29 + 2^28 as well.)
template <class LoadEntry, class StoreEntry, class FAt>
BM_VHD void distance_line_push(LineTop& t, uint32_t u, uint32_t fu, uint32_t n, LoadEntry&& load_entry, StoreEntry&& store_entry, FAt&& f_at) {
	while (t.count > 0) {
		const uint32_t di = t.start - t.site, du = u - t.start; // (di may wrap: its square does not care)
		if (t.f + di * di > fu + du * du)
			distance_line_pop(t, load_entry, f_at);
		else
			break;
	}
	if (t.count == 0) {
		t = {1u, u, 0u, fu};
		return;
	}
	const int64_t num = static_cast<int64_t>(u) * u - static_cast<int64_t>(t.site) * t.site + static_cast<int64_t>(fu) - static_cast<int64_t>(t.f);
	const uint32_t start = 1u + static_cast<uint32_t>(num) / (2u * (u - t.site));
	if (start >= n) return;
	store_entry(t.count - 1, distance_line_pack(t.site, t.start));
	t = {t.count + 1, u, start, fu};
}

// the envelope's value at u, for u going down from n - 1 to 0: entries that start above u go first.  none for a line without a site.
template <class LoadEntry, class FAt>
BM_VHD uint32_t distance_line_emit(LineTop& t, uint32_t u, LoadEntry&& load_entry, FAt&& f_at) {
	if (t.count == 0) return kDistanceNone;
	while (t.start > u) distance_line_pop(t, load_entry, f_at); // (entry 0 starts at 0: the stack never empties here)
	const uint32_t du = u - t.site;
	return t.f + du * du;
}

// ---- the last pass
// BM_DISTANCE_OUTSIDE: m^2, m = the least over the axes of min(i + 1, n - i)
BM_VHD uint32_t distance_outside_sq(const int32_t extent[3], int32_t x, int32_t y, int32_t z) {
	int32_t m = x + 1 < extent[0] - x ? x + 1 : extent[0] - x;
	const int32_t my = y + 1 < extent[1] - y ? y + 1 : extent[1] - y, mz = z + 1 < extent[2] - z ? z + 1 : extent[2] - z;
	m = my < m ? my : m;
	m = mz < m ? mz : m;
	return distance_sq(m);
}

// the key whose maximum names the largest finite value and, among its voxels, the lowest index; 0 (no voxel gives it) for none
BM_VHD uint64_t distance_max_key(uint32_t value, uint32_t index) {
	return value == kDistanceNone ? 0u : (static_cast<uint64_t>(value) << 32 | (0xFFFFFFFFu - index));
}

// the 32 bytes of a bm_distance_result from the key's maximum and the source count
struct DistanceRecord {
	uint64_t sources;
	uint32_t max_sq, reserved0;
	uint64_t max_at, reserved1;
};
BM_VHD DistanceRecord distance_record(uint64_t key, uint64_t sources) {
	if (key == 0) return {sources, kDistanceNone, 0u, 0u, 0u};
	return {sources, static_cast<uint32_t>(key >> 32), 0u, static_cast<uint64_t>(0xFFFFFFFFu - static_cast<uint32_t>(key)), 0u};
}

// ---- the mask: BM_DISTANCE_NONE is above every limit
BM_VHD uint32_t distance_mask_byte(uint32_t value, uint32_t limit_sq, uint32_t above) {
	const bool within = value != kDistanceNone && value <= limit_sq;
	return within != (above != 0) ? 1u : 0u;
}

} // namespace bm
