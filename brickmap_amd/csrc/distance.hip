// distance.hip -- the exact squared Euclidean distance field of a byte volume on the device (bm_distance_field, bm_distance_mask), by the
// rules of distance.h.  Three line passes, one kernel each, and a finishing thread:
//
//   x      : a wave walks a row in chunks of 64 voxels (rows of 32 voxels or fewer: 64 / S rows per wave, S = the power of two that holds a
//            row).  The chunk's bytes come in as aligned words where all four bytes are voxels of the row and as single bytes otherwise,
//            through the chunk's first 17 lanes; a shuffle hands every lane its voxel's bit and one ballot gives the chunk's source mask.
//            A lane's nearest source inside the chunk is a leading or trailing zero count of the masked ballot; the nearest one to the left
//            of the chunk is carried in a scalar; the nearest one to the right comes from looking ahead, chunk by chunk, and that is
//            carried too, with the mask of the chunk it was found in -- every chunk is read once.  f = g^2 (or none) goes to the output field, the ballots' population counts
//            to the workspace's source count with one 64-bit add per wave.
//   line   : once along y (field -> the workspace's plane h) and once along z (h -> field): one lane per line, adjacent lanes adjacent in
//            x.  The lower envelope of distance.h, its stack in the workspace as [entry][line] with the top entry in registers; then the
//            sweep back writes the values.  The z pass takes the minimum with BM_DISTANCE_OUTSIDE's term and feeds the max key: a lane's
//            own maximum, a butterfly over the wave, one 64-bit atomic max per wave.
//   finish : one thread turns the key and the count into the result record.
//   mask   : one lane per four bytes of the output, an aligned word where all four are voxels.
//
// Every loop is bounded by an extent (the look-ahead by the row's chunks, pushes and pops by the line's sites); nothing waits for another
// workgroup; the atomics are the count and the key; nothing is read in the kernel that wrote it, except a lane's own stack entries.
#include <hip/hip_runtime.h>

#include "distance.h"
#include "global_mem.h"
#include "kernels.h"

namespace bm {

namespace {

constexpr int kThreads = 256;
constexpr uint64_t kRowBlocks = 2048; // the x pass's grid at most: eight workgroups for each of 256 compute units

typedef __attribute__((address_space(1))) unsigned long long g_ull;

// the four bytes of a word -> bit k: byte k is not 0
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) {
	const uint32_t nz = ((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u) >> 7;
	return ((nz * 0x00204081u) >> 21) & 15u;
}

// The ballot of "my voxel is a source" over the wave for one chunk of every segment: the lane at place l of its segment stands for voxel
// c0 + l of the row that begins at byte `at` (rows past the last: live = false, no load).  lanes l < words load: word k holds the voxels
// c0 - lead + 4 k ... + 3, lead = the chunk's first byte's address modulo 4.
__device__ __forceinline__ uint64_t chunk_sources(const uint8_t* __restrict__ volume, int64_t at, bool live, int32_t c0, int32_t nx, uint32_t lane, uint32_t l, uint32_t words,
												  uint32_t to_empty) {
	const uint32_t lead = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(volume) + static_cast<uintptr_t>(at + c0)) & 3u);
	uint32_t four = 0;
	if (live && l < words) {
		const int32_t xw = c0 - static_cast<int32_t>(lead) + 4 * static_cast<int32_t>(l); // the voxel of the word's first byte
		if (xw >= 0 && xw + 4 <= nx) {
			four = nonzero_bytes(*(const g_u32*)((const g_u8*)volume + (at + xw)));
		} else {
#pragma unroll
			for (int b = 0; b < 4; ++b) {
				const int32_t x = xw + b;
				if (x >= c0 && x < nx && ld8(volume, static_cast<size_t>(at + x)) != 0) four |= 1u << b;
			}
		}
	}
	const uint32_t from = l + lead; // my byte among the chunk's words
	const uint32_t got = static_cast<uint32_t>(__shfl(static_cast<int>(four), static_cast<int>(lane - l + (from >> 2)), 64));
	const bool solid = ((got >> (from & 3u)) & 1u) != 0;
	return __ballot(live && c0 + static_cast<int32_t>(l) < nx && solid != (to_empty != 0));
}

} // namespace

// field[row * nx + x] = the square of the distance from x to the nearest source of the row, or none; *sources += the sources of all rows.
// shift: log2 of S, the lanes a row gets (6: a whole wave, and then the row is walked in chunks); turns: the rows / (64 / S), rounded up
__global__ __launch_bounds__(kThreads) void distance_x(const uint8_t* __restrict__ volume, uint32_t* __restrict__ field, unsigned long long* __restrict__ sources,
													   const DistanceDims d, const uint32_t shift, const uint32_t turns) {
	const uint32_t lane = threadIdx.x & 63u, S = 1u << shift, l = lane & (S - 1u), seg = lane >> shift;
	const uint32_t wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
	const uint32_t rows = static_cast<uint32_t>(d.extent[1]) * static_cast<uint32_t>(d.extent[2]);
	const int32_t nx = d.extent[0];
	const uint32_t words = (S + 6u) >> 2; // the words that hold S bytes wherever they begin
	uint64_t count = 0;
	// a wave takes turn after turn -- 64 / S rows each -- so that the grid, and with it the adds to the one count, stays bounded
	for (uint32_t turn = wave; turn < turns; turn += gridDim.x * (kThreads / 64)) {
		const uint64_t row64 = (static_cast<uint64_t>(turn) << (6u - shift)) + seg;
		const bool live = row64 < rows;
		const uint32_t row = live ? static_cast<uint32_t>(row64) : 0u;
		const uint32_t z = row / static_cast<uint32_t>(d.extent[1]), y = row - z * static_cast<uint32_t>(d.extent[1]);
		const int64_t at = static_cast<int64_t>(z) * d.slice_pitch + static_cast<int64_t>(y) * d.row_pitch;
		const size_t out = static_cast<size_t>(row) * static_cast<size_t>(nx);
		if (shift < 6u) { // the row is one chunk: its mask is the segment's part of the ballot
			const uint64_t all = chunk_sources(volume, at, live, 0, nx, lane, l, words, d.to_empty);
			count += __popcll(all);
			const uint64_t m = (all >> (seg << shift)) & ((uint64_t{1} << S) - 1u);
			const int32_t g = distance_chunk_nearest(m, l, static_cast<int32_t>(l), -1, -1);
			if (live && static_cast<int32_t>(l) < nx) st32(field, out + l, g < kDistanceMaxExtent ? distance_sq(g) : kDistanceNone);
		} else { // (everything that steers the loops below is a ballot or made of ballots: the same in every lane)
			const int32_t chunks = (nx + 63) >> 6;
			int32_t left = -1;   // the last source before the chunk, or -1
			int32_t ahead = -1;  // the first source after the chunk, or -1
			// every chunk is read once: chunks below `scanned` have been read, and all of them were empty but the one whose mask is kept
			int32_t scanned = 1, kept_chunk = 0;
			uint64_t kept = chunk_sources(volume, at, live, 0, nx, lane, l, words, d.to_empty);
			for (int32_t c = 0; c < chunks; ++c) {
				const int32_t c0 = c << 6;
				const uint64_t m = c == kept_chunk ? kept : 0u;
				count += __popcll(m);
				if (ahead < c0 + 64) { // the source found last lies in this chunk or before it, so its mask has been used: look on
					ahead = -1;
					while (scanned < chunks && ahead < 0) {
						const uint64_t next = chunk_sources(volume, at, live, scanned << 6, nx, lane, l, words, d.to_empty);
						if (next != 0) {
							ahead = (scanned << 6) + __ffsll(static_cast<long long>(next)) - 1;
							kept = next;
							kept_chunk = scanned;
						}
						++scanned;
					}
				}
				const int32_t x = c0 + static_cast<int32_t>(l);
				const int32_t g = distance_chunk_nearest(m, l, x, left, ahead);
				if (live && x < nx) st32(field, out + static_cast<size_t>(x), g < kDistanceMaxExtent ? distance_sq(g) : kDistanceNone);
				if (m != 0) left = c0 + 63 - __clzll(static_cast<long long>(m));
			}
		}
	}
	// (the ballots are the wave's: every lane holds the same count)
	if (lane == 0 && count != 0) __hip_atomic_fetch_add((g_ull*)sources, static_cast<unsigned long long>(count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per line of n values that lie `stride` words apart: out = the lower envelope of in.  nx lines lie side by side in a row of the
// plane, and row r of lines begins at word r * row_step.  key != null (the last pass, along z: a line is (x, y = r) and a value's place
// is its index in the tight field): the values take BM_DISTANCE_OUTSIDE's minimum and feed the max key.
__global__ __launch_bounds__(kThreads) void distance_line(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ stack,
														  unsigned long long* __restrict__ key, const DistanceDims d, const uint32_t lines, const uint32_t n,
														  const uint32_t stride, const uint32_t row_step) {
	const uint32_t line = blockIdx.x * kThreads + threadIdx.x;
	const bool live = line < lines;
	const uint32_t nx = static_cast<uint32_t>(d.extent[0]);
	const uint32_t r = (live ? line : 0u) / nx, x = (live ? line : 0u) - r * nx;
	const size_t base = static_cast<size_t>(r) * row_step + x;
	const uint32_t steps = live ? n : 0u;
	auto f_at = [&](uint32_t j) { return ld32(in, base + static_cast<size_t>(j) * stride); };
	auto load_entry = [&](uint32_t k) { return ld32(stack, static_cast<size_t>(k) * lines + line); };
	auto store_entry = [&](uint32_t k, uint32_t e) { st32(stack, static_cast<size_t>(k) * lines + line, e); };
	LineTop top = {0u, 0u, 0u, 0u};
	uint32_t f = steps > 0 ? f_at(0) : kDistanceNone;
	for (uint32_t u = 0; u < steps; ++u) {
		const uint32_t after = u + 1 < steps ? f_at(u + 1) : kDistanceNone; // (asked for before the pushes and pops of this value)
		if (f != kDistanceNone) distance_line_push(top, u, f, n, load_entry, store_entry, f_at);
		f = after;
	}
	uint64_t best = 0;
	for (uint32_t u = steps; u-- > 0;) {
		uint32_t v = distance_line_emit(top, u, load_entry, f_at);
		const size_t index = base + static_cast<size_t>(u) * stride;
		if (key) {
			if (d.outside) {
				const uint32_t edge = distance_outside_sq(d.extent, static_cast<int32_t>(x), static_cast<int32_t>(r), static_cast<int32_t>(u));
				v = edge < v ? edge : v;
			}
			const uint64_t k = distance_max_key(v, static_cast<uint32_t>(index));
			best = k > best ? k : best;
		}
		st32(out, index, v);
	}
	if (key) { // (the same in every lane: the whole wave is here)
#pragma unroll
		for (int s = 1; s < 64; s <<= 1) {
			const uint64_t other = static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(best), s, 64));
			best = other > best ? other : best;
		}
		if ((threadIdx.x & 63u) == 0 && best != 0) __hip_atomic_fetch_max((g_ull*)key, static_cast<unsigned long long>(best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// tail: the max key and the source count -> the 32 bytes of the result
__global__ __launch_bounds__(64) void distance_finish(const uint64_t* __restrict__ tail, uint64_t* __restrict__ result) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const DistanceRecord rec = distance_record(ld64(tail, 0), ld64(tail, 1));
	st64(result, 0, rec.sources);
	st64(result, 1, static_cast<uint64_t>(rec.max_sq));
	st64(result, 2, rec.max_at);
	st64(result, 3, 0);
}

// out[i] = 1 where field[i] <= limit_sq (above: where it is not), for i < n.  Granule g holds the bytes 4 g - lead ... + 3, lead = the
// output's address modulo 4: a granule whose four bytes are voxels is one aligned word.
__global__ __launch_bounds__(kThreads) void distance_mask(const uint32_t* __restrict__ field, uint8_t* __restrict__ out, const uint32_t n, const uint32_t limit_sq,
														  const uint32_t above, const uint32_t granules) {
	const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
	if (g >= granules) return;
	const uint32_t lead = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(out) & 3u);
	const int64_t first = static_cast<int64_t>(g) * 4 - lead;
	if (first >= 0 && first + 4 <= static_cast<int64_t>(n)) {
		uint32_t word = 0;
#pragma unroll
		for (int b = 0; b < 4; ++b) word |= distance_mask_byte(ld32(field, static_cast<size_t>(first + b)), limit_sq, above) << (8 * b);
		*(g_u32*)((g_u8*)out + first) = word;
	} else {
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const int64_t i = first + b;
			if (i >= 0 && i < static_cast<int64_t>(n)) st8(out, static_cast<size_t>(i), distance_mask_byte(ld32(field, static_cast<size_t>(i)), limit_sq, above));
		}
	}
}

// ---- host-callable launchers (kernels.h)
void launch_distance_field(const DistanceDims& d, const uint8_t* volume, uint32_t* field, void* result, void* workspace, hipStream_t stream, hipEvent_t* marks) {
	int mark = 0;
	auto stamp = [&]() { if (marks) (void)hipEventRecord(marks[mark++], stream); };
	uint8_t* ws = static_cast<uint8_t*>(workspace);
	uint32_t* h = reinterpret_cast<uint32_t*>(ws);
	uint32_t* stack = reinterpret_cast<uint32_t*>(ws + distance_plane_bytes(d));
	unsigned long long* tail = reinterpret_cast<unsigned long long*>(ws + 2 * distance_plane_bytes(d));
	const uint32_t nx = static_cast<uint32_t>(d.extent[0]), ny = static_cast<uint32_t>(d.extent[1]), nz = static_cast<uint32_t>(d.extent[2]);
	stamp();
	(void)hipMemsetAsync(tail, 0, kDistanceTailBytes, stream);
	const uint32_t shift = distance_row_shift(d.extent[0]);
	const uint64_t rows = static_cast<uint64_t>(ny) * nz, per_wave = 64u >> shift, turns = (rows + per_wave - 1) / per_wave;
	const uint64_t blocks = (turns + kThreads / 64 - 1) / (kThreads / 64);
	hipLaunchKernelGGL(distance_x, dim3(static_cast<unsigned>(blocks < kRowBlocks ? blocks : kRowBlocks)), dim3(kThreads), 0, stream, volume, field, tail + 1, d, shift,
					   static_cast<uint32_t>(turns));
	stamp();
	// along y: the lines are (x, z); the lines of one z share a row of lines, ny * nx words from the next
	const uint32_t lines_y = nx * nz, lines_z = nx * ny;
	hipLaunchKernelGGL(distance_line, dim3((lines_y + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, field, h, stack, static_cast<unsigned long long*>(nullptr), d, lines_y,
					   ny, nx, nx * ny);
	stamp();
	// along z: the lines are (x, y), one row of lines per y
	hipLaunchKernelGGL(distance_line, dim3((lines_z + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, h, field, stack, tail, d, lines_z, nz, nx * ny, nx);
	hipLaunchKernelGGL(distance_finish, dim3(1), dim3(64), 0, stream, reinterpret_cast<const uint64_t*>(tail), static_cast<uint64_t*>(result));
	stamp();
}

void launch_distance_mask(const uint32_t* field, uint64_t n, uint32_t limit_sq, uint32_t above, uint8_t* out, hipStream_t stream) {
	const uint32_t lead = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(out) & 3u);
	const uint32_t granules = static_cast<uint32_t>((n + lead + 3) / 4);
	hipLaunchKernelGGL(distance_mask, dim3((granules + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, field, out, static_cast<uint32_t>(n), limit_sq, above, granules);
}

} // namespace bm
