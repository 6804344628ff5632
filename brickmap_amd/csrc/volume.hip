// volume.hip -- batched volume queries against the live scene (bm_scene_query_volumes): for each of n boxes or spheres, the number of
// solid voxels inside, their tight bounds and the brick cells that could not be answered because their brick is not resident.
//
// A work item is a run of 16 brick cells along x that starts at a multiple of 16 cells (so it lies in one supercell: 16 consecutive
// index words, 16 consecutive cube-field bytes) at one (cy, cz) of a record's clipped shape.  Shapes range from one voxel to the whole
// world and their sizes are only known on the device, so the work is laid out there:
//
//   plan   : one lane per record validates and clips it, writes the initial result (0, INT_MAX / INT_MIN bounds, status) and the record's
//            item count; a workgroup scans its 256 counts (64-bit) and leaves their sum
//   scan   : one workgroup turns the workgroups' sums into exclusive offsets and the total (skipped when plan ran as one workgroup)
//   count  : persistent wave64 kernel.  A wave walks the items in strides of four, one item per 16 lanes and one cell per lane; a lane
//            finds its item's record by binary search (workgroup offsets, then the 256 counts inside), reads the plane-0 cube-field
//            byte -- anything but 0 means the cell holds no brick and ends the lane's work there -- then the index word and, when it is
//            loaded, the 64-byte brick, builds the cover mask (closed form per axis for a box and for a sphere's cells that lie wholly
//            inside; the 64-bit integer inequality per voxel for the cells a sphere's surface crosses; a sphere's cells wholly outside are
//            dropped from their corners), popcounts, reduces over the 16 lanes -- over the wave when its four items share a record --
//            and adds with one 64-bit atomic add, one 32-bit add and six atomic min / max per group.  Integer atomics: any order, one result.
//   finish : -1 bounds for empty results, half-open upper bounds, and the 0 / 1 values of BM_VOLUME_ANY
//
// With BM_VOLUME_ANY an item of a record that already has solid != 0 returns at once, and no bounds are kept.
#include <hip/hip_runtime.h>

#include <climits>

#include "global_mem.h"
#include "kernels.h"
#include "voxel_bits.h"

namespace bm {

#ifndef BM_VOLUME_WAVES
#define BM_VOLUME_WAVES 7 // waves per SIMD the count kernel's register budget is sized for (launch bounds: 256 threads, this many per SIMD)
#endif

namespace {

constexpr int kBox = 1, kSphere = 2;      // BM_EDIT_BOX, BM_EDIT_SPHERE
constexpr int kRecordWords = 12, kResultWords = 10; // bm_volume, bm_volume_result

// a record, validated and clipped to the world like an edit's shape (World::edit_bounds)
struct Shape {
	bool ok;         // well-formed
	bool sphere;
	int lo[3], hi[3]; // clipped bounds in voxels, half-open; lo == hi == 0 when nothing is left
	int c[3], radius;
	uint32_t nruns, ncy, ncz; // runs of 16 cells per row, rows, slices of the clipped shape
	__device__ __forceinline__ uint64_t items() const { return static_cast<uint64_t>(nruns) * ncy * ncz; }
};

__device__ __forceinline__ Shape load_shape(const int* __restrict__ volumes, size_t i, int size, int height) {
	const auto p = [&](int k) { return ldi32(volumes, i * kRecordWords + k); };
	Shape s;
	const int shape = p(0);
	s.radius = p(10);
	s.sphere = shape == kSphere;
	s.ok = (shape == kBox || shape == kSphere) && p(11) == 0 && !(s.sphere && s.radius < 0);
	bool inside = s.ok;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		s.c[k] = p(7 + k);
		long long a = p(1 + k), b = p(4 + k);
		if (!s.sphere && b < a) { s.ok = false; inside = false; }
		if (s.sphere) { a = static_cast<long long>(s.c[k]) - s.radius; b = static_cast<long long>(s.c[k]) + s.radius + 1; }
		const long long top = k == 2 ? height : size;
		a = a < 0 ? 0 : (a > top ? top : a);
		b = b < 0 ? 0 : (b > top ? top : b);
		s.lo[k] = static_cast<int>(a);
		s.hi[k] = static_cast<int>(b);
		inside = inside && a < b;
	}
	s.nruns = s.ncy = s.ncz = 0;
	if (inside) {
		s.nruns = static_cast<uint32_t>(((s.hi[0] - 1) >> 7) - (s.lo[0] >> 7) + 1);
		s.ncy = static_cast<uint32_t>(((s.hi[1] - 1) >> 3) - (s.lo[1] >> 3) + 1);
		s.ncz = static_cast<uint32_t>(((s.hi[2] - 1) >> 3) - (s.lo[2] >> 3) + 1);
	}
	return s;
}

// exclusive scan of one 64-bit value per thread of a 256-thread workgroup; *total = the sum
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* lds, uint64_t* total) {
	const uint32_t t = threadIdx.x;
	lds[t] = v;
	__syncthreads();
	uint64_t sum = v;
#pragma unroll
	for (uint32_t d = 1; d < 256; d <<= 1) {
		const uint64_t other = t >= d ? lds[t - d] : 0;
		__syncthreads();
		sum += other;
		lds[t] = sum;
		__syncthreads();
	}
	*total = lds[255];
	return sum - v;
}

// local[i] = items of the records before i in i's workgroup; block_off[b] = items of workgroup b (one workgroup: its offset 0 and the total)
__global__ __launch_bounds__(256) void volume_plan(const int* __restrict__ volumes, uint32_t* __restrict__ results, uint64_t* __restrict__ local,
												   uint64_t* __restrict__ block_off, uint32_t n, int size, int height) {
	__shared__ uint64_t lds[256];
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	uint64_t items = 0;
	if (i < n) {
		const Shape s = load_shape(volumes, i, size, height);
		items = s.items();
		const size_t at = static_cast<size_t>(i) * kResultWords;
		st32(results, at, 0u);
		st32(results, at + 1, 0u);
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			st32(results, at + 2 + k, static_cast<uint32_t>(INT_MAX));
			st32(results, at + 5 + k, static_cast<uint32_t>(INT_MIN));
		}
		st32(results, at + 8, 0u);
		st32(results, at + 9, s.ok ? 0u : 1u);
	}
	uint64_t total;
	const uint64_t before = block_scan(items, lds, &total);
	if (i < n) st64(local, i, before);
	if (threadIdx.x == 0) {
		if (gridDim.x == 1) {
			st64(block_off, 0, 0);
			st64(block_off, 1, total);
		} else {
			st64(block_off, blockIdx.x, total);
		}
	}
}

// block_off[0 ... nblocks): sums -> exclusive offsets; block_off[nblocks] = the total
__global__ __launch_bounds__(256) void volume_scan(uint64_t* __restrict__ block_off, uint32_t nblocks) {
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

// bits [a, b) of a byte, 0 <= a <= b <= 8
__device__ __forceinline__ uint32_t bit_range(int a, int b) { return ((1u << b) - 1u) & ~((1u << a) - 1u); }

__device__ __forceinline__ uint64_t sq(long long d) { return static_cast<uint64_t>(d * d); } // |d| <= 2^31 + 7

template <bool ANY>
__global__ __launch_bounds__(256, BM_VOLUME_WAVES) void volume_count(const DeviceScene sc, const int size, const int height, const int* __restrict__ volumes,
													uint32_t* __restrict__ results, const uint64_t* __restrict__ local,
													const uint64_t* __restrict__ block_off, const uint32_t n, const uint32_t nblocks) {
	const uint64_t total = ld64(block_off, nblocks);
	const uint32_t lane = threadIdx.x & 63, cl = lane & 15;
	const uint64_t waves = static_cast<uint64_t>(gridDim.x) * 4, wave = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
	// the record of the lane's last item and its range of items: consecutive items mostly share it
	uint32_t r = 0;
	uint64_t r_begin = 0, r_end = 0;
	Shape s;
	s.ok = false;
	s.nruns = s.ncy = 1;

	for (uint64_t base = wave * 4; base < total; base += waves * 4) {
		const uint64_t t = base + (lane >> 4);
		const bool valid = t < total;
		if (valid && !(t >= r_begin && t < r_end)) {
			uint32_t a = 0, b = nblocks; // the last workgroup whose offset is <= t, then the last record in it whose offset is <= the rest
			while (b - a > 1) {
				const uint32_t mid = (a + b) >> 1;
				if (ld64(block_off, mid) <= t) a = mid; else b = mid;
			}
			const uint64_t off = ld64(block_off, a), rest = t - off;
			const uint32_t first = a * 256;
			a = 0;
			b = n - first < 256u ? n - first : 256u;
			while (b - a > 1) {
				const uint32_t mid = (a + b) >> 1;
				if (ld64(local, first + mid) <= rest) a = mid; else b = mid;
			}
			r = first + a;
			s = load_shape(volumes, r, size, height);
			r_begin = off + ld64(local, r);
			r_end = r_begin + s.items();
		}
		uint32_t cnt = 0, unres = 0;
		int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
		bool skip = !valid;
		if (ANY && valid) skip = __hip_atomic_load((const g_u32*)results + static_cast<size_t>(r) * kResultWords, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
		if (!skip) {
			s = load_shape(volumes, r, size, height); // again (16 lanes, one address): a shape kept across the search and the reduction costs the registers of a wave per SIMD
			const uint32_t j = static_cast<uint32_t>(t - r_begin), q = j / s.nruns;
			const int cx = ((s.lo[0] >> 7) + static_cast<int>(j - q * s.nruns)) * 16 + static_cast<int>(cl);
			const int cy = (s.lo[1] >> 3) + static_cast<int>(q % s.ncy), cz = (s.lo[2] >> 3) + static_cast<int>(q / s.ncy);
			const int cc[3] = {cx, cy, cz};
			if (cx >= (s.lo[0] >> 3) && cx <= ((s.hi[0] - 1) >> 3) &&
				ld8(sc.cube_field, static_cast<size_t>(cz + 1) * sc.cf_pxy + (static_cast<size_t>(cy + 1) << sc.cf_shift) + static_cast<size_t>(cx + 1)) == 0) {
				// the clipped shape's part of the cell: [v0, v1) per axis, in voxels of the cell
				int v0[3], v1[3];
				uint64_t near2 = 0, far2 = 0;
				const uint64_t r2 = static_cast<uint64_t>(s.radius) * static_cast<uint64_t>(s.radius);
#pragma unroll
				for (int k = 0; k < 3; ++k) {
					v0[k] = s.lo[k] - 8 * cc[k] > 0 ? s.lo[k] - 8 * cc[k] : 0;
					v1[k] = s.hi[k] - 8 * cc[k] < 8 ? s.hi[k] - 8 * cc[k] : 8;
					if (s.sphere) { // nearest and farthest voxel of that part from the centre, per axis
						const long long lo = 8ll * cc[k] + v0[k] - s.c[k], hi = 8ll * cc[k] + v1[k] - 1 - s.c[k];
						near2 += sq(lo > 0 ? lo : (hi < 0 ? hi : 0));
						far2 += sq(-lo > hi ? lo : hi);
					}
				}
				if (!s.sphere || near2 <= r2) { // the shape has a voxel in the cell
					const uint32_t iw = ld32(sc.index_grid, index_word_at(sc.sg_xy, sc.sg_xy2, cx, cy, cz));
					if (!(iw & kLoadedBit)) {
						unres = 1;
					} else {
						const size_t brick = brick_first_word(ld32(sc.pool_base, supercell_of(sc.sg_xy, sc.sg_xy2, cx, cy, cz)), iw);
						uint32_t or_even = 0, or_odd = 0, zbits = 0; // the covered solid bits of words 0, 2, ... (y 0-3) and 1, 3, ... (y 4-7); slices that hold one
						if (!s.sphere || far2 <= r2) {
							const uint32_t xm = bit_range(v0[0], v1[0]), ym = bit_range(v0[1], v1[1]), zm = bit_range(v0[2], v1[2]);
							const uint32_t even = bits4_to_bytes(ym) * xm, odd = bits4_to_bytes(ym >> 4) * xm;
							u32x4 v[4];
#pragma unroll
							for (int h = 0; h < 4; ++h) v[h] = ld128(sc.brick_arena, (brick + 4 * h) * sizeof(uint32_t));
#pragma unroll
							for (int h = 0; h < 4; ++h) {
								const uint32_t m0 = (zm >> (2 * h)) & 1u ? 0xFFFFFFFFu : 0u, m1 = (zm >> (2 * h + 1)) & 1u ? 0xFFFFFFFFu : 0u;
								const uint32_t a = v[h].x & even & m0, b = v[h].y & odd & m0, c = v[h].z & even & m1, d = v[h].w & odd & m1;
								cnt += __popc(a) + __popc(b) + __popc(c) + __popc(d);
								or_even |= a | c;
								or_odd |= b | d;
								zbits |= ((a | b) != 0 ? 1u : 0u) << (2 * h) | ((c | d) != 0 ? 1u : 0u) << (2 * h + 1);
							}
						} else {
							// voxel (x, y, z) of the cell lies at e + (x, y, z) from the centre: (e0 + x)^2 + (e1 + y)^2 + (e2 + z)^2 <= r^2  <=>
							// x (2 e0 + x) + y (2 e1 + y) + z (2 e2 + z) <= room, room = r^2 - |e|^2
							const long long e0 = 8ll * cx - s.c[0], e1 = 8ll * cy - s.c[1], e2 = 8ll * cz - s.c[2];
							const long long lim = 1ll << 24;
							const bool small = e0 > -lim && e0 < lim && e1 > -lim && e1 < lim && e2 > -lim && e2 < lim;
#pragma unroll 1
							for (int w = 0; w < 16; ++w) {
								uint32_t m = 0;
								if (small) {
									// each term is below 2^28 in magnitude, their sum below 2^30: room clamped to +-2^30 decides the same, in 32 bits
									const long long room64 = static_cast<long long>(r2 - sq(e0) - sq(e1) - sq(e2));
									const int room = static_cast<int>(room64 < -(1ll << 30) ? -(1ll << 30) : (room64 > (1ll << 30) ? (1ll << 30) : room64));
									const int ex = 2 * static_cast<int>(e0), ey = 2 * static_cast<int>(e1), ez = 2 * static_cast<int>(e2);
									const int z = w >> 1, rz = room - z * (ez + z);
#pragma unroll
									for (int y = 0; y < 4; ++y) {
										const int yy = 4 * (w & 1) + y, ry = rz - yy * (ey + yy);
#pragma unroll
										for (int x = 0; x < 8; ++x) m |= (x * (ex + x) <= ry ? 1u : 0u) << (8 * y + x);
									}
								} else { // a centre 2^24 voxels or more from the cell: voxel by voxel in 64 bits
#pragma unroll 1
									for (int b = 0; b < 32; ++b)
										m |= (sq(e0 + (b & 7)) + sq(e1 + 4 * (w & 1) + (b >> 3)) + sq(e2 + (w >> 1)) <= r2 ? 1u : 0u) << b;
								}
								m &= ld32(sc.brick_arena, brick + w);
								cnt += __popc(m);
								if (w & 1) or_odd |= m; else or_even |= m;
								zbits |= (m != 0 ? 1u : 0u) << (w >> 1);
							}
						}
						if (!ANY && cnt != 0) {
							uint32_t xbits = or_even | or_odd;
							xbits |= xbits >> 16;
							xbits = (xbits | xbits >> 8) & 0xFFu;
							const uint32_t ybits = nonzero_bytes4(or_even) | nonzero_bytes4(or_odd) << 4;
							const uint32_t bits[3] = {xbits, ybits, zbits};
#pragma unroll
							for (int k = 0; k < 3; ++k) {
								mn[k] = 8 * cc[k] + __builtin_ctz(bits[k]);
								mx[k] = 8 * cc[k] + 31 - __builtin_clz(bits[k]);
							}
						}
					}
				}
			}
		}
		// ---- one set of atomics per 16 lanes, or per wave when its items share a record (lanes without a cell hold the neutral values)
		const uint32_t r0 = __builtin_amdgcn_readfirstlane(r); // lane 0's item is valid: base < total
		const bool same = __ballot(valid && r != r0) == 0;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			if (d >= 16 && !same) break;
			cnt += __shfl_xor(cnt, d, 64);
			unres += __shfl_xor(unres, d, 64);
			if (!ANY) {
#pragma unroll
				for (int k = 0; k < 3; ++k) {
					const int a = __shfl_xor(mn[k], d, 64), b = __shfl_xor(mx[k], d, 64);
					mn[k] = a < mn[k] ? a : mn[k];
					mx[k] = b > mx[k] ? b : mx[k];
				}
			}
		}
		if (valid && (same ? lane == 0 : cl == 0)) {
			uint32_t* res = results + static_cast<size_t>(r) * kResultWords;
			if (cnt != 0) {
				atomicAdd(reinterpret_cast<unsigned long long*>(res), static_cast<unsigned long long>(cnt));
				if (!ANY) {
#pragma unroll
					for (int k = 0; k < 3; ++k) {
						atomicMin(reinterpret_cast<int*>(res) + 2 + k, mn[k]);
						atomicMax(reinterpret_cast<int*>(res) + 5 + k, mx[k]); // the last voxel; finish makes it half-open
					}
				}
			}
			if (unres != 0) atomicAdd(res + 8, unres);
		}
	}
}

__global__ __launch_bounds__(256) void volume_finish(uint32_t* __restrict__ results, uint32_t n, int any) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const size_t at = static_cast<size_t>(i) * kResultWords;
	const bool solid = (ld32(results, at) | ld32(results, at + 1)) != 0;
	if (any) {
		st32(results, at, solid ? 1u : 0u);
		st32(results, at + 1, 0u);
		st32(results, at + 8, !solid && ld32(results, at + 8) != 0 ? 1u : 0u);
	}
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		if (any || !solid) {
			st32(results, at + 2 + k, 0xFFFFFFFFu);
			st32(results, at + 5 + k, 0xFFFFFFFFu);
		} else {
			st32(results, at + 5 + k, ld32(results, at + 5 + k) + 1u);
		}
	}
}

} // namespace

int volume_blocks_per_cu(bool any) {
	return any ? resident_blocks_per_cu(volume_count<true>) : resident_blocks_per_cu(volume_count<false>);
}

size_t volume_tmp_bytes(uint32_t n) { return (static_cast<size_t>(n) + (n + 255) / 256 + 1) * sizeof(uint64_t); }

void launch_volume_query(const DeviceScene& sc, const void* volumes, void* results, uint32_t n, bool any, uint64_t* tmp, int resident_blocks, hipStream_t stream) {
	const uint32_t nblocks = (n + 255) / 256;
	uint64_t* local = tmp;
	uint64_t* block_off = tmp + n;
	const int size = sc.cells * 8, height = sc.cells_height * 8;
	const int* in = static_cast<const int*>(volumes);
	uint32_t* out = static_cast<uint32_t*>(results);
	hipLaunchKernelGGL(volume_plan, dim3(nblocks), dim3(256), 0, stream, in, out, local, block_off, n, size, height);
	if (nblocks > 1) hipLaunchKernelGGL(volume_scan, dim3(1), dim3(256), 0, stream, block_off, nblocks);
	// never more waves than groups of four items: a record has at most (runs per row) * rows * slices of them
	const uint64_t most = static_cast<uint64_t>(n) * static_cast<uint64_t>((sc.cells + 15) / 16) * static_cast<uint64_t>(sc.cells) * static_cast<uint64_t>(sc.cells_height);
	uint64_t blocks = (most + 15) / 16;
	if (blocks > static_cast<uint64_t>(resident_blocks)) blocks = static_cast<uint64_t>(resident_blocks);
	if (blocks < 1) blocks = 1;
	if (any) hipLaunchKernelGGL(volume_count<true>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, sc, size, height, in, out, local, block_off, n, nblocks);
	else hipLaunchKernelGGL(volume_count<false>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, sc, size, height, in, out, local, block_off, n, nblocks);
	hipLaunchKernelGGL(volume_finish, dim3(nblocks), dim3(256), 0, stream, out, n, any ? 1 : 0);
}

} // namespace bm
