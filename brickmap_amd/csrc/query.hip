// query.hip -- batched ray queries against the live scene (bm_scene_cast_rays): what the first hit of each ray is, without a frame.
//
// One persistent wave64 kernel in the shape of wavefront.hip's wf_trace: a wave owns a private range of ray slots (one atomic per
// BM_QUERY_GRAB rays) and refills its idle lanes from it; every round runs either the brick-grid walk (phase A, walk_round) or the
// candidate resolution (phase B, process_candidate with LDS-direct brick staging) for the lanes that want it.  Per ray it does what
// the extend kernel does -- the same device functions, so a hit is bit-identical to the reference's intersect_voxel -- and writes
// one 32-byte bm_ray_hit at the ray's own index.  No shading, no accumulation, no counters.
#include "traverse.h"

#include "kernels.h"

namespace bm {

#ifndef BM_QUERY_GRAB
#define BM_QUERY_GRAB 64 // ray slots a wave reserves per atomic (as BM_WF_GRAB)
#endif
#ifndef BM_QUERY_REFILL
#define BM_QUERY_REFILL 32 // idle lanes that trigger a refill
#endif
#ifndef BM_QUERY_QUORUM_DIV
#define BM_QUERY_QUORUM_DIV 4 // phase B once a quarter of the live lanes hold a candidate
#endif
#ifndef BM_QUERY_STEPS
#define BM_QUERY_STEPS 4
#endif
#ifndef BM_QUERY_WAVES
#define BM_QUERY_WAVES 6 // waves per SIMD the register budget is sized for (launch bounds: 256 threads, this many per SIMD)
#endif

namespace {

// 16-byte global-memory accesses (the kernel arguments are global pointers: no flat_* accesses)
__device__ __forceinline__ float4 ldg4(const float4* p, size_t i) { return p[i]; }
__device__ __forceinline__ void stg4(float4* p, size_t i, float4 v) { p[i] = v; }

__device__ __forceinline__ bool finite3(f3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

} // namespace

// rays: n bm_ray records (two float4 each: origin, direction.x | direction.y, direction.z, tmax, reserved); hits: n bm_ray_hit records
// (distance, normal | voxel, level).  ticket: a zeroed word, the slot counter of this launch.  campos: the LoD centre in brick cells
// (only read when sc's LoD distances are below INT_MAX).
template <bool REQUEST>
__global__ __launch_bounds__(256, BM_QUERY_WAVES) void query_rays(const DeviceScene sc, const int3 campos, const float4* __restrict__ rays,
																 float4* __restrict__ hits, uint32_t* __restrict__ ticket, uint32_t total) {
	__shared__ unsigned long long lds_brick[8 * 256];
	const int lane = threadIdx.x & 63;
	const int cp[3] = {campos.x, campos.y, campos.z};

	RayState r;
	r.hit = false;
	r.n = mk(0.f, 0.f, 0.f);
	Tally tally;
	HitInfo info;
	int state = ST_NEED;
	bool have = false; // the lane holds a ray whose result has not been written yet
	uint32_t idx = 0;
	float tmax = 0.f;
	int scale = 0;     // the walk ran with direction * 2^-scale: its distances are the ray's multiplied by 2^scale
	uint32_t cur = 0, end = 0;
	bool work_left = true;
	long long rounds_left = (static_cast<long long>(total) + 64) * (2ll * sc.cells + sc.cells_height + 64); // hang guard only

	for (;;) {
		// ---- retire: one 32-byte result per ended ray, at the ray's index
		if (state == ST_NEED && have) {
			have = false;
			const float dist = __builtin_ldexpf(r.distance, -scale);
			float4 w0 = make_float4(__int_as_float(0x7F800000), 0.f, 0.f, 0.f);
			float4 w1 = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1));
			if (r.hit && dist <= tmax) {
				int px, py, pz;
				cell_coords(sc, r, px, py, pz); // the hit cell: process_candidate leaves r.p on it
				const int s = info.sub_id;
				int vx = px * 8, vy = py * 8, vz = pz * 8;
				if (info.level == 2) { vx += s & 7; vy += (s >> 3) & 7; vz += s >> 6; }
				if (info.level == 1) { vx += 4 * (s & 1); vy += 4 * ((s >> 1) & 1); vz += 4 * (s >> 2); }
				w0 = make_float4(dist, r.n.x, r.n.y, r.n.z);
				w1 = make_float4(__int_as_float(vx), __int_as_float(vy), __int_as_float(vz), __int_as_float(info.level));
			}
			stg4(hits, 2 * static_cast<size_t>(idx), w0);
			stg4(hits, 2 * static_cast<size_t>(idx) + 1, w1);
		}
		const unsigned long long need = __ballot(state == ST_NEED);
		const int nN = __popcll(need);
		const int nJ = __popcll(__ballot(state == ST_JUMP));
		const int nA = __popcll(__ballot(state == ST_OUTER)) + nJ;
		const int nB = __popcll(__ballot(state == ST_CAND));
		const bool more = work_left || cur < end;
		if (--rounds_left < 0) break;
		// ---- refill idle lanes from the wave's private slot range
		if (more && nN > 0 && (nN >= BM_QUERY_REFILL || nA + nB == 0)) {
			if (cur == end) {
				uint32_t base = 0;
				if (lane == 0) base = atomicAdd(ticket, static_cast<uint32_t>(BM_QUERY_GRAB));
				base = __builtin_amdgcn_readfirstlane(base);
				if (base >= total) {
					work_left = false;
				} else {
					cur = base;
					end = total - base < static_cast<uint32_t>(BM_QUERY_GRAB) ? total : base + static_cast<uint32_t>(BM_QUERY_GRAB);
				}
			}
			const uint32_t avail = end - cur;
			const uint32_t take = static_cast<uint32_t>(nN) < avail ? static_cast<uint32_t>(nN) : avail;
			if (take > 0) {
				const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(need >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(need), 0u));
				if (state == ST_NEED && rank < take) {
					idx = cur + rank;
					const float4 a = ldg4(rays, 2 * static_cast<size_t>(idx)), b = ldg4(rays, 2 * static_cast<size_t>(idx) + 1);
					const f3 o = mk(a.x, a.y, a.z);
					f3 d = mk(a.w, b.x, b.y);
					tmax = __float_as_uint(b.w) == 0u ? b.z : __int_as_float(0x7FC00000); // reserved word set: tmax NaN, every cell is beyond it
					have = true;
					r.hit = false;
					r.n = mk(0.f, 0.f, 0.f); // a ray that starts inside a solid voxel reports this normal
					// degenerate input is a miss, before the walk: non-finite origin or direction, zero direction
					const float m = fmaxf(fabsf(d.x), fmaxf(fabsf(d.y), fabsf(d.z)));
					if (!finite3(o) || !finite3(d) || m == 0.f) {
						state = ST_NEED;
					} else {
						// The walk's sentinel for a zero direction component is the reference's tmax = 1e6; with the largest component
						// in [0.5, 2) no other axis's tmax reaches it inside the grid.  Any other direction walks as direction * 2^-e
						// (largest component in [1, 2)): power-of-two scaling is exact, so every tmax, tdelta and distance of the walk
						// is the unscaled one times 2^e, and the cells visited are the same.  Unit directions are never scaled.
						scale = 0;
						if (m < 0.5f || m >= 2.f) {
							scale = __builtin_amdgcn_frexp_expf(m) - 1;
							d = mk(__builtin_ldexpf(d.x, -scale), __builtin_ldexpf(d.y, -scale), __builtin_ldexpf(d.z, -scale));
						}
						state = ray_setup<false>(sc, o, d, r, tally);
					}
				}
				cur += take;
			}
			continue;
		}
		if (nA + nB == 0) {
			if (!more) break;
			continue;
		}
		const int live = nA + nB;
		if (nB >= (live + BM_QUERY_QUORUM_DIV - 1) / BM_QUERY_QUORUM_DIV || nA == 0) {
			// ---- phase B: resolve non-empty cells.  A cell whose entry distance is already beyond tmax ends the ray as a miss
			// (every hit in it or behind it is at least that far: fp32 addition is monotone), and files no request.
			if (state == ST_CAND) {
				const int axis = move_axis(sc, r.last_step);
				const float nd = axis == 0 ? r.tx - r.dx : (axis == 1 ? r.ty - r.dy : (axis == 2 ? r.tz - r.dz : 0.f));
				if (!(__builtin_ldexpf(nd * 8.f + r.tminn, -scale) <= tmax)) {
					r.hit = false;
					state = ST_NEED;
				} else {
					state = process_candidate<false, true, REQUEST>(sc, cp, r, info, tally, lds_brick);
				}
			}
		} else {
			// ---- phase A: brick-grid walk
			uint32_t runs = 0, lanes = 0;
			state = walk_round<false, BM_QUERY_STEPS>(sc, r, state, nJ, nA - nJ, tally, runs, lanes);
		}
	}
	// (only after the hang guard: a lane still holding a ray reports a miss)
	if (have) {
		stg4(hits, 2 * static_cast<size_t>(idx), make_float4(__int_as_float(0x7F800000), 0.f, 0.f, 0.f));
		stg4(hits, 2 * static_cast<size_t>(idx) + 1, make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1)));
	}
}

// ---- host-callable launchers (kernels.h)
int query_blocks_per_cu(bool request) {
	return request ? resident_blocks_per_cu(query_rays<true>) : resident_blocks_per_cu(query_rays<false>);
}

void launch_query(const DeviceScene& sc, const int campos[3], const void* rays, void* hits, uint32_t n, uint32_t* ticket, int resident_blocks,
				  bool request, hipStream_t stream) {
	long long blocks = (static_cast<long long>(n) + BM_QUERY_GRAB * 4 - 1) / (BM_QUERY_GRAB * 4); // never more waves than slot ranges
	if (blocks > resident_blocks) blocks = resident_blocks;
	if (blocks < 1) blocks = 1;
	const int3 cp = make_int3(campos[0], campos[1], campos[2]);
	const float4* in = static_cast<const float4*>(rays);
	float4* out = static_cast<float4*>(hits);
	if (request) hipLaunchKernelGGL(query_rays<true>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, sc, cp, in, out, ticket, n);
	else hipLaunchKernelGGL(query_rays<false>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, sc, cp, in, out, ticket, n);
}

} // namespace bm
