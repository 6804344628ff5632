// reproject.hip -- temporal accumulation of reproject.h on the device (bm_reproject): one kernel, one thread per pixel, bound by memory.
// A pixel reads its accumulation value (16 bytes) and its hit record (32), gathers four taps of the previous history (a key and a
// float4 each) and writes its value and key of the new history (20): about 90 bytes if the taps hit the cache -- neighbouring pixels
// project to neighbouring places, so a tap is a pixel that three other pixels read as well.  The gather position is arbitrary: no LDS.
// The arithmetic of a pixel is that of reproject.h; what this file decides is only where the operands come from.  The taps of a
// pixel are loaded together and without branches, from positions clamped into the image, and counted afterwards (reproject_tap's
// `inside`): four independent loads in flight instead of four dependent branches.
#include "reproject.h"

#include "global_mem.h"
#include "kernels.h"

namespace bm {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float4 ld_float4(const void* p, size_t i) {
	const u32x4 v = ld128(p, static_cast<int64_t>(i * 16));
	return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ void st_float4(void* p, size_t i, float4 f) {
	u32x4 v;
	v.x = __float_as_uint(f.x); v.y = __float_as_uint(f.y); v.z = __float_as_uint(f.z); v.w = __float_as_uint(f.w);
	st128(p, static_cast<int64_t>(i * 16), v);
}

} // namespace

// accum: (R, G, B, n) per pixel; hits: two float4 per pixel (distance, normal | voxel, level); prev_image / prev_keys: the previous
// history, or null (both); out_image / out_keys: the new one.  n = width * height < 2^32
__global__ __launch_bounds__(kThreads) void reproject(const ReprojectCameras cams, const float4* __restrict__ accum, const float4* __restrict__ hits,
													  const float4* __restrict__ prev_image, const uint32_t* __restrict__ prev_keys,
													  float4* __restrict__ out_image, uint32_t* __restrict__ out_keys, float max_history, size_t n) {
	const size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) return;
	const float4 a = ld_float4(accum, i);
	const float4 h0 = ld_float4(hits, 2 * i), h1 = ld_float4(hits, 2 * i + 1);
	const uint32_t key_p = denoise_key(a.w, h0.y, h0.z, h0.w, __float_as_int(h1.x), __float_as_int(h1.y), __float_as_int(h1.z), __float_as_int(h1.w));
	st32(out_keys, i, key_p);
	float4 out = a;
	if (prev_image != nullptr && key_p != kDenoiseSpecialKey) {
		const uint32_t width = static_cast<uint32_t>(cams.width);
		const uint32_t y = static_cast<uint32_t>(i / width), x = static_cast<uint32_t>(i - static_cast<size_t>(y) * width);
		const float W = static_cast<float>(cams.width), H = static_cast<float>(cams.height);
		float u, v;
		RpTaps taps;
		if (reproject_project(cams.cur, cams.prev, W, H, static_cast<int>(x), static_cast<int>(y), h0.x, u, v) && reproject_taps(u, v, W, H, taps)) {
			// x0, y0 in -1 ... size - 1: a tap coordinate lies in -1 ... size, and its clamped place inside the image
			uint32_t key_q[4];
			float4 val_q[4];
			bool inside[4];
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const int qx = taps.x0 + (k & 1), qy = taps.y0 + (k >> 1);
				inside[k] = qx >= 0 && qx < cams.width && qy >= 0 && qy < cams.height;
				const int cx = min(max(qx, 0), cams.width - 1), cy = min(max(qy, 0), cams.height - 1);
				const size_t q = static_cast<size_t>(cy) * width + static_cast<size_t>(cx);
				key_q[k] = ld32(prev_keys, q);
				val_q[k] = ld_float4(prev_image, q);
			}
			RpSum sum = reproject_zero();
#pragma unroll
			for (int k = 0; k < 4; ++k) reproject_tap(sum, inside[k], key_q[k], key_p, taps.w[k], val_q[k].x, val_q[k].y, val_q[k].z, val_q[k].w);
			const float acc[4] = {a.x, a.y, a.z, a.w};
			float blended[4];
			if (reproject_blend(sum, max_history, acc, blended)) out = make_float4(blended[0], blended[1], blended[2], blended[3]);
		}
	}
	st_float4(out_image, i, out);
}

// ---- host-callable launcher (kernels.h)
void launch_reproject(const ReprojectCameras& cams, float max_history, const float* accum, const void* hits, const void* history_prev, void* history_out,
					  hipStream_t stream) {
	const size_t n = static_cast<size_t>(cams.width) * static_cast<size_t>(cams.height);
	const float4* prev_image = static_cast<const float4*>(history_prev);
	const uint32_t* prev_keys = history_prev ? reinterpret_cast<const uint32_t*>(prev_image + n) : nullptr;
	float4* out_image = static_cast<float4*>(history_out);
	hipLaunchKernelGGL(reproject, dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, cams,
					   reinterpret_cast<const float4*>(accum), static_cast<const float4*>(hits), prev_image, prev_keys, out_image,
					   reinterpret_cast<uint32_t*>(out_image + n), max_history, n);
}

} // namespace bm
