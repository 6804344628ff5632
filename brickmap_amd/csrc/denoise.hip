// denoise.hip -- the a-trous filter of denoise.h on the device (bm_denoise), and the device's pixel-centre rays
// (bm_camera_pixel_rays_device).  Image passes, all bound by memory: every pass reads a float4 image and the keys and writes a float4
// image.  The arithmetic of a pixel is that of denoise.h, tap by tap in its order; what this file decides is only where a tap's
// operands come from:
//   denoise_prepare        one thread per pixel, 48 bytes in, 20 out
//   denoise_moments        a TW x TH tile and its 3-pixel halo staged in LDS as (luminance, key): 8 bytes per staged pixel
//   denoise_atrous_tiled   steps 1 and 2: the tile and its halo of 2 * step pixels staged in LDS as (c, var | luminance | key)
//   denoise_atrous_far     larger steps: the 25 taps are read from global memory -- neighbouring lanes read neighbouring pixels, every
//                          tap is a pixel that 24 other pixels read as well, and the image stays in the last-level cache
// Where the line between the two lies was measured (profiles/denoise_time.txt): at 1080p the LDS pass wins by 7 % at step 1 and 4 % at
// step 2; at step 4 its halo is 2.5 tiles and its 60 KiB of LDS leave two workgroups per CU, and it loses by 20 %.
// A staged pixel outside the image gets the special key, which no filtered pixel carries: the bounds test of a tap is its key test.
#include "denoise.h"

#include "camera_rays.h"
#include "kernels.h"

namespace bm {

namespace {

constexpr int kThreads = 256;
// pixels of the image: width, height <= 65535, so a pixel index is below 2^32
__device__ __forceinline__ size_t pixel_index(int x, int y, int width) { return static_cast<size_t>(y) * static_cast<size_t>(width) + static_cast<size_t>(x); }
__device__ __forceinline__ DnColor color_of(float4 v) { DnColor c = {v.x, v.y, v.z}; return c; }

} // namespace

// accum: (R, G, B, n) per pixel; hits: two float4 per pixel (distance, normal | voxel, level); dst: (c, 1); keys: one word per pixel
__global__ __launch_bounds__(kThreads) void denoise_prepare(const float4* __restrict__ accum, const float4* __restrict__ hits, float4* __restrict__ dst,
															uint32_t* __restrict__ keys, size_t n) {
	const size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) return;
	const float4 a = accum[i];
	const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1];
	const DnColor c = denoise_radiance(a.x, a.y, a.z, a.w);
	keys[i] = denoise_key(a.w, h0.y, h0.z, h0.w, __float_as_int(h1.x), __float_as_int(h1.y), __float_as_int(h1.z), __float_as_int(h1.w));
	dst[i] = make_float4(c.r, c.g, c.b, 1.f);
}

// src: (c, .) -> dst: (c, var).  Tile TW x TH (TW a power of two), TW * TH / 256 pixels per thread.
template <int TW, int TH>
__global__ __launch_bounds__(kThreads) void denoise_moments(const float4* __restrict__ src, const uint32_t* __restrict__ keys, float4* __restrict__ dst,
															int width, int height) {
	constexpr int R = kMomentsRadius, LW = TW + 2 * R, LH = TH + 2 * R;
	__shared__ float s_lum[LW * LH];
	__shared__ uint32_t s_key[LW * LH];
	const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
	for (int e = threadIdx.x; e < LW * LH; e += kThreads) {
		const int lx = e % LW, ly = e / LW;
		const int gx = x0 - R + lx, gy = y0 - R + ly;
		uint32_t key = kDenoiseSpecialKey;
		float lum = 0.f;
		if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
			const size_t q = pixel_index(gx, gy, width);
			key = keys[q];
			lum = denoise_luminance(color_of(src[q]));
		}
		s_key[e] = key;
		s_lum[e] = lum;
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < TW * TH / kThreads; ++k) {
		const int e = threadIdx.x + k * kThreads;
		const int tx = e % TW, ty = e / TW;
		const int x = x0 + tx, y = y0 + ty;
		if (x >= width || y >= height) continue;
		const size_t p = pixel_index(x, y, width);
		float4 v = src[p];
		const uint32_t key_p = s_key[(ty + R) * LW + tx + R];
		if (key_p != kDenoiseSpecialKey) {
			DnMoments total = moments_zero();
#pragma unroll
			for (int dy = 0; dy <= 2 * R; ++dy) {
				DnMoments row = moments_zero();
#pragma unroll
				for (int dx = 0; dx <= 2 * R; ++dx) {
					const int q = (ty + dy) * LW + tx + dx;
					if (s_key[q] == key_p) moments_tap(row, s_lum[q]);
				}
				moments_add_row(total, row);
			}
			v.w = moments_variance(total);
		}
		dst[p] = v;
	}
}

// one a-trous pass at stride STEP, src: (c, var) -> dst: (c', var'), or (c', 1) for the last pass
template <int STEP, int TW, int TH>
__global__ __launch_bounds__(kThreads) void denoise_atrous_tiled(const float4* __restrict__ src, const uint32_t* __restrict__ keys, float4* __restrict__ dst,
																 int width, int height, float sigma_l, int last) {
	constexpr int R = kAtrousRadius * STEP, LW = TW + 2 * R, LH = TH + 2 * R;
	__shared__ float4 s_cv[LW * LH];
	__shared__ float s_lum[LW * LH];
	__shared__ uint32_t s_key[LW * LH];
	const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
	for (int e = threadIdx.x; e < LW * LH; e += kThreads) {
		const int lx = e % LW, ly = e / LW;
		const int gx = x0 - R + lx, gy = y0 - R + ly;
		uint32_t key = kDenoiseSpecialKey;
		float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
		if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
			const size_t q = pixel_index(gx, gy, width);
			key = keys[q];
			v = src[q];
		}
		s_key[e] = key;
		s_cv[e] = v;
		s_lum[e] = denoise_luminance(color_of(v));
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < TW * TH / kThreads; ++k) {
		const int e = threadIdx.x + k * kThreads;
		const int tx = e % TW, ty = e / TW;
		const int x = x0 + tx, y = y0 + ty;
		if (x >= width || y >= height) continue;
		const int pc = (ty + R) * LW + tx + R;
		float4 v = s_cv[pc];
		const uint32_t key_p = s_key[pc];
		if (key_p != kDenoiseSpecialKey) {
			const float l_p = s_lum[pc];
			const float den = atrous_den(sigma_l, v.w);
			DnSum total = atrous_zero();
#pragma unroll
			for (int ky = 0; ky < 5; ++ky) {
				DnSum row = atrous_zero();
#pragma unroll
				for (int kx = 0; kx < 5; ++kx) {
					const int q = (ty + ky * STEP) * LW + tx + kx * STEP;
					if (s_key[q] == key_p) {
						const float4 t = s_cv[q];
						atrous_tap(row, kx, ky, l_p, den, color_of(t), t.w, s_lum[q]);
					}
				}
				atrous_add_row(total, row);
			}
			DnColor c;
			float var;
			atrous_result(total, c, var);
			v = make_float4(c.r, c.g, c.b, var);
		}
		if (last) v.w = 1.f;
		dst[pixel_index(x, y, width)] = v;
	}
}

// the same pass for any stride, taps from global memory: a workgroup is 64 x 4 pixels, a wave one row of 64
__global__ __launch_bounds__(kThreads) void denoise_atrous_far(const float4* __restrict__ src, const uint32_t* __restrict__ keys, float4* __restrict__ dst,
															   int width, int height, int step, float sigma_l, int last) {
	const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (x >= width || y >= height) return;
	const size_t p = pixel_index(x, y, width);
	float4 v = src[p];
	const uint32_t key_p = keys[p];
	if (key_p != kDenoiseSpecialKey) {
		const float l_p = denoise_luminance(color_of(v));
		const float den = atrous_den(sigma_l, v.w);
		DnSum total = atrous_zero();
#pragma unroll
		for (int ky = 0; ky < 5; ++ky) {
			DnSum row = atrous_zero();
			const int qy = y + (ky - kAtrousRadius) * step;
			if (qy >= 0 && qy < height) {
#pragma unroll
				for (int kx = 0; kx < 5; ++kx) {
					const int qx = x + (kx - kAtrousRadius) * step;
					if (qx < 0 || qx >= width) continue;
					const size_t q = pixel_index(qx, qy, width);
					if (keys[q] == key_p) {
						const float4 t = src[q];
						atrous_tap(row, kx, ky, l_p, den, color_of(t), t.w, denoise_luminance(color_of(t)));
					}
				}
			}
			atrous_add_row(total, row);
		}
		DnColor c;
		float var;
		atrous_result(total, c, var);
		v = make_float4(c.r, c.g, c.b, var);
	}
	if (last) v.w = 1.f;
	dst[p] = v;
}

// ray i = y * width + x: the frames' primary ray through the centre of pixel (x, y) without jitter and lens -- pixel_ray_direction
// (camera_rays.h), which bm_camera_pixel_rays (capi.cpp) calls as well, with px = x + 0.5, py = y + 0.5; two float4 per ray (origin, direction.x | direction.y, direction.z, tmax, reserved)
__global__ __launch_bounds__(kThreads) void pixel_rays(const PixelRayBasis b, float4* __restrict__ rays, size_t n) {
	const size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) return;
	const uint32_t width = static_cast<uint32_t>(b.width);
	const uint32_t y = static_cast<uint32_t>(i / width), x = static_cast<uint32_t>(i - static_cast<size_t>(y) * width);
	const float W = static_cast<float>(b.width), H = static_cast<float>(b.height);
	float d[3];
	pixel_ray_direction(b.dir, b.right, b.up, W, H, static_cast<float>(x) + 0.5f, static_cast<float>(y) + 0.5f, d);
	rays[2 * i] = make_float4(b.origin[0], b.origin[1], b.origin[2], d[0]);
	rays[2 * i + 1] = make_float4(d[1], d[2], __int_as_float(0x7F800000), 0.f);
}

// ---- host-callable launchers (kernels.h)
namespace {

constexpr int kTileW = 64, kTileH = 16; // 1024 pixels, 4 per thread

template <int STEP>
void launch_tiled(const float4* src, const uint32_t* keys, float4* dst, int width, int height, float sigma_l, int last, hipStream_t stream) {
	const dim3 grid(static_cast<unsigned>((width + kTileW - 1) / kTileW), static_cast<unsigned>((height + kTileH - 1) / kTileH));
	hipLaunchKernelGGL((denoise_atrous_tiled<STEP, kTileW, kTileH>), grid, dim3(kThreads), 0, stream, src, keys, dst, width, height, sigma_l, last);
}

} // namespace

void launch_denoise(int width, int height, int iterations, float sigma_l, const float* accum, const void* hits, float* out, void* workspace,
					int tiled_max_step, hipStream_t stream, hipEvent_t* marks) {
	int mark = 0;
	auto stamp = [&]() { if (marks) (void)hipEventRecord(marks[mark++], stream); };
	const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
	float4* a = static_cast<float4*>(workspace);
	float4* b = a + n;
	uint32_t* keys = reinterpret_cast<uint32_t*>(b + n);
	const float4* acc4 = reinterpret_cast<const float4*>(accum);
	const float4* hit4 = static_cast<const float4*>(hits);
	float4* out4 = reinterpret_cast<float4*>(out);
	const unsigned blocks = static_cast<unsigned>((n + kThreads - 1) / kThreads);
	stamp();
	hipLaunchKernelGGL(denoise_prepare, dim3(blocks), dim3(kThreads), 0, stream, acc4, hit4, iterations == 0 ? out4 : a, keys, n);
	stamp();
	if (iterations == 0) return;
	const dim3 tiles(static_cast<unsigned>((width + kTileW - 1) / kTileW), static_cast<unsigned>((height + kTileH - 1) / kTileH));
	hipLaunchKernelGGL((denoise_moments<kTileW, kTileH>), tiles, dim3(kThreads), 0, stream, a, keys, b, width, height);
	stamp();
	const float4* src = b;
	float4* spare = a;
	for (int it = 0; it < iterations; ++it) {
		const int last = it == iterations - 1 ? 1 : 0;
		float4* dst = last ? out4 : spare;
		const int step = 1 << it;
		if (step == 1 && step <= tiled_max_step) launch_tiled<1>(src, keys, dst, width, height, sigma_l, last, stream);
		else if (step == 2 && step <= tiled_max_step) launch_tiled<2>(src, keys, dst, width, height, sigma_l, last, stream);
		else {
			const dim3 grid(static_cast<unsigned>((width + 63) / 64), static_cast<unsigned>((height + 3) / 4));
			hipLaunchKernelGGL(denoise_atrous_far, grid, dim3(kThreads), 0, stream, src, keys, dst, width, height, step, sigma_l, last);
		}
		stamp();
		spare = const_cast<float4*>(src);
		src = dst;
	}
}

void launch_pixel_rays(const PixelRayBasis& basis, void* rays, hipStream_t stream) {
	const size_t n = static_cast<size_t>(basis.width) * static_cast<size_t>(basis.height);
	hipLaunchKernelGGL(pixel_rays, dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, basis, static_cast<float4*>(rays), n);
}

} // namespace bm
