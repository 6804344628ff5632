// camera_rays.h -- the view basis of a frame and the direction of the ray through a pixel position, each written once.
// Plain C++ (host + device) like denoise.h.  The basis is the frames' (fill_frame_constants calls camera_basis); the direction is
// the frames' primary ray without jitter and lens, which bm_camera_pixel_rays (capi.cpp), the pixel_rays kernel (denoise.hip) and the
// reprojection (reproject.h) share: fp32 IEEE operations in the order written here, no contraction (-ffp-contract=off).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BM_DHD __host__ __device__ __forceinline__
#else
#define BM_DHD inline
#endif

namespace bm {

struct CameraBasis {
	float origin[3], dir[3], right[3], up[3];
};

// launch_kernels:384-385 in GLM's operation order: right = normalize(cross(dir, up)) * 1.5 * aspect, up = normalize(cross(right, dir)) * 1.5
// with cross(x, y) = (x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y) and normalize(v) = v * (1 / sqrt((x*x + y*y) + z*z))
inline CameraBasis camera_basis(const float position[3], const float direction[3], const float up_hint[3], int width, int height) {
	const float aspect = static_cast<float>(width) / static_cast<float>(height);
	auto cross = [](const float* x, const float* y, float* out) {
		out[0] = x[1] * y[2] - y[1] * x[2];
		out[1] = x[2] * y[0] - y[2] * x[0];
		out[2] = x[0] * y[1] - y[0] * x[1];
	};
	auto normalize = [](float* v) {
		const float inv = 1.0f / std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
		for (int k = 0; k < 3; ++k) v[k] = v[k] * inv;
	};
	CameraBasis b;
	cross(direction, up_hint, b.right);
	normalize(b.right);
	for (int k = 0; k < 3; ++k) b.right[k] = (b.right[k] * 1.5f) * aspect;
	cross(b.right, direction, b.up);
	normalize(b.up);
	for (int k = 0; k < 3; ++k) {
		b.up[k] = b.up[k] * 1.5f;
		b.dir[k] = direction[k];
		b.origin[k] = position[k];
	}
	return b;
}

// primary_ray (traverse.h) with the jitter replaced: pixel x covers ppx in (x - 1, x], so ppx = px - 1; (x + 0.5, y + 0.5) is the centre
// of pixel (x, y).  W, H: the frame's size as floats.  out = normalize(dir + right * ni + up * nj)
BM_DHD void pixel_ray_direction(const float dir[3], const float right[3], const float up[3], float W, float H, float px, float py, float out[3]) {
	const float ppx = px - 1.f, ppy = py - 1.f;
	const float ni = (ppx / W) - 0.5f;
	const float nj = ((H - ppy) / H) - 0.5f;
	float v[3];
	for (int k = 0; k < 3; ++k) v[k] = (dir[k] + right[k] * ni) + up[k] * nj;
	const float inv = 1.0f / sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
	for (int k = 0; k < 3; ++k) out[k] = v[k] * inv;
}

} // namespace bm
