// reproject_host.cpp -- bm_host_reproject: the temporal accumulation of reproject.h as plain loops over host memory, pixel by pixel as
// reproject.hip runs it on the device.  Needs nothing else of the library (no HIP header, no scene): tests/reproject_check.cpp links this
// file alone.
#include <string>

#include "../../include/brickmap.h"
#include "reproject.h"

namespace bm {
// the library's error slot (error.h, defined in scene.cpp); absent -- a null address -- in a program that links this file alone
__attribute__((weak)) void set_error(const std::string& msg);
} // namespace bm

namespace {

int refuse(const char* why) {
	if (bm::set_error) bm::set_error(std::string("bm_host_reproject: ") + why);
	return BM_EINVAL;
}

} // namespace

extern "C" int bm_host_reproject(const bm_reproject_params* params, const bm_camera* camera, const bm_camera* camera_prev, const float* accum,
								 const bm_ray_hit* hits, const void* history_prev, void* history_out) {
	using namespace bm;
	if (!params || !camera || !accum || !hits || !history_out) return refuse("null argument");
	if (history_prev && !camera_prev) return refuse("a previous history needs the camera it was made with");
	const ReprojectParamsView pv = {params->width, params->height, params->max_history, params->flags, params->reserved};
	if (const char* why = reproject_params_problem(pv)) return refuse(why);
	const int width = params->width, height = params->height;
	const size_t N = static_cast<size_t>(width) * static_cast<size_t>(height);
	const float W = static_cast<float>(width), H = static_cast<float>(height);
	const CameraBasis cur = camera_basis(camera->position, camera->direction, camera->up, width, height);
	const bm_camera* before = history_prev ? camera_prev : camera; // (not read without a history)
	const RpPrevCamera prev = reproject_prev_camera(camera_basis(before->position, before->direction, before->up, width, height));
	const float* prev_image = static_cast<const float*>(history_prev);
	const uint32_t* prev_keys = history_prev ? reinterpret_cast<const uint32_t*>(prev_image + 4 * N) : nullptr;
	float* out_image = static_cast<float*>(history_out);
	uint32_t* out_keys = reinterpret_cast<uint32_t*>(out_image + 4 * N);
	for (int y = 0; y < height; ++y)
		for (int x = 0; x < width; ++x) {
			const size_t i = static_cast<size_t>(y) * width + x;
			const float* a = accum + 4 * i;
			const bm_ray_hit& h = hits[i];
			const uint32_t key_p = denoise_key(a[3], h.normal[0], h.normal[1], h.normal[2], h.voxel[0], h.voxel[1], h.voxel[2], h.level);
			out_keys[i] = key_p;
			float* out = out_image + 4 * i;
			for (int k = 0; k < 4; ++k) out[k] = a[k];
			if (!history_prev || key_p == kDenoiseSpecialKey) continue;
			float u, v;
			RpTaps taps;
			if (!reproject_project(cur, prev, W, H, x, y, h.distance, u, v) || !reproject_taps(u, v, W, H, taps)) continue;
			RpSum sum = reproject_zero();
			for (int k = 0; k < 4; ++k) {
				const int qx = taps.x0 + (k & 1), qy = taps.y0 + (k >> 1);
				const bool inside = qx >= 0 && qx < width && qy >= 0 && qy < height;
				const size_t q = inside ? static_cast<size_t>(qy) * width + qx : 0;
				const float* t = prev_image + 4 * q;
				reproject_tap(sum, inside, prev_keys[q], key_p, taps.w[k], t[0], t[1], t[2], t[3]);
			}
			reproject_blend(sum, params->max_history, a, out);
		}
	return 0;
}
