// denoise_host.cpp -- bm_host_denoise: the filter of denoise.h as plain loops over host memory, pass by pass as denoise.hip runs it on
// the device.  Needs nothing else of the library (no HIP header, no scene): tests/denoise_check.cpp links this file alone.
#include <cstring>
#include <string>
#include <vector>

#include "../../include/brickmap.h"
#include "denoise.h"

namespace bm {
// the library's error slot (error.h, defined in scene.cpp); absent -- a null address -- in a program that links this file alone
__attribute__((weak)) void set_error(const std::string& msg);
} // namespace bm

namespace {

int refuse(const char* why) {
	if (bm::set_error) bm::set_error(std::string("bm_host_denoise: ") + why);
	return BM_EINVAL;
}

struct Px { bm::DnColor c; float var; };

} // namespace

extern "C" int bm_host_denoise(const bm_denoise_params* params, const float* accum, const bm_ray_hit* hits, float* out) {
	using namespace bm;
	if (!params || !accum || !hits || !out) return refuse("null argument");
	const DenoiseParamsView pv = {params->width, params->height, params->iterations, params->sigma_l, params->flags, params->reserved};
	if (const char* why = denoise_params_problem(pv)) return refuse(why);
	const int W = params->width, H = params->height;
	const size_t N = static_cast<size_t>(W) * static_cast<size_t>(H);
	std::vector<Px> a(N), b(N);
	std::vector<uint32_t> key(N);
	// prepare
	for (size_t i = 0; i < N; ++i) {
		const float* p = accum + 4 * i;
		const bm_ray_hit& h = hits[i];
		a[i].c = denoise_radiance(p[0], p[1], p[2], p[3]);
		a[i].var = 1.f;
		key[i] = denoise_key(p[3], h.normal[0], h.normal[1], h.normal[2], h.voxel[0], h.voxel[1], h.voxel[2], h.level);
	}
	if (params->iterations > 0) {
		// moments: a -> b
		for (int y = 0; y < H; ++y)
			for (int x = 0; x < W; ++x) {
				const size_t i = static_cast<size_t>(y) * W + x;
				b[i] = a[i];
				if (key[i] == kDenoiseSpecialKey) continue;
				DnMoments total = moments_zero();
				for (int dy = -kMomentsRadius; dy <= kMomentsRadius; ++dy) {
					DnMoments row = moments_zero();
					const int qy = y + dy;
					if (qy >= 0 && qy < H)
						for (int dx = -kMomentsRadius; dx <= kMomentsRadius; ++dx) {
							const int qx = x + dx;
							if (qx < 0 || qx >= W) continue;
							const size_t q = static_cast<size_t>(qy) * W + qx;
							if (key[q] == key[i]) moments_tap(row, denoise_luminance(a[q].c));
						}
					moments_add_row(total, row);
				}
				b[i].var = moments_variance(total);
			}
		// a-trous: b -> a -> b ...
		std::vector<Px>* src = &b;
		std::vector<Px>* dst = &a;
		for (int it = 0; it < params->iterations; ++it) {
			const long long step = 1ll << it;
			for (int y = 0; y < H; ++y)
				for (int x = 0; x < W; ++x) {
					const size_t i = static_cast<size_t>(y) * W + x;
					(*dst)[i] = (*src)[i];
					if (key[i] == kDenoiseSpecialKey) continue;
					const float l_p = denoise_luminance((*src)[i].c);
					const float den = atrous_den(params->sigma_l, (*src)[i].var);
					DnSum total = atrous_zero();
					for (int ky = 0; ky < 5; ++ky) {
						DnSum row = atrous_zero();
						const long long qy = y + (ky - kAtrousRadius) * step;
						if (qy >= 0 && qy < H)
							for (int kx = 0; kx < 5; ++kx) {
								const long long qx = x + (kx - kAtrousRadius) * step;
								if (qx < 0 || qx >= W) continue;
								const size_t q = static_cast<size_t>(qy) * W + static_cast<size_t>(qx);
								if (key[q] != key[i]) continue;
								const Px& t = (*src)[q];
								atrous_tap(row, kx, ky, l_p, den, t.c, t.var, denoise_luminance(t.c));
							}
						atrous_add_row(total, row);
					}
					atrous_result(total, (*dst)[i].c, (*dst)[i].var);
				}
			std::swap(src, dst);
		}
		if (src != &a) a.swap(b);
	}
	for (size_t i = 0; i < N; ++i) {
		out[4 * i + 0] = a[i].c.r; out[4 * i + 1] = a[i].c.g; out[4 * i + 2] = a[i].c.b; out[4 * i + 3] = 1.f;
	}
	return 0;
}
