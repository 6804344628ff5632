// denoise_check.cpp -- a program of its own around the host filter (csrc/denoise_host.cpp, linked alone: no device, no scene): random
// images with random surfaces, sizes and pass counts through bm_host_denoise, every result checked for what must hold whatever the
// noise -- special pixels come out as (c, 1), nothing is non-finite, alpha is 1, a pixel that shares its surface with nobody keeps its
// radiance, a filtered pixel stays within the range of its surface's radiance (every pass is a convex combination), zero passes give
// (c, 1) -- and every refusal refused.  tests/test_denoise_host.py builds it plain and under the address and undefined-behaviour sanitizers.
//   usage: denoise_check <images>      prints "images N pixels N special N filtered N refused N failures N"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>
#include <vector>

#include "../include/brickmap.h"
#include "../brickmap_amd/csrc/denoise.h"

static long long failures = 0;
#define CHECK(cond, ...)                                            \
	do {                                                            \
		if (!(cond)) {                                              \
			if (failures++ < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
		}                                                           \
	} while (0)

int main(int argc, char** argv) {
	const int images = argc > 1 ? std::atoi(argv[1]) : 20;
	std::mt19937 rng(12345);
	auto uni = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
	std::exponential_distribution<float> noise(1.6f);
	long long pixels = 0, special = 0, filtered = 0, refused = 0;
	for (int im = 0; im < images; ++im) {
		// sizes: single rows and columns, single pixels, images narrower than the windows, and larger ones
		const int W = im % 7 == 0 ? 1 : (im % 7 == 1 ? uni(1, 6) : uni(7, 90)), H = im % 5 == 0 ? 1 : (im % 5 == 1 ? uni(1, 6) : uni(7, 60));
		const size_t N = static_cast<size_t>(W) * H;
		bm_denoise_params p{};
		p.width = W; p.height = H; p.iterations = im % 9; p.sigma_l = im % 3 == 0 ? 0.25f : (im % 3 == 1 ? 4.f : 100.f);
		// exact-size allocations, so that the address sanitizer sees a read or write one element past either end
		std::vector<float> accum(4 * N), out(4 * N, std::numeric_limits<float>::quiet_NaN());
		std::vector<bm_ray_hit> hits(N);
		const int surfaces = uni(1, 5);
		for (size_t i = 0; i < N; ++i) {
			const int x = static_cast<int>(i % W), y = static_cast<int>(i / W);
			const int kind = uni(0, 15);
			const float n = kind == 0 ? 0.f : static_cast<float>(uni(1, 3));
			for (int k = 0; k < 3; ++k) accum[4 * i + k] = noise(rng) * n;
			accum[4 * i + 3] = n;
			bm_ray_hit& h = hits[i];
			const int s = ((x * surfaces) / W + (y * 2) / H) % surfaces; // blocks of surfaces
			const int axis = s % 3;
			h.distance = 5.f;
			h.normal[0] = h.normal[1] = h.normal[2] = 0.f;
			h.normal[axis] = s & 1 ? 1.f : -1.f;
			h.voxel[0] = 8 * x; h.voxel[1] = 8 * y; h.voxel[2] = 16;
			h.level = uni(0, 2);
			const int size = h.level == 2 ? 1 : (h.level == 1 ? 4 : 8);
			h.voxel[axis] = 100 * s + 40 - (s & 1 ? size : 0); // one plane per surface, whatever the level
			if (kind == 1) { h.level = -1; h.distance = std::numeric_limits<float>::infinity(); h.voxel[0] = h.voxel[1] = h.voxel[2] = -1; h.normal[axis] = 0.f; }
			if (kind == 2) h.level = 3;
			if (kind == 3) h.normal[axis] = 0.f;
		}
		// one pixel that shares its surface with nobody
		const size_t lone = N - 1;
		hits[lone].level = 2; hits[lone].normal[0] = 1.f; hits[lone].normal[1] = hits[lone].normal[2] = 0.f; hits[lone].voxel[0] = 99999;
		accum[4 * lone] = 3.f; accum[4 * lone + 1] = 2.f; accum[4 * lone + 2] = 1.f; accum[4 * lone + 3] = 2.f;
		const int e = bm_host_denoise(&p, accum.data(), hits.data(), out.data());
		CHECK(e == 0, "image %d (%d x %d, %d passes): error %d", im, W, H, p.iterations, e);
		if (e) continue;
		// per surface key: range of the radiance over its pixels
		std::map<uint32_t, std::pair<float, float>> range[3];
		std::vector<uint32_t> key(N);
		for (size_t i = 0; i < N; ++i) {
			const bm_ray_hit& h = hits[i];
			key[i] = bm::denoise_key(accum[4 * i + 3], h.normal[0], h.normal[1], h.normal[2], h.voxel[0], h.voxel[1], h.voxel[2], h.level);
			for (int k = 0; k < 3; ++k) {
				const float c = accum[4 * i + 3] > 0.f ? accum[4 * i + k] / accum[4 * i + 3] : 0.f;
				auto it = range[k].find(key[i]);
				if (it == range[k].end()) range[k][key[i]] = {c, c};
				else { it->second.first = std::fmin(it->second.first, c); it->second.second = std::fmax(it->second.second, c); }
			}
		}
		for (size_t i = 0; i < N; ++i) {
			const float n = accum[4 * i + 3];
			CHECK(out[4 * i + 3] == 1.f, "image %d pixel %zu: alpha %g", im, i, out[4 * i + 3]);
			for (int k = 0; k < 3; ++k) {
				const float c = n > 0.f ? accum[4 * i + k] / n : 0.f, o = out[4 * i + k];
				CHECK(std::isfinite(o), "image %d pixel %zu: not finite", im, i);
				if (key[i] == bm::kDenoiseSpecialKey || p.iterations == 0 || i == lone) CHECK(o == c, "image %d pixel %zu: %g, expected its own radiance %g", im, i, o, c);
				else {
					const auto& r = range[k][key[i]];
					const float slack = 1e-5f * (1.f + std::fabs(r.second));
					CHECK(o >= r.first - slack && o <= r.second + slack, "image %d pixel %zu: %g outside its surface's range [%g, %g]", im, i, o, r.first, r.second);
				}
			}
			pixels++;
			if (key[i] == bm::kDenoiseSpecialKey) special++; else filtered++;
		}
	}
	// refusals: nothing is written
	{
		float accum[4] = {1, 1, 1, 1}, out[4] = {-7, -7, -7, -7};
		bm_ray_hit hit{};
		hit.normal[2] = 1.f; hit.level = 2;
		auto refuse = [&](bm_denoise_params p, const float* a, const bm_ray_hit* h, float* o) {
			const int e = bm_host_denoise(&p, a, h, o);
			CHECK(e == BM_EINVAL && out[0] == -7.f, "a refusal was not refused (error %d)", e);
			refused++;
		};
		const bm_denoise_params ok = {1, 1, 5, 4.f, 0, 0};
		bm_denoise_params p;
		p = ok; p.iterations = -1; refuse(p, accum, &hit, out);
		p = ok; p.iterations = 9; refuse(p, accum, &hit, out);
		p = ok; p.sigma_l = 0.f; refuse(p, accum, &hit, out);
		p = ok; p.sigma_l = -2.f; refuse(p, accum, &hit, out);
		p = ok; p.sigma_l = std::numeric_limits<float>::infinity(); refuse(p, accum, &hit, out);
		p = ok; p.sigma_l = std::numeric_limits<float>::quiet_NaN(); refuse(p, accum, &hit, out);
		p = ok; p.width = 0; refuse(p, accum, &hit, out);
		p = ok; p.height = 65536; refuse(p, accum, &hit, out);
		p = ok; p.flags = 2; refuse(p, accum, &hit, out);
		p = ok; p.reserved = 1; refuse(p, accum, &hit, out);
		refuse(ok, nullptr, &hit, out);
		refuse(ok, accum, nullptr, out);
		refuse(ok, accum, &hit, nullptr);
		CHECK(bm_host_denoise(nullptr, accum, &hit, out) == BM_EINVAL, "null params");
		CHECK(bm_host_denoise(&ok, accum, &hit, out) == 0 && out[0] == 1.f && out[3] == 1.f, "the good call");
	}
	std::printf("images %d pixels %lld special %lld filtered %lld refused %lld failures %lld\n", images, pixels, special, filtered, refused, failures);
	return failures ? 1 : 0;
}
