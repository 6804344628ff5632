// reproject_check.cpp -- a program of its own around the host routine (csrc/reproject_host.cpp, linked alone: no device, no scene):
// random images, histories, hit records and camera pairs through bm_host_reproject, every result checked for what must hold whatever
// the numbers -- every key is the pixel's denoise_key, a pixel with the special key and every pixel of a call without a history is the
// frame's own value bit for bit, nothing is non-finite for finite input, a pixel takes at most max_history samples over and never
// loses one -- and every refusal refused.  tests/test_reproject_host.py builds it plain and under the address and undefined-behaviour
// sanitizers.
//   usage: reproject_check <images>      prints "images N pixels N special N history N refused N failures N"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../include/brickmap.h"
#include "../brickmap_amd/csrc/reproject.h"

static long long failures = 0;
#define CHECK(cond, ...)                                            \
	do {                                                            \
		if (!(cond)) {                                              \
			if (failures++ < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
		}                                                           \
	} while (0)

int main(int argc, char** argv) {
	const int images = argc > 1 ? std::atoi(argv[1]) : 20;
	std::mt19937 rng(4711);
	auto uni = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
	auto real = [&](float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(rng); };
	std::exponential_distribution<float> noise(1.6f);
	long long pixels = 0, special = 0, history = 0, refused = 0;
	for (int im = 0; im < images; ++im) {
		// sizes: single rows and columns, single pixels, and larger ones
		const int W = im % 7 == 0 ? 1 : (im % 7 == 1 ? uni(1, 6) : uni(7, 90)), H = im % 5 == 0 ? 1 : (im % 5 == 1 ? uni(1, 6) : uni(7, 60));
		const size_t N = static_cast<size_t>(W) * H;
		bm_reproject_params p{};
		p.width = W; p.height = H; p.max_history = im % 3 == 0 ? 1.f : (im % 3 == 1 ? 4.5f : 32.f);
		// the current camera looks down at the plane z = 0 from above; the previous one is a small or a large move away, or looks elsewhere
		bm_camera cam{}, before{};
		cam.position[0] = real(-20.f, 20.f); cam.position[1] = real(-20.f, 20.f); cam.position[2] = real(20.f, 60.f);
		const float dx = real(-0.4f, 0.4f), dy = real(-0.4f, 0.4f), inv = 1.f / std::sqrt(dx * dx + dy * dy + 1.f);
		cam.direction[0] = dx * inv; cam.direction[1] = dy * inv; cam.direction[2] = -inv;
		cam.up[1] = 1.f;
		before = cam;
		const int move = im % 6;
		if (move == 1) before.position[0] += real(-2.f, 2.f);
		if (move == 2) { before.position[2] += real(-5.f, 5.f); before.position[1] += real(-1.f, 1.f); }
		if (move == 3) for (int k = 0; k < 3; ++k) before.direction[k] = -cam.direction[k];       // everything behind it
		if (move == 4) { // far along its own right axis, cross(direction, up): everything outside its image
			before.position[0] += -1e6f * cam.direction[2];
			before.position[2] += 1e6f * cam.direction[0];
		}
		if (move == 5) { before.direction[0] = 0.f; before.direction[1] = 1.f; before.direction[2] = 0.f; } // parallel to up: NaNs
		// exact-size allocations, so that the address sanitizer sees a read or write one element past either end
		std::vector<float> accum(4 * N), prev(5 * N), out(5 * N, std::numeric_limits<float>::quiet_NaN());
		std::vector<bm_ray_hit> hits(N);
		uint32_t* prev_keys = reinterpret_cast<uint32_t*>(prev.data() + 4 * N);
		const uint32_t plane_key = bm::denoise_key(1.f, 0.f, 0.f, 1.f, 0, 0, -1, 2); // the plane z = 0 seen from above
		for (size_t i = 0; i < N; ++i) {
			const int kind = uni(0, 15);
			const float n = kind == 0 ? 0.f : static_cast<float>(uni(1, 3));
			for (int k = 0; k < 3; ++k) accum[4 * i + k] = noise(rng) * n;
			accum[4 * i + 3] = n;
			bm_ray_hit& h = hits[i];
			h.distance = real(15.f, 90.f);
			h.normal[0] = h.normal[1] = 0.f; h.normal[2] = 1.f;
			h.voxel[0] = uni(0, 99); h.voxel[1] = uni(0, 99); h.voxel[2] = kind == 4 ? 7 : -1; // kind 4: another plane
			h.level = 2;
			if (kind == 1) { h.level = -1; h.distance = std::numeric_limits<float>::infinity(); h.voxel[0] = h.voxel[1] = h.voxel[2] = -1; h.normal[2] = 0.f; }
			if (kind == 2) h.level = 3;
			if (kind == 3) h.normal[2] = 0.f;
			const int pk = uni(0, 9);
			const float pn = pk == 0 ? 0.f : real(0.25f, 48.f);
			for (int k = 0; k < 3; ++k) prev[4 * i + k] = noise(rng) * pn;
			prev[4 * i + 3] = pn;
			prev_keys[i] = pk == 1 ? bm::kDenoiseSpecialKey : (pk == 2 ? plane_key + 8 : plane_key);
		}
		const bool with_history = im % 4 != 3;
		const int e = bm_host_reproject(&p, &cam, with_history ? &before : nullptr, accum.data(), hits.data(), with_history ? prev.data() : nullptr, out.data());
		CHECK(e == 0, "image %d (%d x %d): error %d", im, W, H, e);
		if (e) continue;
		const uint32_t* out_keys = reinterpret_cast<const uint32_t*>(out.data() + 4 * N);
		long long took = 0;
		for (size_t i = 0; i < N; ++i) {
			const bm_ray_hit& h = hits[i];
			const float* a = &accum[4 * i];
			const float* o = &out[4 * i];
			const uint32_t key = bm::denoise_key(a[3], h.normal[0], h.normal[1], h.normal[2], h.voxel[0], h.voxel[1], h.voxel[2], h.level);
			CHECK(out_keys[i] == key, "image %d pixel %zu: key %u, expected %u", im, i, out_keys[i], key);
			const bool copied = std::memcmp(a, o, 16) == 0;
			if (key == bm::kDenoiseSpecialKey || !with_history || move >= 3) CHECK(copied, "image %d pixel %zu: not the frame's own value", im, i);
			for (int k = 0; k < 4; ++k) CHECK(std::isfinite(o[k]), "image %d pixel %zu: not finite", im, i);
			CHECK(o[3] >= a[3] && o[3] <= p.max_history + a[3], "image %d pixel %zu: n %g from %g", im, i, o[3], a[3]);
			for (int k = 0; k < 3; ++k) CHECK(o[k] >= a[k], "image %d pixel %zu: radiance was taken away", im, i);
			if (o[3] > a[3]) took++;
			pixels++;
			if (key == bm::kDenoiseSpecialKey) special++;
		}
		history += took;
	}
	// refusals: nothing is written
	{
		float accum[4] = {1, 1, 1, 1}, prev[5] = {1, 1, 1, 1, 0}, out[5] = {-7, -7, -7, -7, -7};
		bm_ray_hit hit{};
		hit.normal[2] = 1.f; hit.level = 2; hit.distance = 3.f;
		bm_camera cam{};
		cam.direction[0] = 1.f; cam.up[2] = 1.f;
		auto refuse = [&](bm_reproject_params p, const bm_camera* c, const bm_camera* cp, const float* a, const bm_ray_hit* h, const void* pv, void* o) {
			const int e = bm_host_reproject(&p, c, cp, a, h, pv, o);
			CHECK(e == BM_EINVAL && out[0] == -7.f && out[4] == -7.f, "a refusal was not refused (error %d)", e);
			refused++;
		};
		const bm_reproject_params ok = {1, 1, 32.f, 0, 0};
		bm_reproject_params p;
		p = ok; p.width = 0; refuse(p, &cam, &cam, accum, &hit, prev, out);
		p = ok; p.height = 65536; refuse(p, &cam, &cam, accum, &hit, prev, out);
		p = ok; p.max_history = 0.5f; refuse(p, &cam, &cam, accum, &hit, prev, out);
		p = ok; p.max_history = std::numeric_limits<float>::infinity(); refuse(p, &cam, &cam, accum, &hit, prev, out);
		p = ok; p.max_history = std::numeric_limits<float>::quiet_NaN(); refuse(p, &cam, &cam, accum, &hit, prev, out);
		p = ok; p.flags = 2; refuse(p, &cam, &cam, accum, &hit, prev, out);
		p = ok; p.reserved = 1; refuse(p, &cam, &cam, accum, &hit, prev, out);
		refuse(ok, nullptr, &cam, accum, &hit, prev, out);
		refuse(ok, &cam, nullptr, accum, &hit, prev, out);
		refuse(ok, &cam, &cam, nullptr, &hit, prev, out);
		refuse(ok, &cam, &cam, accum, nullptr, prev, out);
		refuse(ok, &cam, &cam, accum, &hit, prev, nullptr);
		CHECK(bm_host_reproject(nullptr, &cam, &cam, accum, &hit, prev, out) == BM_EINVAL, "null params");
		CHECK(bm_host_reproject(&ok, &cam, nullptr, accum, &hit, nullptr, out) == 0 && out[0] == 1.f && out[3] == 1.f, "the good call");
	}
	std::printf("images %d pixels %lld special %lld history %lld refused %lld failures %lld\n", images, pixels, special, history, refused, failures);
	return failures ? 1 : 0;
}
