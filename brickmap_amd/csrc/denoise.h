// denoise.h -- the edge-avoiding a-trous filter of 1-spp frames (bm_denoise / bm_host_denoise): the per-pixel rules, written once.
// Plain C++ (host + device) like escape.h and jump.h: the kernels of denoise.hip and the loops of denoise_host.cpp call these functions
// and add nothing of their own to the arithmetic, so the device result equals the host result bit for bit -- fp32 IEEE + - * / sqrt in
// the order written here, no contraction (-ffp-contract=off), no exp: the luminance weight is rational.  DESIGN.md 4.12 has the spec.
//
// A frame is filtered in passes over a width x height image, row-major.  Every pass reads one image and the keys and writes another:
//   prepare   accumulation (R, G, B, n) + first hit  ->  (c, 1) and the pixel's surface key
//   moments   7x7 window at stride 1                 ->  (c, var): variance of the luminance over the taps of the same surface
//   a-trous   5x5 window at stride 2^i, i = 0 ...    ->  (c', var')
// A tap counts only if it lies inside the image and carries the key of the centre pixel; a skipped tap adds nothing (it is not
// multiplied by zero).  Sums run left to right within a row starting from 0.0f, and the row sums are added top to bottom onto 0.0f.
// Special pixels (no sample, a miss, a brick that is not resident, a ray that starts inside a voxel) carry the reserved key: they are
// copied, never filtered and never a tap of another pixel.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BM_DHD __host__ __device__ __forceinline__
#else
#define BM_DHD inline
#endif

namespace bm {

constexpr uint32_t kDenoiseSpecialKey = 0xFFFFFFFFu;
constexpr int kDenoiseMaxIterations = 8;
constexpr int kMomentsRadius = 3; // 7x7
constexpr int kAtrousRadius = 2;  // 5x5

struct DnColor { float r, g, b; };

// c = (R / n, G / n, B / n), or black for a pixel without a terminated path
BM_DHD DnColor denoise_radiance(float R, float G, float B, float n) {
	DnColor c = {0.f, 0.f, 0.f};
	if (n > 0.f) { c.r = R / n; c.g = G / n; c.b = B / n; }
	return c;
}

BM_DHD float denoise_luminance(DnColor c) { return (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b; }

// The surface a pixel sees, as one integer.  In a voxel world every face lies in an axis-aligned integer plane: the entry normal of the
// walk is minus the sign of the move that entered the cell (traverse.h process_candidate / intersect_grid), so a positive normal means the
// ray came in through the cell's HIGH face, voxel + size, and a negative one through its low face, voxel.  Cells of different LoD levels
// (sizes 8, 4, 1 for levels 0, 1, 2) whose entry faces lie in one plane and face the same way get the same key.  The axis is the first
// one whose normal component is not zero (a ray that enters the world box through an edge may carry two).
BM_DHD uint32_t denoise_key(float n, float nx, float ny, float nz, int vx, int vy, int vz, int level) {
	if (!(n > 0.f) || level < 0 || level > 2) return kDenoiseSpecialKey;
	const int a = nx != 0.f ? 0 : (ny != 0.f ? 1 : (nz != 0.f ? 2 : -1));
	if (a < 0) return kDenoiseSpecialKey;
	const float na = a == 0 ? nx : (a == 1 ? ny : nz);
	const uint32_t s = na > 0.f ? 1u : 0u;
	const int size = level == 2 ? 1 : (level == 1 ? 4 : 8);
	const int v = a == 0 ? vx : (a == 1 ? vy : vz);
	const uint32_t plane = static_cast<uint32_t>(v + (s ? size : 0));
	return plane * 8u + static_cast<uint32_t>(a) * 2u + s;
}

// ---- the variance pass: one row of taps is summed into a DnMoments that starts at zero, the rows are then added top to bottom
struct DnMoments { float n, s1, s2; };
BM_DHD DnMoments moments_zero() { DnMoments m = {0.f, 0.f, 0.f}; return m; }
BM_DHD void moments_tap(DnMoments& row, float l) { row.n += 1.f; row.s1 += l; row.s2 += l * l; }
BM_DHD void moments_add_row(DnMoments& total, const DnMoments& row) { total.n += row.n; total.s1 += row.s1; total.s2 += row.s2; }
// max(0, S2 / N - (S1 / N)^2); N >= 1: the centre pixel is a tap of its own.  (the comparison, not fmax: a NaN gives 0 on both sides)
BM_DHD float moments_variance(const DnMoments& m) {
	const float mean = m.s1 / m.n;
	const float v = m.s2 / m.n - mean * mean;
	return v > 0.f ? v : 0.f;
}

// ---- an a-trous pass
BM_DHD float atrous_h(int k) { return k == 2 ? 0.375f : ((k == 1 || k == 3) ? 0.25f : 0.0625f); } // (1/16, 1/4, 3/8, 1/4, 1/16)
BM_DHD float atrous_den(float sigma_l, float var_p) { return sigma_l * sqrtf(var_p) + 1e-4f; }
struct DnSum { float w, r, g, b, v; };
BM_DHD DnSum atrous_zero() { DnSum s = {0.f, 0.f, 0.f, 0.f, 0.f}; return s; }
// the tap in kernel column kx, row ky (0 ... 4): l_p, den_p belong to the centre pixel; c_q, var_q, l_q to the tap
BM_DHD void atrous_tap(DnSum& row, int kx, int ky, float l_p, float den_p, DnColor c_q, float var_q, float l_q) {
	const float x = fabsf(l_p - l_q) / den_p;
	const float t = 1.f + x;
	const float w = (atrous_h(ky) * atrous_h(kx)) / (t * t);
	row.w += w;
	row.r += w * c_q.r;
	row.g += w * c_q.g;
	row.b += w * c_q.b;
	row.v += (w * w) * var_q;
}
BM_DHD void atrous_add_row(DnSum& total, const DnSum& row) { total.w += row.w; total.r += row.r; total.g += row.g; total.b += row.b; total.v += row.v; }
// c' = C / W, var' = V / (W * W); W > 0: the centre tap has weight 9/64
BM_DHD void atrous_result(const DnSum& s, DnColor& c, float& var) {
	c.r = s.r / s.w; c.g = s.g / s.w; c.b = s.b / s.w;
	var = s.v / (s.w * s.w);
}

// ---- what both routes refuse (BM_EINVAL): returns the reason, or null for parameters that are fine
struct DenoiseParamsView { int width, height, iterations; float sigma_l; uint32_t flags, reserved; };
inline const char* denoise_params_problem(const DenoiseParamsView& p) {
	if (p.width < 1 || p.height < 1 || p.width > 65535 || p.height > 65535) return "width and height must be 1 ... 65535";
	if (p.iterations < 0 || p.iterations > kDenoiseMaxIterations) return "iterations must be 0 ... 8";
	if (!(p.sigma_l > 0.f) || !(p.sigma_l <= 3.402823466e38f)) return "sigma_l must be finite and positive";
	if (p.flags != 0 || p.reserved != 0) return "flags and reserved must be 0";
	return nullptr;
}
// workspace of bm_denoise: two float4 images, then the keys
inline size_t denoise_workspace_bytes(int width, int height) { return static_cast<size_t>(width) * static_cast<size_t>(height) * 36; }

} // namespace bm
