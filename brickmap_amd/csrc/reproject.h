// reproject.h -- temporal accumulation for a moving camera (bm_reproject / bm_host_reproject): the per-pixel rules, written once.
// Plain C++ (host + device) like denoise.h: the kernel of reproject.hip and the loops of reproject_host.cpp call these functions and add
// nothing of their own to the arithmetic, so the device result equals the host result bit for bit -- fp32 IEEE + - * / sqrt floor in
// the order written here, no contraction (-ffp-contract=off).  DESIGN.md 4.13 has the spec.
//
// A history of a width x height image is one buffer: width * height float4 (R, G, B, n) row-major -- an accumulation buffer -- then
// width * height uint32 surface keys (denoise_key).  Per pixel p of the frame just rendered:
//   key      key_p = denoise_key of the pixel's first hit; always written to the new history
//   project  P = o + dhat * distance, the point the pixel's centre ray hit; (u, v) = where the PREVIOUS camera saw P, in continuous
//            pixel coordinates in which pixel centres are integers
//   taps     the four pixels around (u, v) with bilinear weights; a tap counts only if it lies inside the image, carries key_p, holds
//            samples (n > 0) and has a weight > 0 -- a skipped tap adds nothing (it is not multiplied by zero)
//   blend    history radiance c_h and sample count n_h (at most max_history) of the counted taps; out = c_h * n_h + accum, n_h + accum.n
// A surface is an exact integer key and the previous camera's ray through a point P of an axis-aligned plane meets that plane only in P,
// so "the previous pixel carries the same key" is an exact disocclusion test: no depth or normal threshold.  A pixel without history --
// no previous frame, a special key, P behind or outside the previous view, no tap that counts -- is the frame's own value, unchanged.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "camera_rays.h"
#include "denoise.h"

namespace bm {

// the previous camera: its basis and the squared lengths of its axes, each (x*x + y*y) + z*z
struct RpPrevCamera {
	CameraBasis b;
	float dd, rr, uu;
};
inline RpPrevCamera reproject_prev_camera(const CameraBasis& b) {
	RpPrevCamera p;
	p.b = b;
	p.dd = (b.dir[0] * b.dir[0] + b.dir[1] * b.dir[1]) + b.dir[2] * b.dir[2];
	p.rr = (b.right[0] * b.right[0] + b.right[1] * b.right[1]) + b.right[2] * b.right[2];
	p.uu = (b.up[0] * b.up[0] + b.up[1] * b.up[1]) + b.up[2] * b.up[2];
	return p;
}

// where the previous camera saw the point that pixel (x, y)'s centre ray of the current camera hit at `distance`: (u, v), the inverse of
// ni = ppx / W - 0.5, nj = (H - ppy) / H - 0.5 with ppx = px - 1 (dir, right and up are mutually orthogonal by construction).
// false: the point is not in front of the previous camera (or a NaN took part)
BM_DHD bool reproject_project(const CameraBasis& cur, const RpPrevCamera& prev, float W, float H, int x, int y, float distance, float& u, float& v) {
	float dhat[3], e[3];
	pixel_ray_direction(cur.dir, cur.right, cur.up, W, H, static_cast<float>(x) + 0.5f, static_cast<float>(y) + 0.5f, dhat);
	for (int k = 0; k < 3; ++k) {
		const float P = cur.origin[k] + dhat[k] * distance;
		e[k] = P - prev.b.origin[k];
	}
	const float t = ((e[0] * prev.b.dir[0] + e[1] * prev.b.dir[1]) + e[2] * prev.b.dir[2]) / prev.dd;
	if (!(t > 0.f)) return false;
	const float a = ((e[0] * prev.b.right[0] + e[1] * prev.b.right[1]) + e[2] * prev.b.right[2]) / (t * prev.rr);
	const float b = ((e[0] * prev.b.up[0] + e[1] * prev.b.up[1]) + e[2] * prev.b.up[2]) / (t * prev.uu);
	u = (a + 0.5f) * W + 0.5f;
	v = (H - (b + 0.5f) * H) + 0.5f;
	return true;
}

// the four taps around (u, v) in the order (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) and their bilinear weights.
// false: every tap lies outside the image (tested in float before the conversion to int, which also catches NaN and infinity)
struct RpTaps {
	int x0, y0;
	float w[4];
};
BM_DHD bool reproject_taps(float u, float v, float W, float H, RpTaps& t) {
	const float x0f = floorf(u), fx = u - x0f;
	const float y0f = floorf(v), fy = v - y0f;
	if (!(x0f >= -1.f && x0f <= W - 1.f && y0f >= -1.f && y0f <= H - 1.f)) return false;
	t.x0 = static_cast<int>(x0f);
	t.y0 = static_cast<int>(y0f);
	const float gx = 1.f - fx, gy = 1.f - fy;
	t.w[0] = gx * gy;
	t.w[1] = fx * gy;
	t.w[2] = gx * fy;
	t.w[3] = fx * fy;
	return true;
}

// the sums over the taps that count, in tap order from 0.0f
struct RpSum { float w, r, g, b, n; };
BM_DHD RpSum reproject_zero() { RpSum s = {0.f, 0.f, 0.f, 0.f, 0.f}; return s; }
// inside: the tap lies in the image (key_q and the tap's value (R, G, B, n_q) mean nothing otherwise)
BM_DHD void reproject_tap(RpSum& s, bool inside, uint32_t key_q, uint32_t key_p, float w, float R, float G, float B, float n_q) {
	if (!inside || key_q != key_p || !(n_q > 0.f) || !(w > 0.f)) return;
	s.w += w;
	s.r += w * (R / n_q);
	s.g += w * (G / n_q);
	s.b += w * (B / n_q);
	s.n += w * n_q;
}
// out = history + the frame's own samples; false (out untouched): no tap counted
BM_DHD bool reproject_blend(const RpSum& s, float max_history, const float accum[4], float out[4]) {
	if (!(s.w > 0.f)) return false;
	float n_h = s.n / s.w;
	n_h = n_h < max_history ? n_h : max_history;
	out[0] = (s.r / s.w) * n_h + accum[0];
	out[1] = (s.g / s.w) * n_h + accum[1];
	out[2] = (s.b / s.w) * n_h + accum[2];
	out[3] = n_h + accum[3];
	return true;
}

// ---- what both routes refuse (BM_EINVAL): returns the reason, or null for parameters that are fine
struct ReprojectParamsView { int width, height; float max_history; uint32_t flags, reserved; };
inline const char* reproject_params_problem(const ReprojectParamsView& p) {
	if (p.width < 1 || p.height < 1 || p.width > 65535 || p.height > 65535) return "width and height must be 1 ... 65535";
	if (!(p.max_history >= 1.f) || !(p.max_history <= 3.402823466e38f)) return "max_history must be finite and at least 1";
	if (p.flags != 0 || p.reserved != 0) return "flags and reserved must be 0";
	return nullptr;
}
// a history: the float4 image, then the keys
inline size_t history_bytes(int width, int height) { return static_cast<size_t>(width) * static_cast<size_t>(height) * 20; }

} // namespace bm
