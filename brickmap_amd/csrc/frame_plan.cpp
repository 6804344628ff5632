// frame_plan.cpp -- the pure-host plans (frame_plan.h).  Of a frame: FrameConstants from a camera and frame parameters (view basis, sky
// constants, the hand-out's geometry, refill and helper-lane rules), the tuning overrides of the environment and the multiply-high division
// constants.  Of a launch (plan_launch): which frames may go out together, in which ring mode, with what grid.  Calls no HIP function.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstddef>
#include <cstring>

#include "camera_rays.h"
#include "error.h"
#include "frame_plan.h"

namespace bm {

// ---------------------------------------------------------------- small host vector helpers (GLM operation order)
namespace {
struct V3 {
	float x, y, z;
};
inline V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline V3 cross3(V3 x, V3 y) { return {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y}; }
inline V3 normalize3(V3 v) { return v * (1.0f / std::sqrt(dot3(v, v))); }
constexpr float kPi = 3.1415926535897932f;

// sunsky.cu:24-26 -- double literals make the tail of this expression double
float sun_intensity(float zenith_cos) {
	const float cutoff = kPi / 1.95f, steepness = 1.5f;
	const double e = 1.0 - static_cast<double>(std::exp(-((cutoff - std::acos(zenith_cos)) / steepness)));
	return static_cast<float>(1000.0 * (0.0 < e ? e : 0.0));
}
} // namespace

// floor(n / d) for every n < 2^30 as umulhi(n, magic) >> shift (Granlund-Montgomery: with l = ceil(log2 d) and
// magic = ceil(2^(30 + l) / d) one has 2^(30+l) <= magic * d < 2^(30+l) + 2^l, which makes the truncated product exact for 30-bit n;
// magic < 2^31 + 1 fits 32 bits; tests/test_host_logic.py replays it against integer division)
void division_magic(uint32_t d, uint32_t* magic, int* shift) {
	int l = 0;
	while ((1ull << l) < d) ++l;
	if (l < 2) l = 2;
	const unsigned __int128 one = static_cast<unsigned __int128>(1) << (30 + l);
	*magic = static_cast<uint32_t>((one + d - 1) / d);
	*shift = l - 2; // (30 + l) - 32
}

// Tuning overrides, read from the environment ONCE per process (A/B runs, tools/): BM_REFILL_MIN (1 ... 64), BM_XCD_HANDOUT (0 / 1),
// BM_HELPERS (0 / 1), BM_TRACE_BLOCKS_PER_CU (> 0), BM_RING_GROUP (1 ... 64).  None set = the product's own rules.  bm_tuning_overrides() reports them, so that
// a measurement can say what it ran under (bench.py echoes them into its line and refuses to go on under BM_BENCH_STRICT=1).
const Tuning& tuning() {
	static const Tuning t = [] {
		Tuning v;
		auto num = [](const char* name, int unset) { const char* e = std::getenv(name); return e && *e ? std::atoi(e) : unset; };
		v.refill_min = num("BM_REFILL_MIN", 0);
		v.xcd_handout = num("BM_XCD_HANDOUT", -1);
		v.helpers = num("BM_HELPERS", -1);
		v.blocks_per_cu = num("BM_TRACE_BLOCKS_PER_CU", 0);
		v.ring_group = num("BM_RING_GROUP", 0);
		return v;
	}();
	return t;
}

// The hand-out counts tickets in 32 bits (trace.hip: `my_tickets`, `base + want`).  The busiest counter owns a 1/8 share of the
// units -- groups of four chunks, or 256x256-pixel super-tiles of 4096 chunks -- times `per_chunk` tickets per chunk: 16, times the
// samples with (chunk, sample) items, times the frames of a group in a uniform launch; every wave may overshoot a used-up counter
// once by up to 64.
static bool tickets_fit(int tiles_x, int tiles_y, bool xcd, long long per_chunk) {
	long long share;
	if (xcd) {
		const long long st = static_cast<long long>((tiles_x + 15) / 16) * ((tiles_y + 15) / 16);
		share = ((st + 7) / 8) * 4096ll * per_chunk;
	} else {
		share = ((static_cast<long long>(tiles_x) * tiles_y * 4 + 7) / 8) * 4ll * per_chunk;
	}
	return share < (1ll << 30) - (1ll << 24); // (2^30: the hand-out divides ticket numbers with 30-bit-exact multiply-high constants)
}

// How many consecutive frames of a UNIFORM launch (plan_launch, below) are handed out together, as (chunk, pixel part, frame)
// items (trace.hip "FRAME GROUPS")?  The one place that decides it.  Frames that add every event with float atomics -- helper lanes
// on -- leave the order of a pixel's additions free already, so their frames may run side by side in a wave: kRingGroup, or
// BM_RING_GROUP (1 = frame after frame, for A/B runs), at most the frames there are.  Ordered frames write back with plain stores and
// compare bit for bit with single launches: 1.  Frames with (chunk, sample) items of two or more samples hold a pixel's samples in
// neighbouring lanes as it is, and the ticket has one field for "which sample of the chunk": 1.  And 1 where the tickets of a group
// would not fit their counter.
int ring_group_of(const FrameConstants& fc, int frames) {
	const bool several_sample_items = (fc.flags & BM_FLAG_SAMPLE_ITEMS) && fc.spp >= 2;
	if (!fc.helpers || several_sample_items || frames < 2) return 1;
	const int chosen = tuning().ring_group;
	int group = chosen >= 1 && chosen <= kMaxRingGroup ? chosen : kRingGroup;
	group = std::min(group, frames);
	if (!tickets_fit(fc.tiles_x, fc.tiles_y, fc.xcd_handout != 0, 16ll * group)) group = 1;
	return group;
}

int fill_frame_constants(const bm_camera* cam, const bm_frame_params* fp_in, FrameConstants* fc, bool hit_records) {
	if (!fp_in) { set_error("null argument"); return BM_EINVAL; }
	if (fp_in->flags & ~(BM_FLAG_PRIMARY_ONLY | BM_FLAG_COUNTERS | BM_FLAG_SAMPLE_ITEMS | BM_FLAG_ORDERED | BM_FLAG_RAY_DIGEST)) {
		set_error("unknown frame flag (bit 8 was the retired K-slot schedule's)");
		return BM_EINVAL;
	}
	// Which frames are ORDERED (every pixel's events accumulated in path order by one lane, one plain write-back: reproducible sums)?
	// Those that ask for it, those that write hit records, primary-only frames.  Every other frame -- the production
	// default -- may add in any order, like the reference's own atomicAdds (kernel.cu:319-322,341-343): it runs with helper lanes
	// (trace.hip HELP) and, when a pixel has several samples, with (4x4 chunk, sample) work items: shorter items, a shorter tail,
	// coherent neighbouring samples (1080p at 4 spp 4.0 -> 3.4 ms, config 3 -4 %).  BM_HELPERS=0 / 1 overrides helper lanes (A/B runs).
	bm_frame_params promoted = *fp_in;
	// (hit records are chains in path order -- an ordered frame -- unless the caller asked for the order-independent ray digest)
	const bool ordered = (promoted.flags & (BM_FLAG_ORDERED | BM_FLAG_PRIMARY_ONLY)) != 0 || (hit_records && !(promoted.flags & BM_FLAG_RAY_DIGEST)) || promoted.spp < 1; // (spp = 0: nothing to trace)
	const bm_frame_params* const fp = &promoted;
	if (!cam || !fp || !fc) { set_error("null argument"); return BM_EINVAL; }
	if (fp->width <= 0 || fp->height <= 0 || fp->spp < 0 || fp->max_bounces < 0 || fp->band_rows <= 0 || fp->shard_count <= 0 ||
		fp->shard_rank < 0 || fp->shard_rank >= fp->shard_count) {
		set_error("bad frame parameters");
		return BM_EINVAL;
	}
	// the kernels pack a pixel as x | y << 16 and index the shard's packed buffers with 32-bit pixel numbers
	if (fp->width > 65535 || fp->height > 65535 || static_cast<long long>(bm_local_rows(fp)) * fp->width >= (1ll << 32)) {
		set_error("frame too large: width and height are limited to 65535 and a shard to 2^32 pixels");
		return BM_EINVAL;
	}
	if ((fp->flags & BM_FLAG_RAY_DIGEST) && (fp->max_bounces >= 255 || static_cast<long long>(fp->spp) * (fp->max_bounces + 1) >= 65536)) {
		set_error("BM_FLAG_RAY_DIGEST: the digest counts a pixel's rays in 16 bits and keys them with 8 bits of segment: spp x segments < 65536, max_bounces < 255");
		return BM_EINVAL;
	}
	const int geo_tiles_x = (fp->width + 15) / 16, geo_tiles_y = (bm_local_rows(fp) + 15) / 16;
	// XCD-aware hand-out: neighbouring rays behind ONE L2 instead of all eight.  Pays where the scene does not fit the caches and the
	// frame has enough 256x256-pixel super-tiles for eight even shares (8K: 510, 4K: 135) -- config 5 115.0 -> 111.5 ms, config 3
	// 24.05 -> 23.90; on a 1080p frame (40 super-tiles) the shares are too uneven: +8 % (profiles/r04_xcd_handout.txt)
	int geo_xcd = (static_cast<long long>(geo_tiles_x) * geo_tiles_y >= 32000) ? 1 : 0;
	if (tuning().xcd_handout == 0 || tuning().xcd_handout == 1) geo_xcd = tuning().xcd_handout;
	// the ticket counters are 32 bits wide (tickets_fit, above): 16 tickets per chunk and, with (chunk, sample) items, per sample
	auto tickets_fit = [&](bool sample_items) { return bm::tickets_fit(geo_tiles_x, geo_tiles_y, geo_xcd != 0, 16ll * (sample_items ? std::max(fp->spp, 1) : 1)); };
	if (!tickets_fit((promoted.flags & BM_FLAG_SAMPLE_ITEMS) != 0)) { // what the caller asked for does not fit: refuse
		set_error("frame too large for the 32-bit ticket counters: tiles x samples per launch (lower spp per call, or render row-band shards)");
		return BM_EINVAL;
	}
	// (chunk, sample) items as the library's own choice -- only where their tickets fit; pixel items carry no spp factor and always
	// do at this point (helper lanes work with either: atomic_acc = HELP)
	if (!ordered && promoted.spp >= 2 && tickets_fit(true)) promoted.flags |= BM_FLAG_SAMPLE_ITEMS;
	std::memset(fc, 0, sizeof *fc);
	const CameraBasis basis = camera_basis(cam->position, cam->direction, cam->up, fp->width, fp->height); // launch_kernels:384-385
	for (int i = 0; i < 3; ++i) {
		fc->right[i] = basis.right[i];
		fc->up[i] = basis.up[i];
		fc->dir[i] = basis.dir[i];
		fc->origin[i] = basis.origin[i];
		fc->campos[i] = static_cast<int>(cam->position[i] / 8.f); // kernel.cu:418
	}
	fc->focal3 = cam->focal_distance * 3; // kernel.cu:191-192 (int 3)
	fc->lens_radius = cam->lens_radius;

	// sky constants (kernel.cu:374,393; sunsky.cu:14-18,28-30,34-44,66-67)
	fc->sun_angular_cos = std::cos(1.5f * kPi / 180.f);
	fc->cone_extent = 1.0f - fc->sun_angular_cos;
	const float px = (fp->sun_position[0] - 0.0f) * 6.28f, py = (fp->sun_position[1] - 0.5f) * 3.14f;
	const V3 sun = normalize3(V3{std::cos(px) * std::sin(py), std::sin(px) * std::sin(py), std::cos(py)});
	fc->sun_direction[0] = sun.x; fc->sun_direction[1] = sun.y; fc->sun_direction[2] = sun.z;
	{ // getConeSample's frame around the sun direction (sunsky.cu:163-174), same fp32 operations as the reference
		const V3 cd = normalize3(sun);
		const V3 ortho = std::fabs(cd.x) > std::fabs(cd.z) ? V3{-cd.y, cd.x, 0.0f} : V3{0.0f, -cd.z, cd.y};
		const V3 o1 = normalize3(ortho);
		const V3 o2 = normalize3(cross3(cd, o1));
		fc->cone_dir[0] = cd.x; fc->cone_dir[1] = cd.y; fc->cone_dir[2] = cd.z;
		fc->cone_o1[0] = o1.x; fc->cone_o1[1] = o1.y; fc->cone_o1[2] = o1.z;
		fc->cone_o2[0] = o2.x; fc->cone_o2[1] = o2.y; fc->cone_o2[2] = o2.z;
	}
	const V3 sky_up{0.0f, 0.0f, 1.0f};
	fc->sunE = sun_intensity(dot3(sun, sky_up));
	const float rayleigh[3] = {5.176821E-6f, 1.2785348E-5f, 2.8530756E-5f};
	const float lambda[3] = {680E-9f, 550E-9f, 450E-9f};
	const float K[3] = {0.686f, 0.678f, 0.666f};
	const float c = static_cast<float>((0.2 * static_cast<double>(1.f)) * 10E-18); // turbidity 1
	const float mie_scale = 0.434f * c * kPi;
	const float expo = static_cast<float>(static_cast<double>(4.0f) - 2.0);
	for (int i = 0; i < 3; ++i) {
		const float total_mie = (std::pow((2.0f * kPi) / lambda[i], expo) * mie_scale) * K[i];
		fc->rayleigh[i] = rayleigh[i];
		fc->mie[i] = total_mie * 0.005f;
		fc->inv_total[i] = 1.0f / (fc->rayleigh[i] + fc->mie[i]);
	}
	const float m = std::pow(1.0f - dot3(sky_up, sun), 5.0f);
	fc->mixf = std::min(std::max(m, 0.0f), 1.0f);

	fc->width = fp->width; fc->height = fp->height;
	fc->spp = fp->spp; fc->sample_base = fp->sample_base; fc->max_bounces = fp->max_bounces;
	fc->base_frame = fp->base_frame; fc->flags = fp->flags;
	fc->band_rows = fp->band_rows; fc->shard_rank = fp->shard_rank; fc->shard_count = fp->shard_count;
	fc->local_rows = bm_local_rows(fp);
	fc->tiles_x = geo_tiles_x;
	fc->tiles_y = geo_tiles_y;
	// When does a wave stop to refill?  Every refill costs the whole wave an atomic's round trip and ~110 instructions, every idle
	// lane costs its share of all passes until then.  An item is all samples of a pixel (or ONE with BM_FLAG_SAMPLE_ITEMS): the
	// longer it is, the rarer the refills, the earlier they pay (measured per workload, profiles/r04_refill_sweep.txt).
	const int refill_override = tuning().refill_min;
	const int samples_per_item = (fp->flags & BM_FLAG_SAMPLE_ITEMS) ? 1 : fp->spp;
	fc->refill_min = samples_per_item >= 4 ? 4 : (samples_per_item >= 2 ? 8 : 16);
	fc->xcd_handout = geo_xcd;
	if (refill_override >= 1 && refill_override <= 64) fc->refill_min = refill_override;
	// shadow rays on helper lanes (trace.hip HELP): every frame that is not ordered (above)
	fc->helpers = ordered ? 0 : 1;
	const int help_override = tuning().helpers;
	if (help_override == 0 || (help_override == 1 && !ordered)) fc->helpers = help_override;
	// with helper lanes an idle lane is not wasted while it waits for the refill -- it takes shadow rays -- so the wave refills later:
	// 24 idle lanes instead of 16 (config 2 -0.2 %, 1080p at 4 spp -1.1 %, config 3 -0.8 %; 32: worse again; profiles/r05_refill_sweep.txt)
	if (fc->helpers && refill_override <= 0) fc->refill_min = 24;
	{ // divisions of the hand-out by per-frame constants (trace.hip refill): multiply-high + shift
		auto set = [](uint32_t d, uint32_t* magic, int* shift) { if (d <= 1u) { *magic = 0u; *shift = 0; } else division_magic(d, magic, shift); };
		set((fp->flags & BM_FLAG_SAMPLE_ITEMS) ? static_cast<uint32_t>(std::max(fp->spp, 1)) : 1u, &fc->div_samples_magic, &fc->div_samples_shift);
		set(static_cast<uint32_t>(fc->tiles_x), &fc->div_tiles_x_magic, &fc->div_tiles_x_shift);
		set(static_cast<uint32_t>(fc->band_rows), &fc->div_band_magic, &fc->div_band_shift);
		set(static_cast<uint32_t>((fc->tiles_x + 15) / 16), &fc->div_st_x_magic, &fc->div_st_x_shift);
	}
	fc->ring_group = 1; // (a launch of one frame; plan_launch sets the groups of a uniform launch)
	return 0;
}

// the hand-out's division by the samples of a (chunk, sample) ticket group, times the frames of a group of a uniform launch
void set_ring_group(FrameConstants* fc, int group, int frames) {
	fc->ring_group = group;
	fc->ring_groups_after = (frames + group - 1) / group - 1;
	const uint32_t d = ((fc->flags & BM_FLAG_SAMPLE_ITEMS) ? static_cast<uint32_t>(std::max(fc->spp, 1)) : 1u) * static_cast<uint32_t>(group);
	if (d <= 1u) { fc->div_samples_magic = 0u; fc->div_samples_shift = 0; } else division_magic(d, &fc->div_samples_magic, &fc->div_samples_shift);
}

// ---------------------------------------------------------------- the plan of a launch
// `count` consecutive frames -- the reference's per-frame loop (main.cpp:117-147: one launch_kernels call per frame) -- as ONE launch
// of the persistent kernel (trace.hip "FRAME RING"): every decision about it that needs no device.  Scene::render_frames issues it.
int plan_launch(int count, const bm_camera* cams, const bm_frame_params* fps, float* const* accums, uint32_t* const* dbgs, int cells, int cells_height, LaunchPlan* out) {
	if (count < 1 || count > kMaxFramesPerLaunch) { set_error("bm_render_frames: 1 ... 256 frames per launch"); return BM_EINVAL; }
	if (!cams || !fps || !accums) { set_error("null argument"); return BM_EINVAL; }
	bool hit_records = false;
	for (int i = 0; i < count; ++i) {
		if (!accums[i]) { set_error("null accumulation buffer"); return BM_EINVAL; }
		hit_records = hit_records || (dbgs && dbgs[i]);
	}
	// ---- constants of every frame; what shapes the hand-out must be the same for all frames of a launch
	std::vector<FrameConstants>& fcs = out->frames;
	fcs.assign(static_cast<size_t>(count), FrameConstants{});
	for (int i = 0; i < count; ++i) {
		if (int e = fill_frame_constants(cams + i, fps + i, &fcs[static_cast<size_t>(i)], hit_records)) return e;
		FrameConstants& f = fcs[static_cast<size_t>(i)];
		f.accum = accums[i];
		f.dbg = dbgs ? dbgs[i] : nullptr;
		f.frames_after = count - 1 - i;
		const FrameConstants& g = fcs[0];
		if (f.width != g.width || f.height != g.height || f.spp != g.spp || f.max_bounces != g.max_bounces || f.flags != g.flags || f.band_rows != g.band_rows ||
			f.shard_rank != g.shard_rank || f.shard_count != g.shard_count) {
			set_error("bm_render_frames: the frames of one launch must agree in width, height, spp, max_bounces, flags and shard (camera, sun, sample_base, base_frame and buffers may differ)");
			return BM_EINVAL;
		}
	}
	// In a launch of several frames a wave refills later: what argues for an early refill in a lone frame -- the paths started last are what
	// the frame's end waits for -- does not count when the next frame covers that end (ring of 20, kernel ms per frame: 24 idle lanes 0.7514,
	// 32: 0.7478, 36: 0.7481, 40: 0.7515; 1080p at 4 spp 2.937 / 2.905 / 2.894 / 2.899; profiles/r06_frame_ring.txt)
	if (count > 1)
		for (FrameConstants& f : fcs) f.refill_min = ring_refill_min(f.refill_min, f.helpers != 0, tuning().refill_min);
	const FrameConstants& fc = fcs[0];
	bool shared_digest = false; // ray-digest frames that all write ONE hit-record buffer (and one accumulation buffer)
	if (count > 1) {
		// Frames of a launch overlap in time.  Hit records are written with plain stores, and so are the pixels of frames that neither
		// run helper lanes nor (chunk, sample) items (read when a lane takes the pixel, written back when it is done): such frames
		// need buffers of their own.  Frames that add with float atomics may share one buffer, like consecutive frames of the
		// reference's accumulation (kernel.cu:319-322,341-343).
		const size_t pixels = static_cast<size_t>(fc.local_rows) * static_cast<size_t>(fc.width);
		const bool plain_pixels = !(fc.helpers || (fc.flags & BM_FLAG_SAMPLE_ITEMS));
		for (int i = 0; i < count; ++i)
			for (int k = 0; k < i; ++k) {
				const char *a = reinterpret_cast<const char*>(accums[i]), *b = reinterpret_cast<const char*>(accums[k]);
				if (plain_pixels && a < b + pixels * 16 && b < a + pixels * 16) {
					set_error("bm_render_frames: ordered frames of one launch need accumulation buffers of their own (they overlap in time and write pixels back with plain stores)");
					return BM_EINVAL;
				}
				const char *c = dbgs ? reinterpret_cast<const char*>(dbgs[i]) : nullptr, *d = dbgs ? reinterpret_cast<const char*>(dbgs[k]) : nullptr;
				if (c && d && c == d && a == b && (fc.flags & BM_FLAG_RAY_DIGEST)) { shared_digest = true; continue; } // (allowed for uniform launches: below)
				if (c && d && c < d + pixels * 32 && d < c + pixels * 32) {
					set_error("bm_render_frames: the frames of one launch need hit-record buffers of their own");
					return BM_EINVAL;
				}
			}
	}
	// ---- a UNIFORM launch?  Frames that differ only in sample_base and buffers, both stepping by constants (a resting camera: the
	// reference's progressive accumulation; bench.py's steps; a rank's batch into one allocation): lanes of consecutive frames may then
	// share a wave (trace.hip), because nothing a lane reads after it took its item depends on the frame any more.
	bool uniform = false, digest_ok = false;
	if (shared_digest) { // every frame names the same two buffers?
		digest_ok = true;
		for (int i = 0; i < count; ++i) digest_ok = digest_ok && dbgs[i] == dbgs[0] && accums[i] == accums[0];
	}
	if (count > 1 && (!hit_records || digest_ok)) {
		auto same_view = [&](const FrameConstants& a, const FrameConstants& b) {
			// everything up to `width` is the view, the sun and the sky (device_types.h); base_frame seeds the RNG
			return std::memcmp(&a, &b, offsetof(FrameConstants, width)) == 0 && a.base_frame == b.base_frame;
		};
		const long long sample_stride = static_cast<long long>(fcs[1].sample_base) - fcs[0].sample_base;
		const long long byte_stride = reinterpret_cast<const char*>(accums[1]) - reinterpret_cast<const char*>(accums[0]);
		const unsigned long long pixels = static_cast<unsigned long long>(fc.local_rows) * static_cast<unsigned long long>(fc.width);
		uniform = sample_stride >= 0 && sample_stride < (1 << 20) && byte_stride >= 0 && byte_stride % 16 == 0 &&
				  static_cast<unsigned long long>(byte_stride / 16) * static_cast<unsigned long long>(count - 1) + pixels < (1ull << 32) &&
				  static_cast<long long>(fcs[0].sample_base) + sample_stride * (count - 1) + fc.spp < (1ll << 31);
		for (int i = 1; i < count && uniform; ++i)
			uniform = same_view(fcs[static_cast<size_t>(i)], fcs[0]) && static_cast<long long>(fcs[static_cast<size_t>(i)].sample_base) == fcs[0].sample_base + sample_stride * i &&
					  reinterpret_cast<const char*>(accums[i]) == reinterpret_cast<const char*>(accums[0]) + byte_stride * i;
		if (uniform) {
			for (int i = 0; i < count; ++i) { // every entry reads like the first; the frame is an offset the lanes add themselves
				fcs[static_cast<size_t>(i)].sample_base = fcs[0].sample_base;
				fcs[static_cast<size_t>(i)].accum = fcs[0].accum;
			}
			fcs[0].ring_uniform = 1;
			fcs[0].ring_sample_stride = static_cast<int>(sample_stride);
			fcs[0].ring_pixel_stride = static_cast<uint32_t>(byte_stride / 16);
			// ... and frames that add with float atomics are handed out several at a time (trace.hip "FRAME GROUPS")
			set_ring_group(&fcs[0], ring_group_of(fcs[0], count), count);
		}
		if (shared_digest && !uniform) digest_ok = false;
	}
	if (shared_digest && !digest_ok) {
		// One hit-record buffer for several frames is the digest of the WHOLE launch: its keys count samples from the first frame's
		// sample_base and its first-hit record is written once -- which only a uniform launch (one view, stepping sample_base) defines
		set_error("bm_render_frames: ray-digest frames may share one hit-record buffer only in a uniform launch (one view and sun, sample_base stepping by a constant, one accumulation buffer)");
		return BM_EINVAL;
	}
	if (shared_digest) {
		// ... and that digest counts the pixel's rays of ALL the frames in 16 bits (word 6) and keys them with 24 bits of sample index
		// counted from the first frame's sample_base: fill_frame_constants checked one frame's share of either
		const long long sample_stride = fc.ring_sample_stride; // (a shared digest is a uniform launch; the entries' own sample_base all read like the first by now)
		if (static_cast<long long>(count) * fc.spp * (fc.max_bounces + 1) >= 65536 || sample_stride * (count - 1) + fc.spp >= (1ll << 24)) {
			set_error("bm_render_frames: ray-digest frames that share one hit-record buffer: frames x spp x segments < 65536 and sample_base stride x (frames - 1) + spp < 2^24 (the digest counts the launch's rays per pixel in 16 bits and keys them with 24 bits of sample)");
			return BM_EINVAL;
		}
	}
	{ // the kernel's hang guard is a 64-bit product (trace.hip round_budget): a launch for which it would wrap -- it would end before it has
	  // traced anything -- is refused (such a launch is weeks of GPU time anyway)
		const unsigned __int128 rounds = static_cast<unsigned __int128>(static_cast<unsigned long long>(fc.tiles_x) * static_cast<unsigned long long>(fc.tiles_y) * 16ull + 64ull) *
										 static_cast<unsigned long long>(fc.spp + 1) * static_cast<unsigned long long>(fc.max_bounces + 2) *
										 static_cast<unsigned long long>(2ll * cells + cells_height + 64) * static_cast<unsigned long long>(count);
		if (rounds >= (static_cast<unsigned __int128>(1) << 62)) {
			set_error("launch too large: tiles x samples x segments x frames overflows the kernel's round budget (render fewer samples or frames per launch)");
			return BM_EINVAL;
		}
	}
	out->ring_mode = count > 1 ? (uniform ? 2 : 1) : 0;
	out->instrumented = instrumented_frame(fc.flags, hit_records);
	out->shared_digest = shared_digest;
	// (one block of ticket counters per frame; a uniform launch uses one per GROUP of frames, the first of them)
	out->counter_blocks = uniform ? fc.ring_groups_after + 1 : count;
	// never more waves than a frame has 64-item groups: an item is a pixel, or ONE sample of a pixel with (chunk, sample) items -- a
	// 1/8 shard of a 1080p frame at 8 spp is 276 480 pixels but 2.2 M items, and sizing its launch by pixels left 40 % of the
	// GPU's wave slots empty (1080 of 1792 workgroups: 1.16 -> 0.95 ms per shard step).  A launch of several frames may start a
	// second frame's worth of waves: those that find the first frame's counters used up go straight on to the next one.
	const long long items = static_cast<long long>(fc.tiles_x) * fc.tiles_y * 256 * ((fc.flags & BM_FLAG_SAMPLE_ITEMS) ? std::max(fc.spp, 1) : 1);
	out->workgroups = (items + 255) / 256 * (count > 1 ? 2 : 1);
	return 0;
}

} // namespace bm
