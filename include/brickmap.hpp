// brickmap.hpp -- header-only C++ mirror of the reference's host interface for the path-trace hot path,
// on top of the C-ABI in brickmap.h.  Same names, argument meaning and error behaviour as the reference
// (file:line into the reference's src/):
//   Camera          camera.h:3-24, camera.cpp:48-54          (input handling needs a window: out of scope)
//   State           state.h:5-34                             (ray queues / GL interop are gone: paths live in registers)
//   Scene           Scene.h:7-44, Scene.cpp:29-258
//   launch_kernels  launch.h:6, kernel.cu:366-439            (fused per-pixel paths; or, with a Wavefront, the reference's queue schedule)
//   launch_frames   main.cpp:117-147                         (that many iterations of the frame loop as ONE launch: the frame ring)
//   hip(...)        assert_cuda.h:5, assert_cuda.cpp:3-13     (print, then exit(code): the reference's cuda() macro)
// A maintainer swaps `#include "launch.h"` + the CUDA sources for this header and links libbrickmap_hip.so;
// see INTEGRATION.md for the exact diff against src/main.cpp.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <array>
#include <vector>

#include "brickmap.h"

namespace brickmap {

// assert_cuda.cpp:3-13: report and abort on any device error (the C-ABI itself only returns codes)
inline int bm_assert(int code, const char* file, int line, bool abort = true) {
	if (code != 0) {
		std::fprintf(stderr, "hip_assert: %s %s %d\n", bm_last_error_string(), file, line);
		if (abort) std::exit(code);
	}
	return code;
}
#define BM_CHECKED(call) ::brickmap::bm_assert((call), __FILE__, __LINE__, true)

struct vec2 { float x, y; };
struct vec3 { float x, y, z; };
struct vec4 { float x, y, z, w; };

// variables.h:37-38, variables.cpp:3-4
inline vec2 sun_position = {0.05f, 0.1f};
inline bool sun_position_changed = true;

struct Camera { // camera.h:3-24
	vec3 position = {512, 512, 300};
	vec3 direction = {1, 0, 0};
	vec3 up = {0, 0, 1};
	float focalDistance = 1;
	float lensRadius = 0.0f;
	double horizontal_angle = 0.0;
	double vertical_angle = 0.0;

	void update() { // camera.cpp:48-54
		vec3 d = {static_cast<float>(std::cos(vertical_angle) * std::sin(horizontal_angle)),
				  static_cast<float>(std::cos(vertical_angle) * std::cos(horizontal_angle)), static_cast<float>(std::sin(vertical_angle))};
		const float inv = 1.0f / std::sqrt((d.x * d.x + d.y * d.y) + d.z * d.z); // glm::normalize
		direction = {d.x * inv, d.y * inv, d.z * inv};
	}
	bm_camera to_c() const {
		bm_camera cam{};
		cam.position[0] = position.x; cam.position[1] = position.y; cam.position[2] = position.z;
		cam.direction[0] = direction.x; cam.direction[1] = direction.y; cam.direction[2] = direction.z;
		cam.up[0] = up.x; cam.up[1] = up.y; cam.up[2] = up.z;
		cam.focal_distance = focalDistance;
		cam.lens_radius = lensRadius;
		return cam;
	}
	// rays through continuous pixel positions (px[i], py[i]) of a width x height frame -- the frames' primary rays without jitter and
	// lens; (x + 0.5, y + 0.5) is pixel (x, y)'s centre (bm_camera_pixel_rays, no counterpart in the reference)
	void pixel_rays(int width, int height, int64_t n, const float* px, const float* py, bm_ray* out) const {
		const bm_camera cam = to_c();
		BM_CHECKED(bm_camera_pixel_rays(&cam, width, height, n, px, py, out));
	}
};
inline Camera camera; // camera.h:24 `extern Camera camera;`

class Scene { // Scene.h:7-44
public:
	struct GPUScene { // passed by value to launch_kernels, like Scene::GPUScene (Scene.h:9-17)
		bm_scene* handle = nullptr;
	};
	GPUScene gpuScene;

	// world dimensions are constexpr in the reference (variables.h:7-8: 4096 x 4096 x 512 voxels)
	explicit Scene(int grid_size = 4096, int grid_height = 512, int device = 0) : device_(device) {
		BM_CHECKED(bm_scene_create(device, grid_size, grid_height, &gpuScene.handle));
	}
	~Scene() { bm_scene_destroy(gpuScene.handle); }
	Scene(const Scene&) = delete;
	Scene& operator=(const Scene&) = delete;

	void generate_supercell(int start_x, int start_y, int start_z) { BM_CHECKED(bm_scene_generate_supercell(gpuScene.handle, start_x, start_y, start_z)); }
	void generate() { BM_CHECKED(bm_scene_generate(gpuScene.handle, static_cast<int>(std::thread::hardware_concurrency()))); }
	void process_load_queue() { BM_CHECKED(bm_scene_process_load_queue(gpuScene.handle, nullptr)); }
	void dump() { BM_CHECKED(bm_scene_dump(gpuScene.handle, "dump.txt")); }
	// BASELINE configs 1-2: everything resident up front (no counterpart in the reference)
	void preload_all() { BM_CHECKED(bm_scene_preload_all(gpuScene.handle)); }

	// the caller's own voxels as the world (no counterpart in the reference; bm_scene_load_voxels): a dense volume [z][y][x] of one byte
	// per voxel, non-zero = solid, in host memory (BM_VOXELS_HOST) or in memory of the scene's device (BM_VOXELS_DEVICE: packed on the
	// GPU, behind the work queued on hip_stream).  Instead of generate(), or to replace the world; the scene is preloaded afterwards.
	void load_voxels(const uint8_t* voxels, size_t bytes, int where = BM_VOXELS_HOST, void* hip_stream = nullptr) {
		BM_CHECKED(bm_scene_load_voxels(gpuScene.handle, voxels, bytes, where, hip_stream));
	}
	// the host world as a dense volume of 0 / 1 in the same layout
	std::vector<uint8_t> voxels() const {
		size_t bytes = 0;
		BM_CHECKED(bm_scene_host_voxels(gpuScene.handle, nullptr, 0, &bytes));
		std::vector<uint8_t> out(bytes);
		BM_CHECKED(bm_scene_host_voxels(gpuScene.handle, out.data(), out.size(), &bytes));
		return out;
	}

	// voxel edits of the live world (no counterpart in the reference; bm_scene_edit): applied in order, behind the frames in flight,
	// seen by every frame issued afterwards.  Integer voxel coordinates; boxes are half-open [lo, hi), spheres hold |v - c|^2 <= r^2.
	void edit(const std::vector<bm_edit>& edits, void* hip_stream = nullptr) {
		BM_CHECKED(bm_scene_edit(gpuScene.handle, static_cast<int>(edits.size()), edits.data(), hip_stream));
	}
	static bm_edit box(int op, const int lo[3], const int hi[3]) {
		bm_edit e{};
		e.op = op; e.shape = BM_EDIT_BOX;
		for (int k = 0; k < 3; ++k) { e.lo[k] = lo[k]; e.hi[k] = hi[k]; }
		return e;
	}
	static bm_edit sphere(int op, const int center[3], int radius) {
		bm_edit e{};
		e.op = op; e.shape = BM_EDIT_SPHERE; e.radius = radius;
		for (int k = 0; k < 3; ++k) e.center[k] = center[k];
		return e;
	}
	void fill_box(const int lo[3], const int hi[3]) { edit({box(BM_EDIT_SET, lo, hi)}); }
	void clear_box(const int lo[3], const int hi[3]) { edit({box(BM_EDIT_CLEAR, lo, hi)}); }
	void fill_sphere(const int center[3], int radius) { edit({sphere(BM_EDIT_SET, center, radius)}); }
	void carve_sphere(const int center[3], int radius) { edit({sphere(BM_EDIT_CLEAR, center, radius)}); }

	// dense regions of the live world (no counterpart in the reference; bm_scene_write_region / bm_scene_read_region): a box of voxels as a
	// volume V[z][y][x] of one byte per voxel (non-zero = solid), x contiguous, rows and slices at the region's pitches, in host memory or
	// in memory of the scene's device.  A write is ordered like an edit; a read is issued like a query on hip_stream.
	struct Region : bm_region {
		// voxels lo <= v < hi; pitches in bytes, 0 = tight
		Region(const int lo_[3], const int hi_[3], int64_t row_pitch_ = 0, int64_t slice_pitch_ = 0) : bm_region{} {
			for (int k = 0; k < 3; ++k) { lo[k] = lo_[k]; hi[k] = hi_[k]; }
			row_pitch = row_pitch_;
			slice_pitch = slice_pitch_;
		}
		size_t voxels() const { return static_cast<size_t>(hi[0] - lo[0]) * static_cast<size_t>(hi[1] - lo[1]) * static_cast<size_t>(hi[2] - lo[2]); }
	};
	void write_region(const Region& region, const uint8_t* voxels, int op = BM_REGION_REPLACE, int where = BM_VOXELS_HOST, void* hip_stream = nullptr) {
		BM_CHECKED(bm_scene_write_region(gpuScene.handle, &region, op, voxels, where, hip_stream));
	}
	void read_region(const Region& region, uint8_t* voxels, int where = BM_VOXELS_HOST, void* hip_stream = nullptr) {
		BM_CHECKED(bm_scene_read_region(gpuScene.handle, &region, voxels, where, hip_stream));
	}

	// ray queries (no counterpart in the reference; bm_scene_cast_rays): the first hit of n rays, device buffers in and out, issued
	// like a frame on hip_stream (after every edit and upload issued before it), asynchronous to the host
	void cast_rays(int64_t n, const bm_ray* rays_dev, bm_ray_hit* hits_dev, uint32_t flags = 0, const float* lod_origin = nullptr,
				   void* hip_stream = nullptr) {
		BM_CHECKED(bm_scene_cast_rays(gpuScene.handle, n, rays_dev, hits_dev, flags, lod_origin, hip_stream));
	}
	// the pixel-centre rays of a width x height frame of `cam`, written on the device (bm_camera_pixel_rays_device): width * height records
	void pixel_rays(const Camera& cam, int width, int height, bm_ray* rays_dev, void* hip_stream = nullptr) {
		const bm_camera c = cam.to_c();
		BM_CHECKED(bm_camera_pixel_rays_device(gpuScene.handle, &c, width, height, rays_dev, hip_stream));
	}
	// the edge-avoiding a-trous filter of a frame of few samples (no counterpart in the reference; bm_denoise): accum_dev = (R, G, B, n) per
	// pixel, hits_dev = the first hit of every pixel's centre ray (pixel_rays + cast_rays with BM_QUERY_LOD around the camera), out_dev =
	// (c, 1) per pixel, which bm_resolve takes (may be accum_dev); workspace_dev: denoise_workspace_bytes() bytes of the caller's
	static size_t denoise_workspace_bytes(int width, int height) {
		size_t bytes = 0;
		BM_CHECKED(bm_denoise_workspace_bytes(width, height, &bytes));
		return bytes;
	}
	void denoise(int width, int height, const float* accum_dev, const bm_ray_hit* hits_dev, float* out_dev, void* workspace_dev, size_t workspace_bytes,
				 int iterations = 5, float sigma_l = 4.f, void* hip_stream = nullptr) {
		const bm_denoise_params p = {width, height, iterations, sigma_l, 0u, 0u};
		BM_CHECKED(bm_denoise(gpuScene.handle, &p, accum_dev, hits_dev, out_dev, workspace_dev, workspace_bytes, hip_stream));
	}
	// temporal accumulation for a moving camera (no counterpart in the reference; bm_reproject): accum_dev = the frame just rendered with
	// `cam`, hits_dev = its guides as for denoise, history_prev_dev = the history of the frame before, rendered with `cam_prev`, or null
	// (no history); history_out_dev = the new history, history_bytes() bytes, never the previous one: two histories take turns.  A history
	// begins with an accumulation buffer of up to max_history + the frame's own samples per pixel, which denoise and bm_resolve take.
	static size_t history_bytes(int width, int height) {
		size_t bytes = 0;
		BM_CHECKED(bm_history_bytes(width, height, &bytes));
		return bytes;
	}
	void reproject(int width, int height, const Camera& cam, const Camera* cam_prev, const float* accum_dev, const bm_ray_hit* hits_dev,
				   const void* history_prev_dev, void* history_out_dev, float max_history = 32.f, void* hip_stream = nullptr) {
		const bm_reproject_params p = {width, height, max_history, 0u, 0u};
		const bm_camera c = cam.to_c();
		bm_camera before{};
		if (cam_prev) before = cam_prev->to_c();
		BM_CHECKED(bm_reproject(gpuScene.handle, &p, &c, cam_prev ? &before : nullptr, accum_dev, hits_dev, history_prev_dev, history_out_dev, hip_stream));
	}
	// the hit under pixel (x, y) of a width x height frame of `cam`: one ray through the pixel's centre, one query, then the host waits.
	// level -1 = nothing there; level 3 = the brick is not resident yet (service the load queue, pick again)
	bm_ray_hit pick(const Camera& cam, int width, int height, int x, int y) {
		const float px = static_cast<float>(x) + 0.5f, py = static_cast<float>(y) + 0.5f;
		bm_ray ray{};
		cam.pixel_rays(width, height, 1, &px, &py, &ray);
		void* buf = nullptr;
		BM_CHECKED(bm_buffer_alloc(device_, sizeof(bm_ray) + sizeof(bm_ray_hit), &buf));
		bm_ray* d_ray = static_cast<bm_ray*>(buf);
		bm_ray_hit* d_hit = reinterpret_cast<bm_ray_hit*>(static_cast<char*>(buf) + sizeof(bm_ray));
		BM_CHECKED(bm_buffer_write(device_, d_ray, &ray, sizeof ray));
		cast_rays(1, d_ray, d_hit);
		bm_ray_hit hit{};
		BM_CHECKED(bm_buffer_read(device_, &hit, d_hit, sizeof hit)); // (waits for the device)
		BM_CHECKED(bm_buffer_free(device_, buf));
		return hit;
	}

	// volume queries (no counterpart in the reference; bm_scene_query_volumes): solid voxels, their bounds and the unresolved brick cells
	// of n boxes or spheres, device buffers in and out, issued like a ray query on hip_stream, asynchronous to the host
	struct Volume : bm_volume {
		static Volume box(const int lo_[3], const int hi_[3]) {
			Volume v{};
			v.shape = BM_EDIT_BOX;
			for (int k = 0; k < 3; ++k) { v.lo[k] = lo_[k]; v.hi[k] = hi_[k]; }
			return v;
		}
		static Volume sphere(const int center_[3], int radius_) {
			Volume v{};
			v.shape = BM_EDIT_SPHERE; v.radius = radius_;
			for (int k = 0; k < 3; ++k) v.center[k] = center_[k];
			return v;
		}
	};
	void query_volumes(int64_t n, const bm_volume* volumes_dev, bm_volume_result* results_dev, uint32_t flags = 0, void* hip_stream = nullptr) {
		BM_CHECKED(bm_scene_query_volumes(gpuScene.handle, n, volumes_dev, results_dev, flags, hip_stream));
	}
	// one shape, one query, then the host waits
	bm_volume_result query_volume(const bm_volume& volume, uint32_t flags = 0) {
		void* buf = nullptr;
		BM_CHECKED(bm_buffer_alloc(device_, sizeof(bm_volume) + sizeof(bm_volume_result), &buf));
		bm_volume_result* d_result = static_cast<bm_volume_result*>(buf);
		bm_volume* d_volume = reinterpret_cast<bm_volume*>(static_cast<char*>(buf) + sizeof(bm_volume_result));
		BM_CHECKED(bm_buffer_write(device_, d_volume, &volume, sizeof volume));
		query_volumes(1, d_volume, d_result, flags);
		bm_volume_result result{};
		BM_CHECKED(bm_buffer_read(device_, &result, d_result, sizeof result)); // (waits for the device)
		BM_CHECKED(bm_buffer_free(device_, buf));
		return result;
	}

	// connected components (no counterpart in the reference; bm_scene_label_region ...): which voxels of the box lo <= v < hi hang together
	// by faces.  labels_dev: a tight int32 volume [z][y][x] of device memory, count_dev: a uint64 there; issued like a query on hip_stream
	void label_region(const int lo[3], const int hi[3], int32_t* labels_dev, uint64_t* count_dev, void* hip_stream = nullptr) {
		BM_CHECKED(bm_scene_label_region(gpuScene.handle, lo, hi, 0u, labels_dev, count_dev, hip_stream));
	}
	// the first min(capacity, count) records of the table of such a label volume, in ascending label
	void label_components(const int lo[3], const int hi[3], const int32_t* labels_dev, bm_component* comps_dev, int64_t capacity, void* hip_stream = nullptr) {
		BM_CHECKED(bm_scene_label_components(gpuScene.handle, lo, hi, labels_dev, comps_dev, capacity, hip_stream));
	}
	// mask_dev[z][y][x] = chosen_dev[record of the voxel's label], 0 for empty voxels and labels outside the n records: what write_region takes
	void label_mask(const int lo[3], const int hi[3], const int32_t* labels_dev, const bm_component* comps_dev, int64_t n, const uint8_t* chosen_dev,
					uint8_t* mask_dev, void* hip_stream = nullptr) {
		BM_CHECKED(bm_scene_label_mask(gpuScene.handle, lo, hi, labels_dev, comps_dev, n, chosen_dev, mask_dev, hip_stream));
	}
	// Clear every voxel of the box whose component (inside the box) has no voxel on one of the `anchor` faces of (box and world) -- bits as
	// bm_component::faces; the default anchors to the four sides and the bottom.  Returns {pieces, voxels} removed.  The host waits.
	struct Removed { uint64_t pieces, voxels; };
	Removed remove_floating(const int lo[3], const int hi[3], uint32_t anchor = 0x1Fu) {
		Removed out{0, 0};
		const size_t voxels = Region(lo, hi).voxels();
		if (voxels == 0) return out;
		void* buf = nullptr; // the count, the labels, then the mask
		BM_CHECKED(bm_buffer_alloc(device_, 8 + voxels * 5, &buf));
		uint64_t* d_count = static_cast<uint64_t*>(buf);
		int32_t* d_labels = reinterpret_cast<int32_t*>(static_cast<char*>(buf) + 8);
		uint8_t* d_mask = reinterpret_cast<uint8_t*>(d_labels + voxels);
		void* table = nullptr;
		try {
			label_region(lo, hi, d_labels, d_count);
			uint64_t count = 0;
			BM_CHECKED(bm_buffer_read(device_, &count, d_count, sizeof count)); // (waits for the device)
			if (count > 0) {
				BM_CHECKED(bm_buffer_alloc(device_, count * (sizeof(bm_component) + 1), &table));
				bm_component* d_comps = static_cast<bm_component*>(table);
				uint8_t* d_chosen = reinterpret_cast<uint8_t*>(d_comps + count);
				label_components(lo, hi, d_labels, d_comps, static_cast<int64_t>(count));
				std::vector<bm_component> comps(count);
				BM_CHECKED(bm_buffer_read(device_, comps.data(), d_comps, count * sizeof(bm_component)));
				std::vector<uint8_t> chosen(count);
				for (uint64_t i = 0; i < count; ++i)
					if ((comps[i].faces & anchor) == 0) { chosen[i] = 1; ++out.pieces; out.voxels += comps[i].voxels; }
				if (out.pieces > 0) {
					BM_CHECKED(bm_buffer_write(device_, d_chosen, chosen.data(), count));
					label_mask(lo, hi, d_labels, d_comps, static_cast<int64_t>(count), d_chosen, d_mask);
					write_region(Region(lo, hi), d_mask, BM_EDIT_CLEAR, BM_VOXELS_DEVICE);
				}
			}
		} catch (...) {
			if (table) (void)bm_buffer_free(device_, table);
			(void)bm_buffer_free(device_, buf);
			throw;
		}
		if (table) BM_CHECKED(bm_buffer_free(device_, table));
		BM_CHECKED(bm_buffer_free(device_, buf));
		return out;
	}

	// rigid settling (no counterpart in the reference; bm_settle): the chosen pieces of a tight int32 label volume of `extent` in device memory
	// fall straight down and land; out_dev (uint8: 0 empty, 1 stayed, 2 fell), drops_dev (int32 per record) and result_dev receive the
	// outcome; workspace_dev: settle_workspace_bytes() bytes of the caller's.  Returns when the result stands.
	static size_t settle_workspace_bytes(const int32_t extent[3], int64_t n) {
		size_t bytes = 0;
		BM_CHECKED(bm_settle_workspace_bytes(extent, n, &bytes));
		return bytes;
	}
	void settle(const int32_t extent[3], const int32_t* labels_dev, const bm_component* comps_dev, int64_t n, const uint8_t* chosen_dev, uint8_t* out_dev, int32_t* drops_dev,
				bm_settle_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream = nullptr) {
		BM_CHECKED(bm_settle(gpuScene.handle, extent, labels_dev, comps_dev, n, chosen_dev, out_dev, drops_dev, result_dev, workspace_dev, workspace_bytes, 0u, hip_stream));
	}
	// Let the floating pieces of the box fall: the components of the box, those without a voxel on one of the `anchor` faces (bits as
	// bm_component::faces) are chosen, settle, write_region with replace.  A piece that touches an anchor face does not move, and the floor
	// is the bottom of the box: take lo[2] down to the ground.  Returns what moved.  The host waits.
	struct Settled { uint64_t pieces, voxels; uint32_t largest_drop; };
	Settled settle_floating(const int lo[3], const int hi[3], uint32_t anchor = 0x1Fu) {
		Settled out{0, 0, 0};
		const size_t voxels = Region(lo, hi).voxels();
		if (voxels == 0) return out;
		const int32_t extent[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
		void* buf = nullptr; // the result, the count, the labels, then out
		BM_CHECKED(bm_buffer_alloc(device_, 40 + voxels * 5, &buf));
		bm_settle_result* d_result = static_cast<bm_settle_result*>(buf);
		uint64_t* d_count = reinterpret_cast<uint64_t*>(static_cast<char*>(buf) + 32);
		int32_t* d_labels = reinterpret_cast<int32_t*>(static_cast<char*>(buf) + 40);
		uint8_t* d_out = reinterpret_cast<uint8_t*>(d_labels + voxels);
		void* table = nullptr;
		try {
			label_region(lo, hi, d_labels, d_count);
			uint64_t count = 0;
			BM_CHECKED(bm_buffer_read(device_, &count, d_count, sizeof count)); // (waits for the device)
			if (count > 0) {
				const size_t ws_bytes = settle_workspace_bytes(extent, static_cast<int64_t>(count));
				const size_t at_drops = count * sizeof(bm_component), at_ws = at_drops + count * 4, at_chosen = at_ws + ((ws_bytes + 3) & ~size_t{3});
				BM_CHECKED(bm_buffer_alloc(device_, at_chosen + count, &table)); // the records, the drops, the workspace, then chosen
				char* base = static_cast<char*>(table);
				bm_component* d_comps = static_cast<bm_component*>(table);
				label_components(lo, hi, d_labels, d_comps, static_cast<int64_t>(count));
				std::vector<bm_component> comps(count);
				BM_CHECKED(bm_buffer_read(device_, comps.data(), d_comps, count * sizeof(bm_component)));
				std::vector<uint8_t> chosen(count);
				bool any = false;
				for (uint64_t i = 0; i < count; ++i)
					if ((comps[i].faces & anchor) == 0) { chosen[i] = 1; any = true; }
				if (any) {
					BM_CHECKED(bm_buffer_write(device_, base + at_chosen, chosen.data(), count));
					settle(extent, d_labels, d_comps, static_cast<int64_t>(count), reinterpret_cast<const uint8_t*>(base + at_chosen), d_out, reinterpret_cast<int32_t*>(base + at_drops),
						   d_result, base + at_ws, ws_bytes);
					bm_settle_result result{};
					BM_CHECKED(bm_buffer_read(device_, &result, d_result, sizeof result));
					out = {result.moved_pieces, result.moved_voxels, result.largest_drop};
					if (result.moved_voxels > 0) write_region(Region(lo, hi), d_out, BM_REGION_REPLACE, BM_VOXELS_DEVICE);
				}
			}
		} catch (...) {
			if (table) (void)bm_buffer_free(device_, table);
			(void)bm_buffer_free(device_, buf);
			throw;
		}
		if (table) BM_CHECKED(bm_buffer_free(device_, table));
		BM_CHECKED(bm_buffer_free(device_, buf));
		return out;
	}

	// triangle meshes -> voxels (no counterpart in the reference; bm_voxelize): n triangles of 9 floats in device memory fill the byte volume
	// of `params` with 0 / 1; result_dev: null, or a bm_voxelize_result there; workspace_dev: voxelize_workspace_bytes() bytes of the caller's
	static size_t voxelize_workspace_bytes(const bm_voxelize_params& params, int64_t n) {
		size_t bytes = 0;
		BM_CHECKED(bm_voxelize_workspace_bytes(&params, n, &bytes));
		return bytes;
	}
	void voxelize(const bm_voxelize_params& params, int64_t n, const float* triangles_dev, uint8_t* volume_dev, bm_voxelize_result* result_dev, void* workspace_dev,
				  size_t workspace_bytes, void* hip_stream = nullptr) {
		BM_CHECKED(bm_voxelize(gpuScene.handle, &params, n, triangles_dev, volume_dev, result_dev, workspace_dev, workspace_bytes, hip_stream));
	}
	// Voxelize n triangles of HOST memory (9 floats each, world voxel units) over their own bounds, clipped to the world, and write the
	// result into the scene with `op` (BM_EDIT_SET adds the mesh, BM_EDIT_CLEAR carves it out).  Returns the result record and the number of
	// voxels of the box in `box_voxels`; a mesh wholly outside the world writes nothing.  The host waits.
	bm_voxelize_result write_mesh(const float* triangles, int64_t n, int op = BM_EDIT_SET, uint32_t mode = BM_VOXELIZE_SURFACE | BM_VOXELIZE_SOLID,
								  size_t* box_voxels = nullptr) {
		bm_voxelize_result out{0, 0, 0};
		if (box_voxels) *box_voxels = 0;
		bm_scene_info info;
		BM_CHECKED(bm_scene_get_info(gpuScene.handle, &info));
		const int world[3] = {info.grid_size, info.grid_size, info.grid_height};
		int lo[3], hi[3];
		for (int a = 0; a < 3; ++a) {
			double mn = 1e30, mx = -1e30;
			for (int64_t i = 0; i < 3 * n; ++i) {
				const double v = triangles[3 * i + a];
				if (!(v - v == 0)) continue; // not finite
				mn = v < mn ? v : mn;
				mx = v > mx ? v : mx;
			}
			if (mn > mx) return out;
			const double first = std::floor(mn) - 1, last = std::floor(mx) + 1; // the voxels a cube of which can touch the mesh
			lo[a] = first < 0 ? 0 : (first > world[a] ? world[a] : static_cast<int>(first));
			hi[a] = last < 0 ? 0 : (last > world[a] ? world[a] : static_cast<int>(last));
			if (hi[a] <= lo[a]) return out;
		}
		bm_voxelize_params p{};
		for (int a = 0; a < 3; ++a) { p.lo[a] = lo[a]; p.extent[a] = hi[a] - lo[a]; }
		p.mode = mode;
		const size_t voxels = Region(lo, hi).voxels(), tri_bytes = static_cast<size_t>(n) * 9 * sizeof(float), ws_bytes = voxelize_workspace_bytes(p, n);
		const size_t at_tri = 16, at_vol = at_tri + (tri_bytes + 15) / 16 * 16, at_ws = at_vol + (voxels + 15) / 16 * 16;
		void* buf = nullptr; // the result, the triangles, the volume, then the workspace
		BM_CHECKED(bm_buffer_alloc(device_, at_ws + ws_bytes, &buf));
		char* base = static_cast<char*>(buf);
		try {
			BM_CHECKED(bm_buffer_write(device_, base + at_tri, triangles, tri_bytes));
			voxelize(p, n, reinterpret_cast<const float*>(base + at_tri), reinterpret_cast<uint8_t*>(base + at_vol), reinterpret_cast<bm_voxelize_result*>(base),
					 base + at_ws, ws_bytes);
			write_region(Region(lo, hi), reinterpret_cast<const uint8_t*>(base + at_vol), op, BM_VOXELS_DEVICE);
			BM_CHECKED(bm_buffer_read(device_, &out, base, sizeof out)); // (waits for the device)
		} catch (...) {
			(void)bm_buffer_free(device_, buf);
			throw;
		}
		BM_CHECKED(bm_buffer_free(device_, buf));
		if (box_voxels) *box_voxels = voxels;
		return out;
	}

	// voxels -> the quads of their surface (no counterpart in the reference; bm_mesh_quads): the byte volume of `params` in device memory
	// gives its first `capacity` quads in quads_dev (null with capacity 0: the counting call) and the totals in result_dev;
	// workspace_dev: mesh_workspace_bytes() bytes of the caller's
	static size_t mesh_workspace_bytes(const bm_mesh_params& params) {
		size_t bytes = 0;
		BM_CHECKED(bm_mesh_workspace_bytes(&params, &bytes));
		return bytes;
	}
	void mesh_quads(const bm_mesh_params& params, const uint8_t* volume_dev, bm_quad* quads_dev, uint64_t capacity, bm_mesh_result* result_dev, void* workspace_dev,
					size_t workspace_bytes, void* hip_stream = nullptr) {
		BM_CHECKED(bm_mesh_quads(gpuScene.handle, &params, volume_dev, quads_dev, capacity, result_dev, workspace_dev, workspace_bytes, hip_stream));
	}
	// n quads -> 2 n triangles of 9 floats, both in device memory: what voxelize reads
	void mesh_triangles(const bm_quad* quads_dev, int64_t n, float* triangles_dev, void* hip_stream = nullptr) {
		BM_CHECKED(bm_mesh_triangles(gpuScene.handle, quads_dev, n, triangles_dev, hip_stream));
	}
	// The surface of the voxels of `region` (its lo and hi; the pitches are not used) of the live scene, closed at the box's sides, in HOST
	// memory: the quads in the contract's order and, when `triangles` is given, their 2 n triangles of 9 floats.  The box is read on the
	// device (read_region), counted, then emitted; the host waits.
	struct Mesh {
		bm_mesh_result result{0, 0};
		std::vector<bm_quad> quads;
	};
	Mesh extract_mesh(const Region& region, std::vector<float>* triangles = nullptr, uint32_t flags = 0) {
		Mesh out;
		if (triangles) triangles->clear();
		bm_mesh_params p{};
		for (int a = 0; a < 3; ++a) { p.lo[a] = region.lo[a]; p.extent[a] = region.hi[a] - region.lo[a]; }
		p.flags = flags;
		const size_t voxels = Region(region.lo, region.hi).voxels(), ws_bytes = mesh_workspace_bytes(p);
		const size_t at_ws = 16, at_vol = at_ws + (ws_bytes + 15) / 16 * 16;
		void* buf = nullptr; // the result, the workspace, then the volume
		void* out_buf = nullptr; // the quads, then the triangles
		BM_CHECKED(bm_buffer_alloc(device_, at_vol + voxels, &buf));
		char* base = static_cast<char*>(buf);
		try {
			read_region(Region(region.lo, region.hi), reinterpret_cast<uint8_t*>(base + at_vol), BM_VOXELS_DEVICE);
			mesh_quads(p, reinterpret_cast<const uint8_t*>(base + at_vol), nullptr, 0, reinterpret_cast<bm_mesh_result*>(base), base + at_ws, ws_bytes);
			BM_CHECKED(bm_buffer_read(device_, &out.result, base, sizeof out.result)); // (waits for the device)
			const size_t n = static_cast<size_t>(out.result.quads);
			if (n > 0) {
				const size_t quad_bytes = n * sizeof(bm_quad), tri_bytes = triangles ? n * 18 * sizeof(float) : 0;
				BM_CHECKED(bm_buffer_alloc(device_, quad_bytes + tri_bytes, &out_buf));
				char* q = static_cast<char*>(out_buf);
				mesh_quads(p, reinterpret_cast<const uint8_t*>(base + at_vol), reinterpret_cast<bm_quad*>(q), n, reinterpret_cast<bm_mesh_result*>(base), base + at_ws, ws_bytes);
				out.quads.resize(n);
				if (triangles) {
					mesh_triangles(reinterpret_cast<const bm_quad*>(q), static_cast<int64_t>(n), reinterpret_cast<float*>(q + quad_bytes));
					triangles->resize(n * 18);
					BM_CHECKED(bm_buffer_read(device_, triangles->data(), q + quad_bytes, tri_bytes));
				}
				BM_CHECKED(bm_buffer_read(device_, out.quads.data(), q, quad_bytes));
			}
		} catch (...) {
			(void)bm_buffer_free(device_, buf);
			if (out_buf) (void)bm_buffer_free(device_, out_buf);
			throw;
		}
		BM_CHECKED(bm_buffer_free(device_, buf));
		if (out_buf) BM_CHECKED(bm_buffer_free(device_, out_buf));
		return out;
	}

	// voxels -> their exact squared distance to the nearest source (no counterpart in the reference; bm_distance_field): the byte volume of
	// `params` in device memory gives the tight field dist_dev and the record result_dev; workspace_dev: distance_workspace_bytes() bytes of
	// the caller's
	static size_t distance_workspace_bytes(const bm_distance_params& params) {
		size_t bytes = 0;
		BM_CHECKED(bm_distance_workspace_bytes(&params, &bytes));
		return bytes;
	}
	void distance_field(const bm_distance_params& params, const uint8_t* volume_dev, uint32_t* dist_dev, bm_distance_result* result_dev, void* workspace_dev,
						size_t workspace_bytes, void* hip_stream = nullptr) {
		BM_CHECKED(bm_distance_field(gpuScene.handle, &params, volume_dev, dist_dev, result_dev, workspace_dev, workspace_bytes, hip_stream));
	}
	// count voxels of a field -> the byte volume (dist <= limit_sq) ? 1 : 0 (BM_DISTANCE_MASK_ABOVE: the opposite): what write_region takes
	void distance_mask(uint64_t count, const uint32_t* dist_dev, uint32_t limit_sq, uint8_t* volume_out_dev, uint32_t flags = 0, void* hip_stream = nullptr) {
		BM_CHECKED(bm_distance_mask(gpuScene.handle, count, dist_dev, limit_sq, flags, volume_out_dev, hip_stream));
	}
	// How far the voxels of `region` (its lo and hi; the pitches are not used) of the live scene are from the nearest solid voxel of the
	// box: the record (max_at and max_sq: the centre, as an index into the box, and the squared radius of the largest empty ball) and, when
	// `field` is given, the distances in HOST memory.  The box is read on the device (read_region); the host waits.
	bm_distance_result clearance(const Region& region, std::vector<uint32_t>* field = nullptr) {
		bm_distance_result out{};
		bm_distance_params p{};
		for (int a = 0; a < 3; ++a) p.extent[a] = region.hi[a] - region.lo[a];
		const size_t voxels = Region(region.lo, region.hi).voxels(), ws_bytes = distance_workspace_bytes(p);
		const size_t at_ws = 32, at_field = at_ws + ws_bytes, at_vol = at_field + voxels * 4;
		void* buf = nullptr; // the result, the workspace, the field, then the volume
		BM_CHECKED(bm_buffer_alloc(device_, at_vol + voxels, &buf));
		char* base = static_cast<char*>(buf);
		try {
			read_region(Region(region.lo, region.hi), reinterpret_cast<uint8_t*>(base + at_vol), BM_VOXELS_DEVICE);
			distance_field(p, reinterpret_cast<const uint8_t*>(base + at_vol), reinterpret_cast<uint32_t*>(base + at_field), reinterpret_cast<bm_distance_result*>(base),
						   base + at_ws, ws_bytes);
			BM_CHECKED(bm_buffer_read(device_, &out, base, sizeof out)); // (waits for the device)
			if (field) {
				field->resize(voxels);
				BM_CHECKED(bm_buffer_read(device_, field->data(), base + at_field, voxels * 4));
			}
		} catch (...) {
			(void)bm_buffer_free(device_, buf);
			throw;
		}
		BM_CHECKED(bm_buffer_free(device_, buf));
		return out;
	}
	// Dilate (grow) or erode (shrink) the live scene inside the box lo <= v < hi with a Euclidean ball of squared radius radius_sq >= 1.
	// The box enlarged by m = ceil(sqrt(radius_sq)) on every side is read (read_region gives 0 outside the world); grow takes its distance
	// to solid and sets the voxels of the box with D <= radius_sq, shrink takes its distance to empty and clears them.  Because the margin
	// covers the radius, the result inside the box is that of the operation on the whole world; beyond the world's border counts as
	// empty.  Returns the number of voxels changed.  The host waits.
	uint64_t grow(const int lo[3], const int hi[3], uint32_t radius_sq) { return morph(lo, hi, radius_sq, false); }
	uint64_t shrink(const int lo[3], const int hi[3], uint32_t radius_sq) { return morph(lo, hi, radius_sq, true); }

	// voxels + seeds -> exact shortest face-step distances (no counterpart in the reference; bm_travel_field): the byte volume of `params` in
	// device memory (non-zero = blocked) and n seeds (x, y, z) there give the tight field field_dev and the record result_dev;
	// workspace_dev: travel_workspace_bytes() bytes of the caller's.  Returns when the field stands.
	static size_t travel_workspace_bytes(const bm_travel_params& params) {
		size_t bytes = 0;
		BM_CHECKED(bm_travel_workspace_bytes(&params, &bytes));
		return bytes;
	}
	void travel_field(const bm_travel_params& params, const uint8_t* volume_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev, bm_travel_result* result_dev,
					  void* workspace_dev, size_t workspace_bytes, void* hip_stream = nullptr) {
		BM_CHECKED(bm_travel_field(gpuScene.handle, &params, volume_dev, seeds_dev, n, field_dev, result_dev, workspace_dev, workspace_bytes, hip_stream));
	}
	// n starts -> the first `capacity` voxels of every path down the field and the paths' lengths (bm_travel_paths); asynchronous
	void travel_paths(const int32_t extent[3], const uint32_t* field_dev, const int32_t* starts_dev, int64_t n, int32_t capacity, int32_t* path_dev, int32_t* lengths_dev,
					  void* hip_stream = nullptr) {
		BM_CHECKED(bm_travel_paths(gpuScene.handle, extent, field_dev, starts_dev, n, capacity, path_dev, lengths_dev, hip_stream));
	}
	// A shortest face-step path through the empty voxels of the live scene from world voxel `start` to world voxel `goal`, inside the
	// bounding box of the two enlarged by 32 and clipped to the world: the box is read on the device (read_region), the travel field is
	// seeded at the goal, and the walk goes down from the start.  Returns the path's world voxels (x, y, z), the start first and the goal
	// last; empty when there is no path (within max_steps, 0 = no limit).  The host waits.
	std::vector<std::array<int, 3>> find_path(const int start[3], const int goal[3], uint32_t max_steps = 0) {
		std::vector<std::array<int, 3>> out;
		bm_scene_info info;
		BM_CHECKED(bm_scene_get_info(gpuScene.handle, &info));
		const int world[3] = {info.grid_size, info.grid_size, info.grid_height};
		int lo[3], hi[3];
		int32_t ends[6]; // the goal (the seed), then the start, in the box's coordinates
		bm_travel_params p{};
		for (int a = 0; a < 3; ++a) {
			const int mn = start[a] < goal[a] ? start[a] : goal[a], mx = start[a] < goal[a] ? goal[a] : start[a];
			lo[a] = mn - 32 > 0 ? mn - 32 : 0;
			hi[a] = mx + 33 < world[a] ? mx + 33 : world[a];
			if (hi[a] <= lo[a]) return out;
			p.extent[a] = hi[a] - lo[a];
			ends[a] = goal[a] - lo[a];
			ends[3 + a] = start[a] - lo[a];
		}
		p.max_steps = max_steps;
		const size_t voxels = Region(lo, hi).voxels(), ws_bytes = travel_workspace_bytes(p);
		const size_t at_ends = 32, at_len = at_ends + 32, at_ws = at_len + 16, at_field = at_ws + ws_bytes, at_vol = at_field + voxels * 4;
		void* buf = nullptr; // the result, the two ends, the path's length, the workspace, the field, then the volume
		BM_CHECKED(bm_buffer_alloc(device_, at_vol + voxels, &buf));
		char* base = static_cast<char*>(buf);
		void* path_buf = nullptr;
		try {
			BM_CHECKED(bm_buffer_write(device_, base + at_ends, ends, sizeof ends));
			read_region(Region(lo, hi), reinterpret_cast<uint8_t*>(base + at_vol), BM_VOXELS_DEVICE);
			uint32_t* field = reinterpret_cast<uint32_t*>(base + at_field);
			travel_field(p, reinterpret_cast<const uint8_t*>(base + at_vol), reinterpret_cast<const int32_t*>(base + at_ends), 1, field, reinterpret_cast<bm_travel_result*>(base),
						 base + at_ws, ws_bytes);
			const bool inside = ends[3] >= 0 && ends[4] >= 0 && ends[5] >= 0 && ends[3] < p.extent[0] && ends[4] < p.extent[1] && ends[5] < p.extent[2];
			uint32_t t = BM_TRAVEL_NONE;
			if (inside) BM_CHECKED(bm_buffer_read(device_, &t, field + (static_cast<size_t>(ends[5]) * p.extent[1] + ends[4]) * p.extent[0] + ends[3], sizeof t));
			if (t != BM_TRAVEL_NONE) {
				const int32_t capacity = static_cast<int32_t>(t) + 1;
				BM_CHECKED(bm_buffer_alloc(device_, static_cast<size_t>(capacity) * 12, &path_buf));
				travel_paths(p.extent, field, reinterpret_cast<const int32_t*>(base + at_ends) + 3, 1, capacity, static_cast<int32_t*>(path_buf),
							 reinterpret_cast<int32_t*>(base + at_len));
				std::vector<int32_t> host(static_cast<size_t>(capacity) * 3);
				BM_CHECKED(bm_buffer_read(device_, host.data(), path_buf, host.size() * 4)); // (waits for the device)
				out.resize(static_cast<size_t>(capacity));
				for (size_t k = 0; k < out.size(); ++k) out[k] = {host[3 * k] + lo[0], host[3 * k + 1] + lo[1], host[3 * k + 2] + lo[2]};
			}
		} catch (...) {
			if (path_buf) (void)bm_buffer_free(device_, path_buf);
			(void)bm_buffer_free(device_, buf);
			throw;
		}
		if (path_buf) BM_CHECKED(bm_buffer_free(device_, path_buf));
		BM_CHECKED(bm_buffer_free(device_, buf));
		return out;
	}

	// ground navigation (no counterpart in the reference; bm_foot_room, bm_foot_field, bm_foot_paths): the byte volume of `params` in device
	// memory gives a tight room volume (one byte per voxel); the room bytes and n seeds give the tight uint32 walk field and the result;
	// a field gives paths.  workspace_dev: foot_workspace_bytes() bytes of the caller's.  foot_field returns when the field stands, the
	// other two are asynchronous.
	static size_t foot_workspace_bytes(const bm_foot_params& params) {
		size_t bytes = 0;
		BM_CHECKED(bm_foot_workspace_bytes(&params, &bytes));
		return bytes;
	}
	void foot_room(const bm_foot_params& params, const uint8_t* volume_dev, uint8_t* room_dev, void* hip_stream = nullptr) {
		BM_CHECKED(bm_foot_room(gpuScene.handle, &params, volume_dev, room_dev, hip_stream));
	}
	void foot_field(const bm_foot_params& params, const uint8_t* room_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev, bm_foot_result* result_dev, void* workspace_dev,
					size_t workspace_bytes, void* hip_stream = nullptr) {
		BM_CHECKED(bm_foot_field(gpuScene.handle, &params, room_dev, seeds_dev, n, field_dev, result_dev, workspace_dev, workspace_bytes, hip_stream));
	}
	void foot_paths(const bm_foot_params& params, const uint8_t* room_dev, const uint32_t* field_dev, const int32_t* starts_dev, int64_t n, int32_t capacity, int32_t* path_dev,
					int32_t* lengths_dev, void* hip_stream = nullptr) {
		BM_CHECKED(bm_foot_paths(gpuScene.handle, &params, room_dev, field_dev, starts_dev, n, capacity, path_dev, lengths_dev, hip_stream));
	}
	// A shortest walk from world voxel `start` to world voxel `goal` for an agent `height` voxels tall that climbs `climb` and drops `drop`
	// voxels per move, inside the box of find_path taken down by `drop`: the box is read on the device (read_region), the room bytes are
	// made with the floor where the box stands on the world's bottom, both ends are snapped to the highest stand at or below them in
	// their columns, the field is seeded at the goal with BM_FOOT_TOWARD, and the walk goes down from the start.  Returns the walk's world
	// voxels, the start's ground first and the goal's last; empty when there is no way on foot.  The host waits.
	std::vector<std::array<int, 3>> find_walk(const int start[3], const int goal[3], int height = 2, int climb = 1, int drop = 3) {
		std::vector<std::array<int, 3>> out;
		bm_scene_info info;
		BM_CHECKED(bm_scene_get_info(gpuScene.handle, &info));
		const int world[3] = {info.grid_size, info.grid_size, info.grid_height};
		int lo[3], hi[3];
		int32_t ends[6]; // the goal (the seed), then the start, in the box's coordinates
		bm_foot_params p{};
		for (int a = 0; a < 3; ++a) {
			const int mn = start[a] < goal[a] ? start[a] : goal[a], mx = start[a] < goal[a] ? goal[a] : start[a], down = a == 2 ? 32 + drop : 32;
			lo[a] = mn - down > 0 ? mn - down : 0;
			hi[a] = mx + 33 < world[a] ? mx + 33 : world[a];
			if (hi[a] <= lo[a]) return out;
			p.extent[a] = hi[a] - lo[a];
			ends[a] = goal[a] - lo[a];
			ends[3 + a] = start[a] - lo[a];
		}
		p.height = height;
		p.climb = climb;
		p.drop = drop;
		p.flags = BM_FOOT_TOWARD | (lo[2] == 0 ? 0u : BM_FOOT_NO_FLOOR);
		const size_t voxels = Region(lo, hi).voxels(), ws_bytes = foot_workspace_bytes(p);
		const size_t at_ends = 32, at_len = at_ends + 32, at_ws = at_len + 16, at_field = at_ws + ws_bytes, at_vol = at_field + voxels * 4, at_room = at_vol + voxels;
		void* buf = nullptr; // the result, the two ends, the path's length, the workspace, the field, the volume, then the room bytes
		BM_CHECKED(bm_buffer_alloc(device_, at_room + voxels, &buf));
		char* base = static_cast<char*>(buf);
		void* path_buf = nullptr;
		try {
			read_region(Region(lo, hi), reinterpret_cast<uint8_t*>(base + at_vol), BM_VOXELS_DEVICE);
			const uint8_t* room = reinterpret_cast<const uint8_t*>(base + at_room);
			foot_room(p, reinterpret_cast<const uint8_t*>(base + at_vol), reinterpret_cast<uint8_t*>(base + at_room));
			std::vector<uint8_t> cells(voxels);
			BM_CHECKED(bm_buffer_read(device_, cells.data(), room, voxels)); // (waits for the device)
			bool grounded = true;
			for (int e = 0; e < 2; ++e) { // the highest stand at or below each end
				int32_t* at = ends + 3 * e;
				bool found = false;
				if (at[0] >= 0 && at[1] >= 0 && at[2] >= 0 && at[0] < p.extent[0] && at[1] < p.extent[1] && at[2] < p.extent[2])
					for (int32_t z = at[2]; z >= 0 && !found; --z) {
						const uint8_t cell = cells[(static_cast<size_t>(z) * p.extent[1] + at[1]) * p.extent[0] + at[0]];
						if ((cell & 0x80u) && (cell & 0x7Fu) >= static_cast<unsigned>(height)) {
							at[2] = z;
							found = true;
						}
					}
				grounded = grounded && found;
			}
			if (grounded) {
				BM_CHECKED(bm_buffer_write(device_, base + at_ends, ends, sizeof ends));
				uint32_t* field = reinterpret_cast<uint32_t*>(base + at_field);
				foot_field(p, room, reinterpret_cast<const int32_t*>(base + at_ends), 1, field, reinterpret_cast<bm_foot_result*>(base), base + at_ws, ws_bytes);
				uint32_t t = BM_FOOT_NONE;
				BM_CHECKED(bm_buffer_read(device_, &t, field + (static_cast<size_t>(ends[5]) * p.extent[1] + ends[4]) * p.extent[0] + ends[3], sizeof t));
				if (t != BM_FOOT_NONE) {
					const int32_t capacity = static_cast<int32_t>(t) + 1;
					BM_CHECKED(bm_buffer_alloc(device_, static_cast<size_t>(capacity) * 12, &path_buf));
					foot_paths(p, room, field, reinterpret_cast<const int32_t*>(base + at_ends) + 3, 1, capacity, static_cast<int32_t*>(path_buf),
							   reinterpret_cast<int32_t*>(base + at_len));
					std::vector<int32_t> host(static_cast<size_t>(capacity) * 3);
					BM_CHECKED(bm_buffer_read(device_, host.data(), path_buf, host.size() * 4)); // (waits for the device)
					out.resize(static_cast<size_t>(capacity));
					for (size_t k = 0; k < out.size(); ++k) out[k] = {host[3 * k] + lo[0], host[3 * k + 1] + lo[1], host[3 * k + 2] + lo[2]};
				}
			}
		} catch (...) {
			if (path_buf) (void)bm_buffer_free(device_, path_buf);
			(void)bm_buffer_free(device_, buf);
			throw;
		}
		if (path_buf) BM_CHECKED(bm_buffer_free(device_, path_buf));
		BM_CHECKED(bm_buffer_free(device_, buf));
		return out;
	}

	// where water stands (no counterpart in the reference; bm_water_field, bm_water_mask): the byte volume of `params` in device memory
	// (non-zero = solid, z up), the open faces of its flags and n drains (x, y, z) there give the tight uint32 field of spill levels and the
	// record; a field gives the byte mask of its pools.  workspace_dev: water_workspace_bytes() bytes of the caller's.  water_field returns
	// when the field stands, water_mask is asynchronous.
	static size_t water_workspace_bytes(const bm_water_params& params) {
		size_t bytes = 0;
		BM_CHECKED(bm_water_workspace_bytes(&params, &bytes));
		return bytes;
	}
	void water_field(const bm_water_params& params, const uint8_t* volume_dev, const int32_t* drains_dev, int64_t n, uint32_t* field_dev, bm_water_result* result_dev,
					 void* workspace_dev, size_t workspace_bytes, void* hip_stream = nullptr) {
		BM_CHECKED(bm_water_field(gpuScene.handle, &params, volume_dev, drains_dev, n, field_dev, result_dev, workspace_dev, workspace_bytes, hip_stream));
	}
	void water_mask(const int32_t extent[3], const uint32_t* field_dev, uint32_t min_depth, uint8_t* mask_dev, void* hip_stream = nullptr) {
		BM_CHECKED(bm_water_mask(gpuScene.handle, extent, field_dev, min_depth, mask_dev, hip_stream));
	}
	// Where water stands in the box lo <= v < hi of the live scene: the box is read on the device (read_region) and its spill levels are
	// taken with the given faces open (default: the four sides), the drains (world voxels) and the sea (a world z; below lo[2] = none,
	// clamped into the box).  Returns the record; `field`, when given, gets the levels [z][y][x] in the box's coordinates (voxel - lo) and
	// `mask`, when given, the bytes of bm_water_mask at min_depth.  The host waits.
	bm_water_result pools(const int lo[3], const int hi[3], std::vector<uint32_t>* field = nullptr, std::vector<uint8_t>* mask = nullptr, uint32_t min_depth = 1,
						  const std::vector<std::array<int, 3>>& drains = {}, int sea_level = -1, uint32_t open_faces = 15u) {
		bm_water_params p{};
		for (int a = 0; a < 3; ++a) p.extent[a] = hi[a] - lo[a];
		const int sea = sea_level - lo[2];
		p.sea_level = sea_level < 0 || sea < 0 ? 0u : static_cast<uint32_t>(sea < p.extent[2] ? sea : p.extent[2]);
		p.flags = open_faces;
		std::vector<int32_t> local;
		for (const auto& d : drains)
			for (int a = 0; a < 3; ++a) local.push_back(d[a] - lo[a]);
		const size_t voxels = Region(lo, hi).voxels(), ws_bytes = water_workspace_bytes(p), drain_bytes = (local.size() * 4 + 15) & ~size_t{15};
		const size_t at_drains = 32, at_ws = at_drains + drain_bytes, at_field = at_ws + ws_bytes, at_vol = at_field + voxels * 4, at_mask = at_vol + ((voxels + 15) & ~size_t{15});
		void* buf = nullptr; // the result, the drains, the workspace, the field, the volume, then the mask
		BM_CHECKED(bm_buffer_alloc(device_, at_mask + voxels, &buf));
		char* base = static_cast<char*>(buf);
		bm_water_result rec{};
		try {
			if (!local.empty()) BM_CHECKED(bm_buffer_write(device_, base + at_drains, local.data(), local.size() * 4));
			read_region(Region(lo, hi), reinterpret_cast<uint8_t*>(base + at_vol), BM_VOXELS_DEVICE);
			uint32_t* levels = reinterpret_cast<uint32_t*>(base + at_field);
			water_field(p, reinterpret_cast<const uint8_t*>(base + at_vol), local.empty() ? nullptr : reinterpret_cast<const int32_t*>(base + at_drains),
						static_cast<int64_t>(drains.size()), levels, reinterpret_cast<bm_water_result*>(base), base + at_ws, ws_bytes);
			BM_CHECKED(bm_buffer_read(device_, &rec, base, sizeof rec));
			if (field) {
				field->resize(voxels);
				BM_CHECKED(bm_buffer_read(device_, field->data(), levels, voxels * 4));
			}
			if (mask) {
				water_mask(p.extent, levels, min_depth, reinterpret_cast<uint8_t*>(base + at_mask));
				mask->resize(voxels);
				BM_CHECKED(bm_buffer_read(device_, mask->data(), base + at_mask, voxels)); // (waits for the device)
			}
		} catch (...) {
			(void)bm_buffer_free(device_, buf);
			throw;
		}
		BM_CHECKED(bm_buffer_free(device_, buf));
		return rec;
	}

private:
	uint64_t morph(const int lo[3], const int hi[3], uint32_t radius_sq, bool erode) {
		bool bad = radius_sq < 1 || radius_sq > 3u * 16383u * 16383u;
		for (int a = 0; a < 3; ++a) bad = bad || hi[a] <= lo[a];
		if (bad) { // (as bm_assert reports a refused call)
			std::fprintf(stderr, "hip_assert: grow / shrink: a box that is not empty and radius_sq in 1 ... 3 * 16383^2 expected %s %d\n", __FILE__, __LINE__);
			std::exit(BM_EINVAL);
		}
		int m = 1;
		while (static_cast<uint32_t>(m) * static_cast<uint32_t>(m) < radius_sq) ++m;
		int big_lo[3], big_hi[3];
		bm_distance_params p{};
		for (int a = 0; a < 3; ++a) {
			big_lo[a] = lo[a] - m;
			big_hi[a] = hi[a] + m;
			p.extent[a] = big_hi[a] - big_lo[a];
		}
		p.flags = erode ? BM_DISTANCE_TO_EMPTY : 0u;
		const size_t voxels = Region(big_lo, big_hi).voxels(), ws_bytes = distance_workspace_bytes(p);
		const size_t at_ws = 32, at_field = at_ws + ws_bytes, at_vol = at_field + voxels * 4, at_mask = at_vol + voxels;
		void* buf = nullptr; // the result, the workspace, the field, the volume, then the mask
		BM_CHECKED(bm_buffer_alloc(device_, at_mask + voxels, &buf));
		char* base = static_cast<char*>(buf);
		uint64_t changed = 0;
		try {
			read_region(Region(big_lo, big_hi), reinterpret_cast<uint8_t*>(base + at_vol), BM_VOXELS_DEVICE);
			distance_field(p, reinterpret_cast<const uint8_t*>(base + at_vol), reinterpret_cast<uint32_t*>(base + at_field), reinterpret_cast<bm_distance_result*>(base),
						   base + at_ws, ws_bytes);
			distance_mask(voxels, reinterpret_cast<const uint32_t*>(base + at_field), radius_sq, reinterpret_cast<uint8_t*>(base + at_mask));
			// the box is the enlarged volume's inside: the same bytes at the enlarged volume's pitches
			const int64_t row = p.extent[0], slice = row * p.extent[1];
			const size_t inner = static_cast<size_t>(m) * static_cast<size_t>(slice + row + 1);
			write_region(Region(lo, hi, row, slice), reinterpret_cast<const uint8_t*>(base + at_mask + inner), erode ? BM_EDIT_CLEAR : BM_EDIT_SET, BM_VOXELS_DEVICE);
			std::vector<uint8_t> host(2 * voxels); // the volume as it was, then the mask
			BM_CHECKED(bm_buffer_read(device_, host.data(), base + at_vol, 2 * voxels)); // (waits for the device)
			for (int z = 0; z < hi[2] - lo[2]; ++z)
				for (int y = 0; y < hi[1] - lo[1]; ++y)
					for (int x = 0; x < hi[0] - lo[0]; ++x) {
						const size_t i = inner + static_cast<size_t>(z) * slice + static_cast<size_t>(y) * row + x;
						if (host[voxels + i] && (host[i] != 0) == erode) ++changed;
					}
		} catch (...) {
			(void)bm_buffer_free(device_, buf);
			throw;
		}
		BM_CHECKED(bm_buffer_free(device_, buf));
		return changed;
	}

	int device_;
};

// Which part of the frame this process renders (no counterpart in the reference, which is single-GPU: main.cpp:89 computes
// `multi_gpu` and never uses it): the frame's rows are dealt out in bands of `band_rows` rows, band b to rank b % count, and
// a rank's rows are packed in increasing y into its State's blit_buffer.  {0, 1} = the whole frame.
struct Shard {
	int rank = 0, count = 1;
	int band_rows = 8;  // rows per band: many bands per rank, so that every rank sees every part of the image (the job is as fast as its slowest rank)
};

struct State { // state.h:5-34 without the wavefront queues and the GL interop
	vec4* blit_buffer = nullptr; // device memory, float4 per pixel: rgb = radiance sum, a = terminated paths
	size_t screen_width, screen_height;
	int device;
	Shard shard;           // the rows blit_buffer holds (default: all of them)
	size_t local_rows = 0; // = screen_height for the whole frame

	State(size_t width, size_t height, int device_ = 0, Shard shard_ = {}) : screen_width(width), screen_height(height), device(device_), shard(shard_) { alloc(); }
	~State() { bm_buffer_free(device, blit_buffer); }
	void screen_resize(size_t width, size_t height) {
		screen_width = width;
		screen_height = height;
		BM_CHECKED(bm_buffer_free(device, blit_buffer));
		alloc();
	}

private:
	void alloc() {
		bm_frame_params fp{};
		fp.width = static_cast<int32_t>(screen_width); fp.height = static_cast<int32_t>(screen_height);
		fp.band_rows = shard.count > 1 ? shard.band_rows : fp.height; fp.shard_rank = shard.rank; fp.shard_count = shard.count;
		local_rows = static_cast<size_t>(bm_local_rows(&fp));
		void* p = nullptr;
		BM_CHECKED(bm_buffer_alloc(device, screen_width * (local_rows ? local_rows : 1) * sizeof(vec4), &p));
		BM_CHECKED(bm_buffer_zero(device, p, screen_width * (local_rows ? local_rows : 1) * sizeof(vec4), nullptr));
		blit_buffer = static_cast<vec4*>(p);
	}
};

namespace detail {
inline bm_camera camera_to_c() { return camera.to_c(); }
inline bm_frame_params frame_params(const State& state, int max_bounces) {
	bm_frame_params fp{};
	fp.width = static_cast<int32_t>(state.screen_width);
	fp.height = static_cast<int32_t>(state.screen_height);
	fp.spp = 1;
	fp.max_bounces = max_bounces;
	fp.base_frame = 1;
	fp.band_rows = state.shard.count > 1 ? state.shard.band_rows : fp.height;
	fp.shard_rank = state.shard.rank;
	fp.shard_count = state.shard.count;
	fp.sun_position[0] = sun_position.x;
	fp.sun_position[1] = sun_position.y;
	return fp;
}
inline bool camera_changed(const Camera& last) {
	return last.position.x != camera.position.x || last.position.y != camera.position.y || last.position.z != camera.position.z ||
		   last.direction.x != camera.direction.x || last.direction.y != camera.direction.y || last.direction.z != camera.direction.z ||
		   last.focalDistance != camera.focalDistance || last.lensRadius != camera.lensRadius;
}
} // namespace detail

namespace detail {
// the statics of launch_kernels (kernel.cu:369,387-403: frame counter, first call, last camera) shared by its two forms
struct FusedStatics {
	bool first_time = true;
	int sample_base = 0;
	Camera last;
};
inline FusedStatics& fused_statics() { static FusedStatics s; return s; }
// kernel.cu:387-403: a camera / sun change (or the first call) resets the accumulation; returns the frame parameters of the next call
inline bm_frame_params begin_frames(State& state, vec4* blit_buffer, int spp, int max_bounces) {
	FusedStatics& st = fused_statics();
	bool reset_buffer = st.first_time || camera_changed(st.last);
	st.first_time = false;
	if (sun_position_changed) {
		sun_position_changed = false;
		reset_buffer = true;
	}
	if (reset_buffer) {
		BM_CHECKED(bm_buffer_zero(state.device, blit_buffer, state.screen_width * state.local_rows * sizeof(vec4), nullptr));
		st.sample_base = 0;
	}
	bm_frame_params fp = frame_params(state, max_bounces);
	fp.spp = spp;
	fp.sample_base = st.sample_base;
	// a shard has few pixels and (usually) many samples: (4x4 chunk, sample) work items keep the persistent waves fed
	if (state.shard.count > 1) fp.flags |= BM_FLAG_SAMPLE_ITEMS;
	return fp;
}
} // namespace detail

// launch_kernels (launch.h:6, kernel.cu:366-439).  The cudaSurfaceObject_t and the three queue pointers of the
// reference signature are gone (no GL surface; paths live in registers); `spp` complete paths per pixel are
// traced per call instead of one bounce of every in-flight path.  As in the reference the call blocks until
// the frame is done (kernel.cu:431) and a camera / sun change resets the accumulation (kernel.cu:387-403).
inline int launch_kernels(State& state, vec4* blit_buffer, Scene::GPUScene gpuScene, int spp = 1, int max_bounces = 3) {
	const bm_camera cam = detail::camera_to_c();
	const bm_frame_params fp = detail::begin_frames(state, blit_buffer, spp, max_bounces);
	BM_CHECKED(bm_render_frame(gpuScene.handle, &cam, &fp, reinterpret_cast<float*>(blit_buffer), nullptr, nullptr));
	BM_CHECKED(bm_synchronize(gpuScene.handle));
	detail::fused_statics().sample_base += spp;
	detail::fused_statics().last = camera;
	return 0; // the reference always returns cudaSuccess (kernel.cu:438)
}

// `frames` consecutive iterations of the reference's frame loop (main.cpp:117-147: launch_kernels once per frame) for the current
// camera and sun as ONE launch of the persistent kernel (bm_render_frames, the "frame ring"): exactly the frames that many
// launch_kernels calls render -- each with its own sample offsets, ticket counters and rays, all accumulating into blit_buffer like
// consecutive frames of the reference (kernel.cu:319-322,341-343) -- but a wave that has run out of work in frame i starts on
// frame i+1 by itself, so the end of a frame is covered by the next one (1080p, 1 spp: 0.86 instead of 1.03 ms per frame).
// Blocks until the last frame is done.  A host whose camera moves every frame keeps calling launch_kernels.
inline int launch_frames(State& state, vec4* blit_buffer, Scene::GPUScene gpuScene, int frames, int spp = 1, int max_bounces = 3) {
	if (frames < 1) return 0;
	const bm_camera cam = detail::camera_to_c();
	const bm_frame_params first = detail::begin_frames(state, blit_buffer, spp, max_bounces);
	for (int done = 0; done < frames;) {
		const int n = frames - done < 256 ? frames - done : 256; // (bm_render_frames takes up to 256 frames per launch)
		std::vector<bm_camera> cams(static_cast<size_t>(n), cam);
		std::vector<bm_frame_params> fps(static_cast<size_t>(n), first);
		std::vector<float*> buffers(static_cast<size_t>(n), reinterpret_cast<float*>(blit_buffer));
		for (int i = 0; i < n; ++i) fps[static_cast<size_t>(i)].sample_base = first.sample_base + (done + i) * spp;
		BM_CHECKED(bm_render_frames(gpuScene.handle, n, cams.data(), fps.data(), buffers.data(), nullptr, nullptr));
		done += n;
	}
	BM_CHECKED(bm_synchronize(gpuScene.handle));
	detail::fused_statics().sample_base += frames * spp;
	detail::fused_statics().last = camera;
	return 0;
}

// ---- multi-GPU: one process (or thread) per GPU, every one with its own Scene replica, State shard and Comm.
// The per-frame loop of main.cpp:142-147 becomes, on every rank:
//     launch_kernels(state, state.blit_buffer, scene.gpuScene, spp);      // this rank's bands (state.shard)
//     scene.process_load_queue();
//     gather_frame(comm, state, frame_on_root);                           // ncclSend / ncclRecv + assembly, RCCL over xGMI
// INTEGRATION.md has the whole program.
struct Comm {
	bm_comm* handle = nullptr;
	int rank = 0, world = 1;
	// ncclGetUniqueId: called on ONE rank; hand the 128 bytes to the others (MPI_Bcast, a file, a socket)
	static void unique_id(unsigned char id[BM_COMM_ID_BYTES]) { BM_CHECKED(bm_comm_unique_id(id)); }
	Comm(int device, int rank_, int world_, const unsigned char id[BM_COMM_ID_BYTES]) : rank(rank_), world(world_) {
		BM_CHECKED(bm_comm_create(device, rank, world, id, &handle));
	}
	~Comm() { bm_comm_destroy(handle); }
	Comm(const Comm&) = delete;
	Comm& operator=(const Comm&) = delete;
	void barrier() { BM_CHECKED(bm_comm_barrier(handle, nullptr)); }
};

// The exchange of one frame: every rank's packed bands to `root`, assembled there into frame_on_root (height x width float4,
// device memory of the root; ignored on the other ranks).  Enqueued on the default stream behind the frame; returns at once.
inline void gather_frame(Comm& comm, const State& state, vec4* frame_on_root, int root = 0) {
	BM_CHECKED(bm_gather_frame(comm.handle, reinterpret_cast<const float*>(state.blit_buffer), reinterpret_cast<float*>(frame_on_root),
							   static_cast<int>(state.screen_height), static_cast<int>(state.screen_width), state.shard.count > 1 ? state.shard.band_rows : static_cast<int>(state.screen_height),
							   root, nullptr));
}

// The exchange of a BATCH of frames (what a rank rendered with launch_frames-style launches into one allocation of `count` packed
// shard buffers): one message per peer for the whole batch (bm_gather_frames).  packed = count x local_rows x width float4,
// frames_on_root = count x height x width float4 (ignored on the other ranks).
inline void gather_frames(Comm& comm, const State& state, const vec4* packed, vec4* frames_on_root, int count, int root = 0) {
	BM_CHECKED(bm_gather_frames(comm.handle, reinterpret_cast<const float*>(packed), reinterpret_cast<float*>(frames_on_root), count,
								static_cast<int>(state.screen_height), static_cast<int>(state.screen_width),
								state.shard.count > 1 ? state.shard.band_rows : static_cast<int>(state.screen_height), root, nullptr));
}

// Streams that run side by side (bm_probe_streams): for a host that pipelines frames over two streams with the exchange on a third.
// The HIP stream handles come back as void*; the caller releases them with bm_release_streams (or hipStreamDestroy).
inline std::vector<void*> probe_streams(int device, int count) {
	std::vector<void*> streams(static_cast<size_t>(count), nullptr);
	BM_CHECKED(bm_probe_streams(device, count, streams.data()));
	return streams;
}

// The reference's own schedule.  RayQueue* queue / queue2 and ShadowQueue* shadowQueue of the reference signature
// (state.h:19-21) and the statics / __device__ globals of kernel.cu:106-119,369 live in a Wavefront object; one call
// advances every path in flight by one segment, exactly like the reference's launch_kernels, and the buffer swap of
// main.cpp:146 happens inside.  `ray_queue_buffer_size` is variables.h:61.
struct Wavefront {
	bm_wavefront* handle = nullptr;
	explicit Wavefront(Scene::GPUScene gpuScene, uint32_t ray_queue_buffer_size = 2 * 1048576) {
		BM_CHECKED(bm_wavefront_create(gpuScene.handle, ray_queue_buffer_size, &handle));
	}
	~Wavefront() { bm_wavefront_destroy(handle); }
	Wavefront(const Wavefront&) = delete;
	Wavefront& operator=(const Wavefront&) = delete;
};

inline int launch_kernels(State& state, vec4* blit_buffer, Scene::GPUScene gpuScene, Wavefront& queues, int max_bounces = 3) {
	static Camera last;
	static bool first_time = true;
	bool reset_buffer = !first_time && detail::camera_changed(last); // kernel.cu:387
	first_time = false;
	if (sun_position_changed) { // kernel.cu:389-395
		sun_position_changed = false;
		reset_buffer = true;
	}
	if (reset_buffer) { // kernel.cu:397-403
		BM_CHECKED(bm_buffer_zero(state.device, blit_buffer, state.screen_width * state.screen_height * sizeof(vec4), nullptr));
		BM_CHECKED(bm_wavefront_reset(queues.handle));
	}
	const bm_camera cam = detail::camera_to_c();
	const bm_frame_params fp = detail::frame_params(state, max_bounces);
	BM_CHECKED(bm_wavefront_frame(queues.handle, &cam, &fp, reinterpret_cast<float*>(blit_buffer), nullptr));
	BM_CHECKED(bm_synchronize(gpuScene.handle)); // kernel.cu:431
	last = camera;
	return 0;
}

} // namespace brickmap
