// capi.cpp -- extern "C" surface of libbrickmap_hip.so (declared in include/brickmap.h).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include <new>

#include "camera_rays.h"
#include "denoise.h"
#include "kernels.h"
#include "distance.h"
#include "foot.h"
#include "mesh.h"
#include "reproject.h"
#include "scene.h"
#include "settle.h"
#include "travel.h"
#include "voxelize.h"
#include "water.h"
#include "wavefront.h"

struct bm_scene {
	bm::Scene impl;
	explicit bm_scene(int device) : impl(device) {}
};

struct bm_wavefront {
	bm::Wavefront impl;
	bm_wavefront(bm::Scene* scene, uint32_t queue_size) : impl(scene, queue_size) {}
};

using bm::set_error;

static_assert(sizeof(bm_ray) == 32 && sizeof(bm_ray_hit) == 32, "the query kernel reads and writes 32-byte records");

#define BM_NEED(scene)                                   \
	do {                                                 \
		if (!(scene)) {                                  \
			set_error("null scene handle");              \
			return BM_EINVAL;                            \
		}                                                \
	} while (0)

extern "C" {

const char* bm_last_error_string(void) { return bm::last_error(); }

int bm_device_count(int* count) {
	if (!count) { set_error("null argument"); return BM_EINVAL; }
	BM_HIP(hipGetDeviceCount(count));
	return 0;
}

int bm_device_name(int device, char* buf, size_t buflen, int* compute_units) {
	hipDeviceProp_t prop;
	BM_HIP(hipGetDeviceProperties(&prop, device));
	if (buf && buflen) {
		std::strncpy(buf, prop.gcnArchName, buflen - 1);
		buf[buflen - 1] = 0;
	}
	if (compute_units) *compute_units = prop.multiProcessorCount; // main.cpp:97 sm_cores
	return 0;
}

int bm_scene_create(int device, int grid_size, int grid_height, bm_scene** out) {
	if (!out) { set_error("null argument"); return BM_EINVAL; }
	*out = nullptr;
	bm_scene* s = new (std::nothrow) bm_scene(device);
	if (!s) { set_error("out of host memory"); return BM_EINVAL; }
	if (int e = s->impl.init(grid_size, grid_height)) {
		delete s;
		return e;
	}
	*out = s;
	return 0;
}

void bm_scene_destroy(bm_scene* scene) { delete scene; }

int bm_scene_set_lod(bm_scene* scene, int lod8, int lod2) { BM_NEED(scene); return scene->impl.set_lod(lod8, lod2); }
int bm_scene_set_queue_capacity(bm_scene* scene, int capacity) { BM_NEED(scene); return scene->impl.set_queue_capacity(capacity); }
int bm_scene_set_streaming_mode(bm_scene* scene, int overlapped) { BM_NEED(scene); return scene->impl.set_streaming_mode(overlapped); }
int bm_scene_generate(bm_scene* scene, int threads) { BM_NEED(scene); return scene->impl.generate(threads); }
int bm_scene_generate_supercell(bm_scene* scene, int sx, int sy, int sz) { BM_NEED(scene); return scene->impl.generate_supercell(sx, sy, sz); }
int bm_scene_preload_all(bm_scene* scene) { BM_NEED(scene); return scene->impl.preload_all(); }
int bm_scene_reset_residency(bm_scene* scene) { BM_NEED(scene); return scene->impl.reset_residency(); }
int bm_scene_process_load_queue(bm_scene* scene, uint32_t* serviced) { BM_NEED(scene); return scene->impl.process_load_queue(serviced); }
int bm_scene_dump(bm_scene* scene, const char* path) { BM_NEED(scene); return scene->impl.dump(path); }
int bm_scene_get_info(bm_scene* scene, bm_scene_info* info) { BM_NEED(scene); return scene->impl.info(info); }

int bm_scene_host_supercell(bm_scene* scene, int supercell, uint32_t* indices4096, uint32_t* brick_count, uint32_t* bricks, uint32_t brick_capacity) {
	BM_NEED(scene);
	bm::World& w = scene->impl.world;
	if (supercell < 0 || supercell >= static_cast<int>(w.supercells.size())) { set_error("bad supercell (or world not generated)"); return BM_EINVAL; }
	const bm::HostSupercell& c = w.supercells[supercell];
	if (c.indices.size() != static_cast<size_t>(bm::kCellsPerSupercell)) { set_error("supercell not generated"); return BM_ESTATE; }
	if (indices4096) std::memcpy(indices4096, c.indices.data(), bm::kCellsPerSupercell * sizeof(uint32_t));
	if (brick_count) *brick_count = static_cast<uint32_t>(c.bricks.size());
	if (bricks) {
		const size_t n = c.bricks.size() < brick_capacity ? c.bricks.size() : brick_capacity;
		std::memcpy(bricks, c.bricks.data(), n * sizeof(bm::Brick));
	}
	return 0;
}

int bm_scene_device_indices(bm_scene* scene, int supercell, uint32_t* indices4096) { BM_NEED(scene); return scene->impl.device_indices(supercell, indices4096); }

int bm_scene_device_brick(bm_scene* scene, int supercell, uint32_t device_slot, uint32_t* out16) { BM_NEED(scene); return scene->impl.device_brick(supercell, device_slot, out16); }

int bm_scene_edit(bm_scene* scene, int count, const bm_edit* edits, void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.edit(count, edits, static_cast<hipStream_t>(hip_stream));
}

int bm_scene_set_voxels(bm_scene* scene, int n, const int32_t* xyz, const uint8_t* values, void* hip_stream) {
	BM_NEED(scene);
	if (n < 0 || (n > 0 && (!xyz || !values))) { set_error("bm_scene_set_voxels: bad count or null argument"); return BM_EINVAL; }
	std::vector<bm_edit> edits;
	edits.reserve(static_cast<size_t>(n));
	for (int i = 0; i < n; ++i) {
		const int32_t* v = xyz + 3 * static_cast<size_t>(i);
		if (v[0] < 0 || v[1] < 0 || v[2] < 0 || v[0] == INT32_MAX || v[1] == INT32_MAX || v[2] == INT32_MAX) continue; // outside the world: a no-op
		bm_edit e{};
		e.op = values[i] ? BM_EDIT_SET : BM_EDIT_CLEAR;
		e.shape = BM_EDIT_BOX;
		for (int k = 0; k < 3; ++k) { e.lo[k] = v[k]; e.hi[k] = v[k] + 1; }
		edits.push_back(e);
	}
	return scene->impl.edit(static_cast<int>(edits.size()), edits.data(), static_cast<hipStream_t>(hip_stream));
}

// the readbacks of the walk fields (walk_fields.h) need the world on the device; the build statistics do not
#define BM_FIELDS(scene, f)                                         \
	BM_NEED(scene);                                                 \
	bm::WalkFields* const f = (scene)->impl.fields_on_device();     \
	if (!f) return BM_ESTATE
int bm_scene_device_cube_field(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes) { BM_FIELDS(scene, f); return f->device_cube_field(dst, capacity, bytes); }
int bm_scene_host_cube_field(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes) { BM_NEED(scene); return scene->impl.host_cube_field(dst, capacity, bytes); }
int bm_scene_escape_table(bm_scene* scene, int32_t* dst, size_t capacity, size_t* count) { BM_FIELDS(scene, f); return f->escape_table(dst, capacity, count); }
int bm_scene_sun_plane(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes, int32_t* plan12) { BM_FIELDS(scene, f); return f->sun_plane(dst, capacity, bytes, plan12); }
int bm_scene_shadow_heights(bm_scene* scene, uint32_t* dst, size_t capacity, size_t* count, uint64_t* bytes, int32_t* plan4) { BM_FIELDS(scene, f); return f->shadow_heights(dst, capacity, count, bytes, plan4); }
int bm_scene_sun_plane_stats(bm_scene* scene, uint64_t* builds, float* last_build_ms) { BM_NEED(scene); return scene->impl.fields().sun_plane_stats(builds, last_build_ms); }
int bm_scene_view_plane(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes, float* origin3) { BM_FIELDS(scene, f); return f->view_plane(dst, capacity, bytes, origin3); }
int bm_scene_view_plane_stats(bm_scene* scene, uint64_t* builds, float* last_build_ms) { BM_NEED(scene); return scene->impl.fields().view_plane_stats(builds, last_build_ms); }
int bm_scene_last_edit_ms(bm_scene* scene, float* scatter_ms, float* field_ms) { BM_NEED(scene); return scene->impl.last_edit_ms(scatter_ms, field_ms); }

int bm_scene_load_voxels(bm_scene* scene, const uint8_t* voxels, size_t bytes, int where, void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.load_voxels(voxels, bytes, where, static_cast<hipStream_t>(hip_stream));
}
int bm_scene_host_voxels(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes) { BM_NEED(scene); return scene->impl.host_voxels(dst, capacity, bytes); }
int bm_scene_last_load_ms(bm_scene* scene, float* pack_ms, float* field_ms, float* mirror_ms) { BM_NEED(scene); return scene->impl.last_load_ms(pack_ms, field_ms, mirror_ms); }

int bm_scene_write_region(bm_scene* scene, const bm_region* region, int op, const uint8_t* voxels, int where, void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.write_region(region, op, voxels, where, static_cast<hipStream_t>(hip_stream));
}
int bm_scene_read_region(bm_scene* scene, const bm_region* region, uint8_t* voxels, int where, void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.read_region(region, voxels, where, static_cast<hipStream_t>(hip_stream));
}
int bm_scene_last_region_ms(bm_scene* scene, float* pack_ms, float* copy_ms, float* scatter_ms, float* field_ms) {
	BM_NEED(scene);
	return scene->impl.last_region_ms(pack_ms, copy_ms, scatter_ms, field_ms);
}

int bm_scene_cast_rays(bm_scene* scene, int64_t n, const bm_ray* rays_dev, bm_ray_hit* hits_dev, uint32_t flags, const float lod_origin[3], void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.cast_rays(n, rays_dev, hits_dev, flags, lod_origin, static_cast<hipStream_t>(hip_stream));
}

int bm_scene_query_volumes(bm_scene* scene, int64_t n, const bm_volume* volumes_dev, bm_volume_result* results_dev, uint32_t flags, void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.query_volumes(n, volumes_dev, results_dev, flags, static_cast<hipStream_t>(hip_stream));
}

// (bm_host_label_volume is csrc/label_host.cpp: host code that needs nothing of the library)
int bm_scene_label_region(bm_scene* scene, const int32_t lo[3], const int32_t hi[3], uint32_t flags, int32_t* labels_dev, uint64_t* count_dev, void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.label_region(lo, hi, flags, labels_dev, count_dev, static_cast<hipStream_t>(hip_stream));
}
int bm_scene_label_components(bm_scene* scene, const int32_t lo[3], const int32_t hi[3], const int32_t* labels_dev, bm_component* comps_dev, int64_t capacity,
							  void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.label_components(lo, hi, labels_dev, comps_dev, capacity, static_cast<hipStream_t>(hip_stream));
}
int bm_scene_label_mask(bm_scene* scene, const int32_t lo[3], const int32_t hi[3], const int32_t* labels_dev, const bm_component* comps_dev, int64_t n,
						const uint8_t* chosen_dev, uint8_t* mask_dev, void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.label_mask(lo, hi, labels_dev, comps_dev, n, chosen_dev, mask_dev, static_cast<hipStream_t>(hip_stream));
}
int bm_scene_last_label_ms(bm_scene* scene, float* local_ms, float* merge_ms, float* flatten_ms) { BM_NEED(scene); return scene->impl.last_label_ms(local_ms, merge_ms, flatten_ms); }

int bm_camera_pixel_rays(const bm_camera* camera, int width, int height, int64_t n, const float* px, const float* py, bm_ray* out) {
	if (!camera || width <= 0 || height <= 0 || width > 65535 || height > 65535 || n < 0 || (n > 0 && (!px || !py || !out))) {
		set_error("bm_camera_pixel_rays: bad argument");
		return BM_EINVAL;
	}
	// the camera basis of the frames (fill_frame_constants, this translation unit is built with -ffp-contract=off like it)
	bm_frame_params p{};
	p.width = width; p.height = height; p.spp = 1; p.band_rows = height; p.shard_count = 1;
	bm::FrameConstants fc;
	if (int e = bm::fill_frame_constants(camera, &p, &fc)) return e;
	const float W = static_cast<float>(width), H = static_cast<float>(height);
	for (int64_t i = 0; i < n; ++i) {
		bm_ray& r = out[i];
		bm::pixel_ray_direction(fc.dir, fc.right, fc.up, W, H, px[i], py[i], r.direction); // (csrc/camera_rays.h: the rule, written once)
		for (int k = 0; k < 3; ++k) r.origin[k] = fc.origin[k];
		r.tmax = std::numeric_limits<float>::infinity();
		r.reserved = 0;
	}
	return 0;
}

int bm_camera_pixel_rays_device(bm_scene* scene, const bm_camera* camera, int width, int height, bm_ray* rays_dev, void* hip_stream) {
	BM_NEED(scene);
	return bm::pixel_rays(scene->impl.gpu(), camera, width, height, rays_dev, static_cast<hipStream_t>(hip_stream));
}

// (bm_host_denoise is csrc/denoise_host.cpp: host code that needs nothing of the library)
int bm_denoise_workspace_bytes(int width, int height, size_t* bytes) {
	if (!bytes || width < 1 || height < 1 || width > 65535 || height > 65535) { set_error("bm_denoise_workspace_bytes: bad argument"); return BM_EINVAL; }
	*bytes = bm::denoise_workspace_bytes(width, height);
	return 0;
}

int bm_denoise(bm_scene* scene, const bm_denoise_params* params, const float* accum_dev, const bm_ray_hit* hits_dev, float* out_dev, void* workspace_dev,
			   size_t workspace_bytes, void* hip_stream) {
	BM_NEED(scene);
	return bm::denoise(scene->impl.gpu(), params, accum_dev, hits_dev, out_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream));
}

int bm_debug_denoise_times(bm_scene* scene, const bm_denoise_params* params, const float* accum_dev, const bm_ray_hit* hits_dev, float* out_dev,
						   void* workspace_dev, size_t workspace_bytes, void* hip_stream, float* kernel_ms) {
	BM_NEED(scene);
	if (!kernel_ms) { set_error("bm_debug_denoise_times: null argument"); return BM_EINVAL; }
	return bm::denoise(scene->impl.gpu(), params, accum_dev, hits_dev, out_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream), kernel_ms);
}

// (bm_host_voxelize is csrc/voxelize_host.cpp: host code that needs nothing of the library)
int bm_voxelize_workspace_bytes(const bm_voxelize_params* params, int64_t n, size_t* bytes) {
	if (!params || !bytes) { set_error("bm_voxelize_workspace_bytes: null argument"); return BM_EINVAL; }
	const bm::VxParamsView pv = bm::voxelize_params_view(*params);
	if (const char* why = bm::voxelize_params_problem(pv, n)) { set_error(std::string("bm_voxelize_workspace_bytes: ") + why); return BM_EINVAL; }
	*bytes = bm::voxelize_workspace_bytes(bm::voxelize_dims(pv), static_cast<uint32_t>(n));
	return 0;
}

int bm_voxelize(bm_scene* scene, const bm_voxelize_params* params, int64_t n, const float* triangles_dev, uint8_t* volume_dev, bm_voxelize_result* result_dev,
				void* workspace_dev, size_t workspace_bytes, void* hip_stream) {
	BM_NEED(scene);
	return bm::voxelize(scene->impl.gpu(), params, n, triangles_dev, volume_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream));
}

int bm_debug_voxelize_times(bm_scene* scene, const bm_voxelize_params* params, int64_t n, const float* triangles_dev, uint8_t* volume_dev,
							bm_voxelize_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream, float* kernel_ms) {
	BM_NEED(scene);
	if (!kernel_ms) { set_error("bm_debug_voxelize_times: null argument"); return BM_EINVAL; }
	return bm::voxelize(scene->impl.gpu(), params, n, triangles_dev, volume_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream), kernel_ms);
}

// (bm_host_mesh_quads and bm_host_mesh_triangles are csrc/mesh_host.cpp: host code that needs nothing of the library)
int bm_mesh_workspace_bytes(const bm_mesh_params* params, size_t* bytes) {
	if (!params || !bytes) { set_error("bm_mesh_workspace_bytes: null argument"); return BM_EINVAL; }
	const bm::MeshParamsView pv = bm::mesh_params_view(*params);
	if (const char* why = bm::mesh_params_problem(pv)) { set_error(std::string("bm_mesh_workspace_bytes: ") + why); return BM_EINVAL; }
	*bytes = bm::mesh_workspace_bytes(bm::mesh_dims(pv));
	return 0;
}

int bm_mesh_quads(bm_scene* scene, const bm_mesh_params* params, const uint8_t* volume_dev, bm_quad* quads_dev, uint64_t capacity, bm_mesh_result* result_dev,
				  void* workspace_dev, size_t workspace_bytes, void* hip_stream) {
	BM_NEED(scene);
	return bm::mesh_quads(scene->impl.gpu(), params, volume_dev, quads_dev, capacity, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream));
}

int bm_debug_mesh_times(bm_scene* scene, const bm_mesh_params* params, const uint8_t* volume_dev, bm_quad* quads_dev, uint64_t capacity, bm_mesh_result* result_dev,
						void* workspace_dev, size_t workspace_bytes, void* hip_stream, float* kernel_ms) {
	BM_NEED(scene);
	if (!kernel_ms) { set_error("bm_debug_mesh_times: null argument"); return BM_EINVAL; }
	return bm::mesh_quads(scene->impl.gpu(), params, volume_dev, quads_dev, capacity, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream), kernel_ms);
}

int bm_mesh_triangles(bm_scene* scene, const bm_quad* quads_dev, int64_t n, float* triangles_dev, void* hip_stream) {
	BM_NEED(scene);
	return bm::mesh_triangles(scene->impl.gpu(), quads_dev, n, triangles_dev, static_cast<hipStream_t>(hip_stream));
}

// (bm_host_distance_field and bm_host_distance_mask are csrc/distance_host.cpp: host code that needs nothing of the library)
int bm_distance_workspace_bytes(const bm_distance_params* params, size_t* bytes) {
	if (!params || !bytes) { set_error("bm_distance_workspace_bytes: null argument"); return BM_EINVAL; }
	const bm::DistanceParamsView pv = bm::distance_params_view(*params);
	if (const char* why = bm::distance_params_problem(pv)) { set_error(std::string("bm_distance_workspace_bytes: ") + why); return BM_EINVAL; }
	*bytes = bm::distance_workspace_bytes(bm::distance_dims(pv));
	return 0;
}

int bm_distance_field(bm_scene* scene, const bm_distance_params* params, const uint8_t* volume_dev, uint32_t* dist_dev, bm_distance_result* result_dev, void* workspace_dev,
					  size_t workspace_bytes, void* hip_stream) {
	BM_NEED(scene);
	return bm::distance_field(scene->impl.gpu(), params, volume_dev, dist_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream));
}

int bm_debug_distance_times(bm_scene* scene, const bm_distance_params* params, const uint8_t* volume_dev, uint32_t* dist_dev, bm_distance_result* result_dev,
							void* workspace_dev, size_t workspace_bytes, void* hip_stream, float* kernel_ms) {
	BM_NEED(scene);
	if (!kernel_ms) { set_error("bm_debug_distance_times: null argument"); return BM_EINVAL; }
	return bm::distance_field(scene->impl.gpu(), params, volume_dev, dist_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream), kernel_ms);
}

int bm_distance_mask(bm_scene* scene, uint64_t count, const uint32_t* dist_dev, uint32_t limit_sq, uint32_t flags, uint8_t* volume_out_dev, void* hip_stream) {
	BM_NEED(scene);
	return bm::distance_mask(scene->impl.gpu(), count, dist_dev, limit_sq, flags, volume_out_dev, static_cast<hipStream_t>(hip_stream));
}

// (bm_host_travel_field and bm_host_travel_paths are csrc/travel_host.cpp: host code that needs nothing of the library)
int bm_travel_workspace_bytes(const bm_travel_params* params, size_t* bytes) {
	if (!params || !bytes) { set_error("bm_travel_workspace_bytes: null argument"); return BM_EINVAL; }
	const bm::TravelParamsView pv = bm::travel_params_view(*params);
	if (const char* why = bm::travel_params_problem(pv)) { set_error(std::string("bm_travel_workspace_bytes: ") + why); return BM_EINVAL; }
	*bytes = bm::travel_workspace_bytes(bm::travel_dims(pv));
	return 0;
}

int bm_travel_field(bm_scene* scene, const bm_travel_params* params, const uint8_t* volume_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev,
					bm_travel_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream) {
	BM_NEED(scene);
	return bm::travel_field(scene->impl.gpu(), params, volume_dev, seeds_dev, n, field_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream));
}

int bm_debug_travel_times(bm_scene* scene, const bm_travel_params* params, const uint8_t* volume_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev,
						  bm_travel_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream, uint32_t batch, float* stage_ms, uint32_t* counts) {
	BM_NEED(scene);
	if (!stage_ms || !counts) { set_error("bm_debug_travel_times: null argument"); return BM_EINVAL; }
	return bm::travel_field(scene->impl.gpu(), params, volume_dev, seeds_dev, n, field_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream), batch,
							stage_ms, counts);
}

int bm_travel_paths(bm_scene* scene, const int32_t extent[3], const uint32_t* field_dev, const int32_t* starts_dev, int64_t n, int32_t capacity, int32_t* path_dev,
					int32_t* lengths_dev, void* hip_stream) {
	BM_NEED(scene);
	return bm::travel_paths(scene->impl.gpu(), extent, field_dev, starts_dev, n, capacity, path_dev, lengths_dev, static_cast<hipStream_t>(hip_stream));
}

// (bm_host_settle is csrc/settle_host.cpp: host code that needs nothing of the library)
int bm_settle_workspace_bytes(const int32_t extent[3], int64_t n, size_t* bytes) {
	if (!extent || !bytes) { set_error("bm_settle_workspace_bytes: null argument"); return BM_EINVAL; }
	if (const char* why = bm::settle_extent_problem(extent)) { set_error(std::string("bm_settle_workspace_bytes: ") + why); return BM_EINVAL; }
	if (n < 0 || n > bm::kSettleMaxVoxels) { set_error("bm_settle_workspace_bytes: a negative number of records, or more than 2^31 - 2"); return BM_EINVAL; }
	*bytes = bm::settle_workspace_bytes(bm::settle_dims(extent, n));
	return 0;
}

int bm_settle(bm_scene* scene, const int32_t extent[3], const int32_t* labels_dev, const bm_component* comps_dev, int64_t n, const uint8_t* chosen_dev, uint8_t* out_dev,
			  int32_t* drops_dev, bm_settle_result* result_dev, void* workspace_dev, size_t workspace_bytes, uint32_t flags, void* hip_stream) {
	BM_NEED(scene);
	return bm::settle(scene->impl.gpu(), extent, labels_dev, comps_dev, n, chosen_dev, out_dev, drops_dev, result_dev, workspace_dev, workspace_bytes, flags,
					  static_cast<hipStream_t>(hip_stream));
}

int bm_debug_settle_times(bm_scene* scene, const int32_t extent[3], const int32_t* labels_dev, const bm_component* comps_dev, int64_t n, const uint8_t* chosen_dev,
						  uint8_t* out_dev, int32_t* drops_dev, bm_settle_result* result_dev, void* workspace_dev, size_t workspace_bytes, uint32_t flags, void* hip_stream,
						  uint32_t batch, float* stage_ms, uint32_t* counts) {
	BM_NEED(scene);
	if (!stage_ms || !counts) { set_error("bm_debug_settle_times: null argument"); return BM_EINVAL; }
	return bm::settle(scene->impl.gpu(), extent, labels_dev, comps_dev, n, chosen_dev, out_dev, drops_dev, result_dev, workspace_dev, workspace_bytes, flags,
					  static_cast<hipStream_t>(hip_stream), batch, stage_ms, counts);
}

// (bm_host_foot_room, bm_host_foot_field and bm_host_foot_paths are csrc/foot_host.cpp: host code that needs nothing of the library)
int bm_foot_workspace_bytes(const bm_foot_params* params, size_t* bytes) {
	if (!params || !bytes) { set_error("bm_foot_workspace_bytes: null argument"); return BM_EINVAL; }
	const bm::FootParamsView pv = bm::foot_params_view(*params);
	if (const char* why = bm::foot_params_problem(pv)) { set_error(std::string("bm_foot_workspace_bytes: ") + why); return BM_EINVAL; }
	*bytes = bm::foot_workspace_bytes(bm::foot_dims(pv));
	return 0;
}

int bm_foot_room(bm_scene* scene, const bm_foot_params* params, const uint8_t* volume_dev, uint8_t* room_dev, void* hip_stream) {
	BM_NEED(scene);
	return bm::foot_room(scene->impl.gpu(), params, volume_dev, room_dev, static_cast<hipStream_t>(hip_stream));
}

int bm_foot_field(bm_scene* scene, const bm_foot_params* params, const uint8_t* room_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev, bm_foot_result* result_dev,
				  void* workspace_dev, size_t workspace_bytes, void* hip_stream) {
	BM_NEED(scene);
	return bm::foot_field(scene->impl.gpu(), params, room_dev, seeds_dev, n, field_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream));
}

int bm_debug_foot_times(bm_scene* scene, const bm_foot_params* params, const uint8_t* room_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev,
						bm_foot_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream, uint32_t batch, float* stage_ms, uint32_t* counts) {
	BM_NEED(scene);
	if (!stage_ms || !counts) { set_error("bm_debug_foot_times: null argument"); return BM_EINVAL; }
	return bm::foot_field(scene->impl.gpu(), params, room_dev, seeds_dev, n, field_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream), batch,
						  stage_ms, counts);
}

int bm_foot_paths(bm_scene* scene, const bm_foot_params* params, const uint8_t* room_dev, const uint32_t* field_dev, const int32_t* starts_dev, int64_t n, int32_t capacity,
				  int32_t* path_dev, int32_t* lengths_dev, void* hip_stream) {
	BM_NEED(scene);
	return bm::foot_paths(scene->impl.gpu(), params, room_dev, field_dev, starts_dev, n, capacity, path_dev, lengths_dev, static_cast<hipStream_t>(hip_stream));
}

// (bm_host_water_field and bm_host_water_mask are csrc/water_host.cpp: host code that needs nothing of the library)
int bm_water_workspace_bytes(const bm_water_params* params, size_t* bytes) {
	if (!params || !bytes) { set_error("bm_water_workspace_bytes: null argument"); return BM_EINVAL; }
	const bm::TravelParamsView pv = bm::water_params_view(*params);
	if (const char* why = bm::water_params_problem(pv)) { set_error(std::string("bm_water_workspace_bytes: ") + why); return BM_EINVAL; }
	*bytes = bm::travel_workspace_bytes(bm::water_dims(pv));
	return 0;
}

int bm_water_field(bm_scene* scene, const bm_water_params* params, const uint8_t* volume_dev, const int32_t* drains_dev, int64_t n, uint32_t* field_dev,
				   bm_water_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream) {
	BM_NEED(scene);
	return bm::water_field(scene->impl.gpu(), params, volume_dev, drains_dev, n, field_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream));
}

int bm_debug_water_times(bm_scene* scene, const bm_water_params* params, const uint8_t* volume_dev, const int32_t* drains_dev, int64_t n, uint32_t* field_dev,
						 bm_water_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream, uint32_t batch, float* stage_ms, uint32_t* counts) {
	BM_NEED(scene);
	if (!stage_ms || !counts) { set_error("bm_debug_water_times: null argument"); return BM_EINVAL; }
	return bm::water_field(scene->impl.gpu(), params, volume_dev, drains_dev, n, field_dev, result_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(hip_stream), batch,
						   stage_ms, counts);
}

int bm_water_mask(bm_scene* scene, const int32_t extent[3], const uint32_t* field_dev, uint32_t min_depth, uint8_t* mask_dev, void* hip_stream) {
	BM_NEED(scene);
	return bm::water_mask(scene->impl.gpu(), extent, field_dev, min_depth, mask_dev, static_cast<hipStream_t>(hip_stream));
}

// (bm_host_reproject is csrc/reproject_host.cpp: host code that needs nothing of the library)
int bm_history_bytes(int width, int height, size_t* bytes) {
	if (!bytes || width < 1 || height < 1 || width > 65535 || height > 65535) { set_error("bm_history_bytes: bad argument"); return BM_EINVAL; }
	*bytes = bm::history_bytes(width, height);
	return 0;
}

int bm_reproject(bm_scene* scene, const bm_reproject_params* params, const bm_camera* camera, const bm_camera* camera_prev, const float* accum_dev,
				 const bm_ray_hit* hits_dev, const void* history_prev_dev, void* history_out_dev, void* hip_stream) {
	BM_NEED(scene);
	return bm::reproject(scene->impl.gpu(), params, camera, camera_prev, accum_dev, hits_dev, history_prev_dev, history_out_dev, static_cast<hipStream_t>(hip_stream));
}

int bm_scene_column_heights(bm_scene* scene, int sx, int sy, float* heights) {
	BM_NEED(scene);
	const bm::WorldDims& d = scene->impl.world.dims;
	if (!heights || sx < 0 || sy < 0 || sx >= d.supergrid_xy || sy >= d.supergrid_xy) { set_error("bad column"); return BM_EINVAL; }
	scene->impl.world.column_heights(sx, sy, heights);
	return 0;
}

int bm_host_column_heights(int grid_size, int grid_height, int sx, int sy, float* heights) {
	bm::World w;
	if (!heights || !w.dims.set(grid_size, grid_height) || sx < 0 || sy < 0 || sx >= w.dims.supergrid_xy || sy >= w.dims.supergrid_xy) {
		set_error("bad world dimensions or column");
		return BM_EINVAL;
	}
	w.column_heights(sx, sy, heights);
	return 0;
}

int bm_host_generate_supercell(int grid_size, int grid_height, int sx, int sy, int sz, uint32_t* indices4096, uint32_t* brick_count,
							   uint32_t* bricks, uint32_t brick_capacity) {
	bm::World w;
	if (!w.dims.set(grid_size, grid_height) || sx < 0 || sy < 0 || sz < 0 || sx >= w.dims.supergrid_xy || sy >= w.dims.supergrid_xy ||
		sz >= w.dims.supergrid_z) {
		set_error("bad world dimensions or supercell");
		return BM_EINVAL;
	}
	w.generate_supercell(sx, sy, sz);
	const bm::HostSupercell& c = w.supercells[w.dims.supercell_id(sx, sy, sz)];
	if (indices4096) std::memcpy(indices4096, c.indices.data(), bm::kCellsPerSupercell * sizeof(uint32_t));
	if (brick_count) *brick_count = static_cast<uint32_t>(c.bricks.size());
	if (bricks) {
		const size_t n = c.bricks.size() < brick_capacity ? c.bricks.size() : brick_capacity;
		std::memcpy(bricks, c.bricks.data(), n * sizeof(bm::Brick));
	}
	return 0;
}

} // extern "C"

namespace {
// the supercell arrays of the host doors below -> a HostSupercell (slots no word names are free; the lowest is reused first), and back
int import_supercell(const uint32_t* indices4096, const uint32_t* brick_count, const uint32_t* bricks, uint32_t brick_capacity, bm::HostSupercell* c) {
	if (!indices4096 || !brick_count || (!bricks && *brick_count > 0) || *brick_count > 4096u || *brick_count > brick_capacity) {
		set_error("bad supercell arrays");
		return BM_EINVAL;
	}
	c->indices.assign(indices4096, indices4096 + bm::kCellsPerSupercell);
	c->bricks.resize(*brick_count);
	if (*brick_count) std::memcpy(c->bricks.data(), bricks, *brick_count * sizeof(bm::Brick));
	std::vector<uint8_t> used(*brick_count, 0);
	for (uint32_t word : c->indices) {
		if (!word) continue;
		if (!(word & BM_BRICK_LOADED_BIT) || (word & BM_BRICK_INDEX_BITS) >= *brick_count) { set_error("an index word names no brick"); return BM_EINVAL; }
		used[word & BM_BRICK_INDEX_BITS] = 1;
	}
	for (uint32_t s = *brick_count; s-- > 0;)
		if (!used[s]) c->free_slots.push_back(s);
	return 0;
}
int export_supercell(const bm::HostSupercell& c, uint32_t* indices4096, uint32_t* brick_count, uint32_t* bricks, uint32_t brick_capacity) {
	if (c.bricks.size() > brick_capacity) { set_error("brick buffer too small for the edited supercell"); return BM_EINVAL; }
	std::memcpy(indices4096, c.indices.data(), bm::kCellsPerSupercell * sizeof(uint32_t));
	if (!c.bricks.empty()) std::memcpy(bricks, c.bricks.data(), c.bricks.size() * sizeof(bm::Brick));
	*brick_count = static_cast<uint32_t>(c.bricks.size());
	return 0;
}
bool supercell_in_world(bm::WorldDims* dims, int grid_size, int grid_height, int sx, int sy, int sz) {
	if (dims->set(grid_size, grid_height) && sx >= 0 && sy >= 0 && sz >= 0 && sx < dims->supergrid_xy && sy < dims->supergrid_xy && sz < dims->supergrid_z) return true;
	set_error("bad world dimensions or supercell");
	return false;
}
} // namespace

extern "C" {

int bm_host_edit_supercell(int grid_size, int grid_height, int sx, int sy, int sz, uint32_t* indices4096, uint32_t* brick_count,
						   uint32_t* bricks, uint32_t brick_capacity, int count, const bm_edit* edits) {
	bm::WorldDims dims;
	if (!supercell_in_world(&dims, grid_size, grid_height, sx, sy, sz)) return BM_EINVAL;
	bm::HostSupercell c;
	if (int e = import_supercell(indices4096, brick_count, bricks, brick_capacity, &c)) return e;
	std::string why;
	if (!bm::World::validate_edits(edits, count, &why)) { set_error("bm_host_edit_supercell: " + why); return BM_EINVAL; }
	bm::World::edit_supercell(dims, c, sx, sy, sz, edits, count, nullptr);
	return export_supercell(c, indices4096, brick_count, bricks, brick_capacity);
}

int bm_host_write_region_supercell(int grid_size, int grid_height, int sx, int sy, int sz, uint32_t* indices4096, uint32_t* brick_count,
								   uint32_t* bricks, uint32_t brick_capacity, const bm_region* region, int op, const uint8_t* voxels) {
	bm::WorldDims dims;
	if (!supercell_in_world(&dims, grid_size, grid_height, sx, sy, sz)) return BM_EINVAL;
	bm::HostSupercell c;
	if (int e = import_supercell(indices4096, brick_count, bricks, brick_capacity, &c)) return e;
	if (!region || !voxels) { set_error("bm_host_write_region_supercell: null region or volume"); return BM_EINVAL; }
	if (op != BM_REGION_REPLACE && op != BM_EDIT_SET && op != BM_EDIT_CLEAR) { set_error("bm_host_write_region_supercell: unknown op"); return BM_EINVAL; }
	bm_region r = *region;
	std::string why;
	uint64_t span = 0;
	if (!bm::World::validate_region(&r, &why, &span)) { set_error("bm_host_write_region_supercell: " + why); return BM_EINVAL; }
	int lo[3], hi[3];
	if (!bm::World::region_bounds(dims, r, lo, hi)) return 0;
	bm::World::RegionSource src;
	src.voxels = voxels;
	src.row_pitch = r.row_pitch;
	src.slice_pitch = r.slice_pitch;
	for (int k = 0; k < 3; ++k) src.origin[k] = r.lo[k];
	bm::World::write_region_supercell(dims, c, sx, sy, sz, lo, hi, op, src, nullptr);
	return export_supercell(c, indices4096, brick_count, bricks, brick_capacity);
}

int bm_host_load_supercell(int grid_size, int grid_height, int sx, int sy, int sz, const uint8_t* voxels, uint32_t* indices4096, uint32_t* bricks,
						   uint32_t* brick_count) {
	bm::WorldDims dims;
	if (!dims.set(grid_size, grid_height) || sx < 0 || sy < 0 || sz < 0 || sx >= dims.supergrid_xy || sy >= dims.supergrid_xy || sz >= dims.supergrid_z) {
		set_error("bad world dimensions or supercell");
		return BM_EINVAL;
	}
	if (!voxels || !indices4096 || !bricks || !brick_count) { set_error("null argument"); return BM_EINVAL; }
	bm::HostSupercell c;
	bm::World::load_supercell(dims, c, sx, sy, sz, voxels);
	std::memcpy(indices4096, c.indices.data(), bm::kCellsPerSupercell * sizeof(uint32_t));
	if (!c.bricks.empty()) std::memcpy(bricks, c.bricks.data(), c.bricks.size() * sizeof(bm::Brick));
	*brick_count = static_cast<uint32_t>(c.bricks.size());
	return 0;
}

int bm_debug_division_magic(uint32_t divisor, uint32_t* magic, int* shift) {
	if (!magic || !shift || divisor < 3u || divisor >= (1u << 23)) { bm::set_error("bad argument"); return BM_EINVAL; }
	bm::division_magic(divisor, magic, shift);
	return 0;
}

int bm_host_cube_field(int grid_size, int grid_height, uint8_t* field, size_t capacity, size_t* bytes) {
	bm::World w;
	if (!w.dims.set(grid_size, grid_height)) { set_error("bad world dimensions"); return BM_EINVAL; }
	const size_t need = 8ull * (w.dims.cells + 2) * (w.dims.cells + 2) * (w.dims.cells_height + 2);
	if (bytes) *bytes = need;
	if (!field) return 0;
	if (capacity < need) { set_error("cube field buffer too small"); return BM_EINVAL; }
	w.generate(8);
	std::vector<uint8_t> f;
	w.build_cube_field(f, 8);
	std::memcpy(field, f.data(), need);
	return 0;
}

int bm_buffer_alloc(int device, size_t bytes, void** dev_ptr) {
	if (!dev_ptr) { set_error("null argument"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device));
	BM_HIP(hipMalloc(dev_ptr, bytes ? bytes : 4));
	return 0;
}
int bm_buffer_free(int device, void* dev_ptr) {
	BM_HIP(hipSetDevice(device));
	BM_HIP(hipFree(dev_ptr));
	return 0;
}
int bm_buffer_zero(int device, void* dev_ptr, size_t bytes, void* hip_stream) {
	BM_HIP(hipSetDevice(device));
	BM_HIP(hipMemsetAsync(dev_ptr, 0, bytes, static_cast<hipStream_t>(hip_stream))); // launch_kernels:399
	return 0;
}
int bm_buffer_read(int device, void* host_dst, const void* dev_src, size_t bytes) {
	BM_HIP(hipSetDevice(device));
	BM_HIP(hipDeviceSynchronize());
	BM_HIP(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
	return 0;
}
int bm_buffer_write(int device, void* dev_dst, const void* host_src, size_t bytes) {
	BM_HIP(hipSetDevice(device));
	BM_HIP(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
	return 0;
}

int bm_local_rows(const bm_frame_params* p) {
	if (!p || p->band_rows <= 0 || p->shard_count <= 0 || p->height <= 0) return 0;
	// rows y with (y / band) % count == rank
	const int band = p->band_rows, count = p->shard_count, rank = p->shard_rank;
	const int full_bands = p->height / band, tail = p->height % band;
	int rows = 0;
	if (rank < full_bands) rows = ((full_bands - 1 - rank) / count + 1) * band;
	if (tail && full_bands % count == rank) rows += tail;
	return rows;
}

int bm_render_frame(bm_scene* scene, const bm_camera* camera, const bm_frame_params* params, float* accum_dev, uint32_t* debug_dev, void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.render(camera, params, accum_dev, debug_dev, static_cast<hipStream_t>(hip_stream));
}
int bm_render_frames(bm_scene* scene, int count, const bm_camera* cameras, const bm_frame_params* params, float* const* accum_dev, uint32_t* const* debug_dev,
					 void* hip_stream) {
	BM_NEED(scene);
	return scene->impl.render_frames(count, cameras, params, accum_dev, debug_dev, static_cast<hipStream_t>(hip_stream));
}
int bm_frame_plan_of(const bm_frame_params* params, int hit_records, bm_frame_plan* out) {
	if (!params || !out) { set_error("null argument"); return BM_EINVAL; }
	bm_camera cam{};
	cam.direction[0] = 1.f; cam.up[2] = 1.f; cam.focal_distance = 1.f; // (the plan does not depend on the view)
	bm::FrameConstants fc;
	if (int e = bm::fill_frame_constants(&cam, params, &fc, hit_records != 0)) return e;
	std::memset(out, 0, sizeof *out);
	out->flags = fc.flags;
	out->helpers = fc.helpers;
	out->sample_items = (fc.flags & BM_FLAG_SAMPLE_ITEMS) ? 1 : 0;
	out->ordered = (fc.helpers || out->sample_items) ? 0 : 1;
	out->xcd_handout = fc.xcd_handout;
	out->refill_min = fc.refill_min;
	out->refill_min_in_ring = bm::ring_refill_min(fc.refill_min, fc.helpers != 0, bm::tuning().refill_min);
	out->tiles_x = fc.tiles_x; out->tiles_y = fc.tiles_y; out->local_rows = fc.local_rows;
	out->instrumented = bm::instrumented_frame(fc.flags, hit_records != 0) ? 1 : 0;
	out->ring_group = bm::ring_group_of(fc, bm::kMaxRingGroup); // (of a launch long enough for a whole group)
	return 0;
}
int bm_launch_plan_of(int count, const bm_camera* cameras, const bm_frame_params* params, float* const* accum_dev, uint32_t* const* debug_dev, int grid_size,
					  int grid_height, bm_launch_plan* out) {
	if (!out) { set_error("null argument"); return BM_EINVAL; }
	std::memset(out, 0, sizeof *out); // (a refused plan reads all zero)
	bm::WorldDims dims;
	if (!dims.set(grid_size, grid_height)) { set_error("bad world dimensions"); return BM_EINVAL; }
	bm::LaunchPlan plan;
	if (int e = bm::plan_launch(count, cameras, params, accum_dev, debug_dev, dims.cells, dims.cells_height, &plan)) return e;
	const bm::FrameConstants& fc = plan.frames[0];
	out->ring_mode = plan.ring_mode;
	out->ring_group = fc.ring_group;
	out->sample_stride = fc.ring_sample_stride;
	out->pixel_stride = fc.ring_pixel_stride;
	out->shared_digest = plan.shared_digest ? 1 : 0;
	out->instrumented = plan.instrumented ? 1 : 0;
	out->counter_blocks = plan.counter_blocks;
	out->refill_min = fc.refill_min;
	out->workgroups = plan.workgroups;
	return 0;
}
int bm_trace_waves_per_simd(int device, int instrumented, int xcd_handout, int helpers, int* waves) {
	if (!waves) { set_error("null argument"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device));
	// a 256-thread workgroup is one wave on each of a compute unit's four SIMDs: resident workgroups per CU = waves per SIMD
	*waves = bm::trace_blocks_per_cu(instrumented != 0, xcd_handout != 0, helpers != 0);
	if (bm::tuning().blocks_per_cu > 0 && !instrumented && *waves > bm::tuning().blocks_per_cu) *waves = bm::tuning().blocks_per_cu;
	return 0;
}
int bm_tuning_overrides(char* buf, size_t buflen) {
	if (!buf || buflen == 0) { set_error("null argument"); return BM_EINVAL; }
	const bm::Tuning& t = bm::tuning();
	std::string s;
	auto add = [&s](const char* name, int v) { if (!s.empty()) s += ' '; s += name; s += '='; s += std::to_string(v); };
	if (t.refill_min >= 1 && t.refill_min <= 64) add("BM_REFILL_MIN", t.refill_min);
	if (t.xcd_handout == 0 || t.xcd_handout == 1) add("BM_XCD_HANDOUT", t.xcd_handout);
	if (t.helpers == 0 || t.helpers == 1) add("BM_HELPERS", t.helpers);
	if (t.blocks_per_cu > 0) add("BM_TRACE_BLOCKS_PER_CU", t.blocks_per_cu);
	if (t.ring_group >= 1 && t.ring_group <= bm::kMaxRingGroup) add("BM_RING_GROUP", t.ring_group);
	if (s.size() + 1 > buflen) { set_error("buffer too small"); return BM_EINVAL; }
	std::memcpy(buf, s.c_str(), s.size() + 1);
	return 0;
}
int bm_resolve(bm_scene* scene, const float* accum_dev, float* out_dev, int64_t n_pixels, void* hip_stream) {
	BM_NEED(scene);
	return bm::resolve(scene->impl.gpu(), accum_dev, out_dev, n_pixels, static_cast<hipStream_t>(hip_stream));
}
int bm_synchronize(bm_scene* scene) { BM_NEED(scene); return scene->impl.synchronize(); }
int bm_last_render_ms(bm_scene* scene, float* ms) { BM_NEED(scene); return scene->impl.last_render_ms(ms); }
int bm_render_times(bm_scene* scene, float* ms, int capacity, int* count) { BM_NEED(scene); return scene->impl.render_times(ms, capacity, count); }
int bm_counters_read(bm_scene* scene, bm_counters* out) { BM_NEED(scene); return scene->impl.counters_read(out); }
int bm_counters_reset(bm_scene* scene) { BM_NEED(scene); return scene->impl.counters_reset(); }
int bm_sched_stats_read(bm_scene* scene, bm_sched_stats* out) { BM_NEED(scene); return scene->impl.sched_stats_read(out); }
int bm_sched_detail_read(bm_scene* scene, uint64_t* out8) { BM_NEED(scene); return scene->impl.sched_detail_read(out8); }

int bm_wavefront_create(bm_scene* scene, uint32_t queue_size, bm_wavefront** out) {
	BM_NEED(scene);
	if (!out) { set_error("null argument"); return BM_EINVAL; }
	*out = nullptr;
	bm_wavefront* w = new (std::nothrow) bm_wavefront(&scene->impl, queue_size);
	if (!w) { set_error("out of host memory"); return BM_EINVAL; }
	if (int e = w->impl.init()) {
		delete w;
		return e;
	}
	*out = w;
	return 0;
}
void bm_wavefront_destroy(bm_wavefront* wf) { delete wf; }
#define BM_NEED_WF(wf)                                   \
	do {                                                 \
		if (!(wf)) {                                     \
			set_error("null wavefront handle");          \
			return BM_EINVAL;                            \
		}                                                \
	} while (0)
int bm_wavefront_reset(bm_wavefront* wf) { BM_NEED_WF(wf); return wf->impl.reset(); }
int bm_wavefront_frame(bm_wavefront* wf, const bm_camera* camera, const bm_frame_params* params, float* accum_dev, void* hip_stream) {
	BM_NEED_WF(wf);
	if (!camera || !params) { set_error("null argument"); return BM_EINVAL; }
	return wf->impl.frame(camera, params, accum_dev, static_cast<hipStream_t>(hip_stream));
}
int bm_wavefront_stats(bm_wavefront* wf, uint32_t* out6) { BM_NEED_WF(wf); return wf->impl.stats(out6); }
int bm_wavefront_read_queue(bm_wavefront* wf, int which, uint32_t first, uint32_t count, void* host_out) {
	BM_NEED_WF(wf);
	return wf->impl.read_queue(which, first, count, host_out);
}
int bm_wavefront_times(bm_wavefront* wf, float* ms5) { BM_NEED_WF(wf); return wf->impl.times(ms5); }
int bm_wavefront_counters_read(bm_wavefront* wf, int which, bm_counters* out) { BM_NEED_WF(wf); return wf->impl.counters_read(which, out); }
int bm_wavefront_sched_stats_read(bm_wavefront* wf, int which, uint64_t* out6) {
	BM_NEED_WF(wf);
	return wf->impl.sched_stats_read(which, reinterpret_cast<unsigned long long*>(out6));
}
int bm_wavefront_counters_reset(bm_wavefront* wf) { BM_NEED_WF(wf); return wf->impl.counters_reset(); }

int bm_debug_sincos(int device, int n, const float* x_host, float* sin_host, float* cos_host) {
	if (n <= 0 || !x_host || !sin_host || !cos_host) { set_error("bad argument"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device));
	float *dx = nullptr, *ds = nullptr, *dc = nullptr;
	const size_t bytes = static_cast<size_t>(n) * sizeof(float);
	BM_HIP(hipMalloc(reinterpret_cast<void**>(&dx), bytes));
	BM_HIP(hipMalloc(reinterpret_cast<void**>(&ds), bytes));
	BM_HIP(hipMalloc(reinterpret_cast<void**>(&dc), bytes));
	BM_HIP(hipMemcpy(dx, x_host, bytes, hipMemcpyHostToDevice));
	bm::launch_debug_sincos(n, dx, ds, dc, nullptr);
	BM_HIP(hipGetLastError());
	BM_HIP(hipDeviceSynchronize());
	BM_HIP(hipMemcpy(sin_host, ds, bytes, hipMemcpyDeviceToHost));
	BM_HIP(hipMemcpy(cos_host, dc, bytes, hipMemcpyDeviceToHost));
	(void)hipFree(dx); (void)hipFree(ds); (void)hipFree(dc);
	return 0;
}

int bm_debug_sky(int device, const float sun_position[2], int n, const float* viewdirs_host, float* sun_host, float* sky_host, float* sunsky_host) {
	if (n <= 0 || !sun_position || !viewdirs_host || !sun_host || !sky_host || !sunsky_host) { set_error("bad argument"); return BM_EINVAL; }
	bm_camera cam{};
	cam.direction[0] = 1.f; cam.up[2] = 1.f; cam.focal_distance = 1.f;
	bm_frame_params fp{};
	fp.width = 16; fp.height = 16; fp.spp = 1; fp.max_bounces = 3; fp.base_frame = 1; fp.band_rows = 16; fp.shard_count = 1;
	fp.sun_position[0] = sun_position[0]; fp.sun_position[1] = sun_position[1];
	bm::FrameConstants fc;
	if (int e = bm::fill_frame_constants(&cam, &fp, &fc)) return e;
	BM_HIP(hipSetDevice(device));
	const size_t bytes = static_cast<size_t>(n) * 3 * sizeof(float);
	float* d[4] = {nullptr, nullptr, nullptr, nullptr};
	for (auto& p : d) BM_HIP(hipMalloc(reinterpret_cast<void**>(&p), bytes));
	BM_HIP(hipMemcpy(d[0], viewdirs_host, bytes, hipMemcpyHostToDevice));
	bm::launch_debug_sky(fc, n, d[0], d[1], d[2], d[3], nullptr);
	BM_HIP(hipGetLastError());
	BM_HIP(hipDeviceSynchronize());
	BM_HIP(hipMemcpy(sun_host, d[1], bytes, hipMemcpyDeviceToHost));
	BM_HIP(hipMemcpy(sky_host, d[2], bytes, hipMemcpyDeviceToHost));
	BM_HIP(hipMemcpy(sunsky_host, d[3], bytes, hipMemcpyDeviceToHost));
	for (auto& p : d) (void)hipFree(p);
	return 0;
}

} // extern "C"
