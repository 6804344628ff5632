// device_ops.h -- the device operators that keep no state: kernels on the caller's stream over the caller's buffers, which read nothing
// of a scene's world.  A scene only names the GPU they run on (Scene::gpu()); calls on different streams are independent.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/brickmap.h"

namespace bm {

struct Gpu {
	int device;
	int compute_units;
};

// [p, p + bytes) lies inside one allocation of `device` (which is current)
bool device_span_ok(int device, const void* p, size_t bytes);

int resolve(const Gpu& gpu, const float* accum, float* out, long long n, hipStream_t stream);
// the a-trous filter (denoise.hip): the workspace is the caller's
// kernel_ms: null, or 2 + iterations durations -- prepare, moments, every pass (the call then waits; bm_debug_denoise_times)
int denoise(const Gpu& gpu, const bm_denoise_params* params, const float* accum, const bm_ray_hit* hits, float* out, void* workspace, size_t workspace_bytes,
			hipStream_t stream, float* kernel_ms = nullptr);
// meshes -> voxels (voxelize.hip): like the filter, the buffers and the workspace are the caller's
// kernel_ms: null, or 5 durations -- zeroing, plan + scan, surface, solid, the dense pass (the call then waits; bm_debug_voxelize_times)
int voxelize(const Gpu& gpu, const bm_voxelize_params* params, int64_t n, const float* triangles, uint8_t* volume, bm_voxelize_result* result, void* workspace,
			 size_t workspace_bytes, hipStream_t stream, float* kernel_ms = nullptr);
// voxels -> quads (mesh.hip): like voxelize, the buffers and the workspace are the caller's
// kernel_ms: null, or 3 durations -- count, scan, emit (the call then waits; bm_debug_mesh_times)
int mesh_quads(const Gpu& gpu, const bm_mesh_params* params, const uint8_t* volume, bm_quad* quads, uint64_t capacity, bm_mesh_result* result, void* workspace,
			   size_t workspace_bytes, hipStream_t stream, float* kernel_ms = nullptr);
int mesh_triangles(const Gpu& gpu, const bm_quad* quads, int64_t n, float* triangles, hipStream_t stream);
// voxels -> their squared distance to the nearest source (distance.hip): like mesh_quads, the buffers and the workspace are the caller's
// kernel_ms: null, or 3 durations -- the x pass, the y pass, the z pass + finish (the call then waits; bm_debug_distance_times)
int distance_field(const Gpu& gpu, const bm_distance_params* params, const uint8_t* volume, uint32_t* dist, bm_distance_result* result, void* workspace,
				   size_t workspace_bytes, hipStream_t stream, float* kernel_ms = nullptr);
int distance_mask(const Gpu& gpu, uint64_t count, const uint32_t* dist, uint32_t limit_sq, uint32_t flags, uint8_t* volume_out, hipStream_t stream);
// voxels + seeds -> shortest face-step distances (travel.hip): the buffers and the workspace are the caller's.  Unlike its siblings the
// call returns when the field stands: it waits on `stream` between batches of `batch` rounds (0 = kTravelBatch).  stage_ms: null, or 3
// durations -- set-up, rounds, finish; counts: null, or the rounds enqueued and the looks of the host (bm_debug_travel_times)
int travel_field(const Gpu& gpu, const bm_travel_params* params, const uint8_t* volume, const int32_t* seeds, int64_t n, uint32_t* field, bm_travel_result* result,
				 void* workspace, size_t workspace_bytes, hipStream_t stream, uint32_t batch = 0, float* stage_ms = nullptr, uint32_t* counts = nullptr);
int travel_paths(const Gpu& gpu, const int32_t extent[3], const uint32_t* field, const int32_t* starts, int64_t n, int32_t capacity, int32_t* path, int32_t* lengths,
				 hipStream_t stream);
// labels + chosen records -> the settled volume, the drops and the record (settle.hip): the buffers and the workspace are the caller's.
// Like travel_field the call returns when the result stands: it waits on `stream` between batches of `batch` rounds (0 = kSettleBatch).
// stage_ms: null, or 3 durations -- set-up, rounds, move + finish; counts: null, or the rounds enqueued and the looks of the host
// (bm_debug_settle_times)
int settle(const Gpu& gpu, const int32_t extent[3], const int32_t* labels, const bm_component* comps, int64_t n, const uint8_t* chosen, uint8_t* out, int32_t* drops,
		   bm_settle_result* result, void* workspace, size_t workspace_bytes, uint32_t flags, hipStream_t stream, uint32_t batch = 0, float* stage_ms = nullptr,
		   uint32_t* counts = nullptr);
// ground navigation (foot.hip): a byte volume -> room bytes; room bytes + seeds -> the walk field and the record; a field -> paths.  The
// buffers and the workspace are the caller's.  foot_room and foot_paths are asynchronous; like travel_field, foot_field returns when the
// field stands: it waits on `stream` between batches of `batch` rounds (0 = kFootBatch).  stage_ms: null, or 3 durations -- set-up,
// rounds, finish; counts: null, or the rounds enqueued and the looks of the host (bm_debug_foot_times)
int foot_room(const Gpu& gpu, const bm_foot_params* params, const uint8_t* volume, uint8_t* room, hipStream_t stream);
int foot_field(const Gpu& gpu, const bm_foot_params* params, const uint8_t* room, const int32_t* seeds, int64_t n, uint32_t* field, bm_foot_result* result, void* workspace,
			   size_t workspace_bytes, hipStream_t stream, uint32_t batch = 0, float* stage_ms = nullptr, uint32_t* counts = nullptr);
int foot_paths(const Gpu& gpu, const bm_foot_params* params, const uint8_t* room, const uint32_t* field, const int32_t* starts, int64_t n, int32_t capacity, int32_t* path,
			   int32_t* lengths, hipStream_t stream);
// spill levels and pools (water.hip): a byte volume + drains -> the field and the record; a field -> the mask.  The buffers and the
// workspace are the caller's.  Like travel_field, water_field returns when the field stands: it waits on `stream` between batches of
// `batch` rounds (0 = kTravelBatch); water_mask is asynchronous.  stage_ms: null, or 3 durations -- set-up, rounds, finish; counts: null,
// or the rounds enqueued, the looks of the host and the tile visits (bm_debug_water_times)
int water_field(const Gpu& gpu, const bm_water_params* params, const uint8_t* volume, const int32_t* drains, int64_t n, uint32_t* field, bm_water_result* result,
				void* workspace, size_t workspace_bytes, hipStream_t stream, uint32_t batch = 0, float* stage_ms = nullptr, uint32_t* counts = nullptr);
int water_mask(const Gpu& gpu, const int32_t extent[3], const uint32_t* field, uint32_t min_depth, uint8_t* mask, hipStream_t stream);
// pixel-centre rays of a frame, written on the device (denoise.hip)
int pixel_rays(const Gpu& gpu, const bm_camera* cam, int width, int height, bm_ray* rays, hipStream_t stream);
// temporal accumulation (reproject.hip): one kernel on the caller's stream over the caller's buffers
int reproject(const Gpu& gpu, const bm_reproject_params* params, const bm_camera* cam, const bm_camera* cam_prev, const float* accum, const bm_ray_hit* hits,
			  const void* history_prev, void* history_out, hipStream_t stream);

} // namespace bm
