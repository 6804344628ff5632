// device_ops.cpp -- the stateless device operators (device_ops.h): what each refuses about its parameters and the caller's buffers, then its launch.
#include "device_ops.h"

#include <cstdlib>
#include <string>

#include "buffer_checks.h"
#include "camera_rays.h"
#include "denoise.h"
#include "distance.h"
#include "error.h"
#include "foot.h"
#include "hip_owned.h"
#include "kernels.h"
#include "mesh.h"
#include "settle.h"
#include "travel.h"
#include "voxelize.h"
#include "water.h"

namespace bm {

bool device_span_ok(int device, const void* p, size_t bytes) {
	hipPointerAttribute_t attr{};
	void* base = nullptr;
	size_t size = 0;
	if (hipPointerGetAttributes(&attr, p) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != device ||
		hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &size, const_cast<void*>(p)) != hipSuccess ||
		static_cast<const uint8_t*>(base) + size < static_cast<const uint8_t*>(p) + bytes) {
		(void)hipGetLastError();
		return false;
	}
	return true;
}

int resolve(const Gpu& gpu, const float* accum, float* out, long long n, hipStream_t stream) {
	if (!accum || !out || n < 0) { set_error("bad argument"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(gpu.device));
	launch_resolve(accum, out, n, stream);
	BM_HIP(hipGetLastError());
	return 0;
}

// ---- the a-trous filter (bm_denoise): image passes on the caller's stream over the caller's buffers; nothing of the world is read
int denoise(const Gpu& gpu, const bm_denoise_params* params, const float* accum, const bm_ray_hit* hits, float* out, void* workspace, size_t workspace_bytes,
			hipStream_t stream, float* kernel_ms) {
	if (!params || !accum || !hits || !out || !workspace) { set_error("bm_denoise: null argument"); return BM_EINVAL; }
	const DenoiseParamsView pv = {params->width, params->height, params->iterations, params->sigma_l, params->flags, params->reserved};
	if (const char* why = denoise_params_problem(pv)) { set_error(std::string("bm_denoise: ") + why); return BM_EINVAL; }
	const size_t need = denoise_workspace_bytes(params->width, params->height);
	if (workspace_bytes < need) { set_error("bm_denoise: the workspace is smaller than bm_denoise_workspace_bytes"); return BM_EINVAL; }
	if (!all_aligned(16, accum, hits, out, workspace)) { set_error("bm_denoise: buffers must be 16-byte aligned"); return BM_EINVAL; }
	const size_t image = need / 36 * 16;
	const Span ws = span_of(workspace, need);
	if (spans_overlap(span_of(accum, image), ws) || spans_overlap(span_of(out, image), ws) || spans_overlap(span_of(hits, 2 * image), ws)) {
		set_error("bm_denoise: the workspace overlaps an image");
		return BM_EINVAL;
	}
	BM_HIP(hipSetDevice(gpu.device));
	static const int tiled_max_step = [] { // experiment knob: the largest a-trous stride that stages its taps in LDS (0, 1, 2)
		const char* e = std::getenv("BM_DENOISE_TILED_MAX");
		return e && *e ? std::atoi(e) : kDenoiseTiledMaxStep;
	}();
	// without a pass there is one kernel; the 2 + iterations durations the caller reads are defined all the same
	const int stages = params->iterations == 0 ? 1 : 2 + params->iterations;
	if (kernel_ms)
		for (int i = 0; i < 2 + params->iterations; ++i) kernel_ms[i] = 0.f;
	return launch_staged<3 + kDenoiseMaxIterations>(stages, kernel_ms, [&](hipEvent_t* marks) {
		launch_denoise(params->width, params->height, params->iterations, params->sigma_l, accum, hits, out, workspace, tiled_max_step, stream, marks);
	});
}

// ---- meshes -> voxels (bm_voxelize): kernels on the caller's stream over the caller's buffers; nothing of the world is read
int voxelize(const Gpu& gpu, const bm_voxelize_params* params, int64_t n, const float* triangles, uint8_t* volume, bm_voxelize_result* result, void* workspace,
			 size_t workspace_bytes, hipStream_t stream, float* kernel_ms) {
	if (!params) { set_error("bm_voxelize: null params"); return BM_EINVAL; }
	const VxParamsView pv = voxelize_params_view(*params);
	if (const char* why = voxelize_params_problem(pv, n)) { set_error(std::string("bm_voxelize: ") + why); return BM_EINVAL; }
	if (!volume || !workspace || (n > 0 && !triangles)) { set_error("bm_voxelize: null buffer"); return BM_EINVAL; }
	const VoxelizeDims d = voxelize_dims(pv);
	const size_t need = voxelize_workspace_bytes(d, static_cast<uint32_t>(n));
	if (workspace_bytes < need) { set_error("bm_voxelize: the workspace is smaller than bm_voxelize_workspace_bytes"); return BM_EINVAL; }
	if (!aligned(triangles, 4) || !aligned(result, 8) || !aligned(workspace, 16)) {
		set_error("bm_voxelize: triangles must be 4-byte, the result 8-byte and the workspace 16-byte aligned");
		return BM_EINVAL;
	}
	const size_t span = static_cast<size_t>(pv.extent[2] - 1) * static_cast<size_t>(d.slice_pitch) + static_cast<size_t>(pv.extent[1] - 1) * static_cast<size_t>(d.row_pitch) +
						static_cast<size_t>(pv.extent[0]);
	const size_t tri_bytes = static_cast<size_t>(n) * 9 * sizeof(float);
	const Span ws = span_of(workspace, need);
	BM_HIP(hipSetDevice(gpu.device));
	// (a volume whose pitches carry it past its allocation has no extent to overlap anything with, see mesh_quads)
	if ((spans_overlap(span_of(volume, span), ws) && device_span_ok(gpu.device, volume, span)) || spans_overlap(span_of(triangles, tri_bytes), ws) ||
		(result && spans_overlap(span_of(result, sizeof(bm_voxelize_result)), ws))) {
		set_error("bm_voxelize: the workspace overlaps the volume, the triangles or the result");
		return BM_EINVAL;
	}
	if (!device_span_ok(gpu.device, volume, span) || !device_span_ok(gpu.device, workspace, need) || (n > 0 && !device_span_ok(gpu.device, triangles, tri_bytes)) ||
		(result && !device_span_ok(gpu.device, result, sizeof(bm_voxelize_result)))) {
		set_error("bm_voxelize: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	static const int per_cu[2] = {voxelize_blocks_per_cu(false), voxelize_blocks_per_cu(true)};
	const int resident[2] = {per_cu[0] * gpu.compute_units, per_cu[1] * gpu.compute_units};
	return launch_staged<6>(5, kernel_ms, [&](hipEvent_t* marks) {
		launch_voxelize(d, triangles, static_cast<uint32_t>(n), volume, result, workspace, resident, stream, marks);
	});
}

// ---- voxels -> quads (bm_mesh_quads, bm_mesh_triangles): kernels on the caller's stream over the caller's buffers; nothing of the world is read
int mesh_quads(const Gpu& gpu, const bm_mesh_params* params, const uint8_t* volume, bm_quad* quads, uint64_t capacity, bm_mesh_result* result, void* workspace,
			   size_t workspace_bytes, hipStream_t stream, float* kernel_ms) {
	if (!params) { set_error("bm_mesh_quads: null params"); return BM_EINVAL; }
	const MeshParamsView pv = mesh_params_view(*params);
	if (const char* why = mesh_params_problem(pv)) { set_error(std::string("bm_mesh_quads: ") + why); return BM_EINVAL; }
	if (!volume || !result || !workspace) { set_error("bm_mesh_quads: null volume, result or workspace"); return BM_EINVAL; }
	if (!quads && capacity > 0) { set_error("bm_mesh_quads: null quads with a capacity above 0"); return BM_EINVAL; }
	if (capacity > (uint64_t{1} << 40)) { set_error("bm_mesh_quads: a capacity above 2^40"); return BM_EINVAL; }
	const MeshDims d = mesh_dims(pv);
	const size_t need = mesh_workspace_bytes(d);
	if (workspace_bytes < need) { set_error("bm_mesh_quads: the workspace is smaller than bm_mesh_workspace_bytes"); return BM_EINVAL; }
	if (!aligned(quads, 4) || !aligned(result, 8) || !aligned(workspace, 16)) {
		set_error("bm_mesh_quads: quads must be 4-byte, the result 8-byte and the workspace 16-byte aligned");
		return BM_EINVAL;
	}
	const size_t span = static_cast<size_t>(mesh_span(d));
	const size_t quad_bytes = quads ? static_cast<size_t>(capacity) * sizeof(bm_quad) : 0;
	const Span ws = span_of(workspace, need);
	BM_HIP(hipSetDevice(gpu.device));
	// (a volume whose pitches carry it past its allocation has no extent to overlap anything with: whether that phantom extent crosses the
	// workspace depends on where the allocator put the two, and the refusal must not)
	if ((spans_overlap(span_of(volume, span), ws) && device_span_ok(gpu.device, volume, span)) || spans_overlap(span_of(quads, quad_bytes), ws) ||
		spans_overlap(span_of(result, sizeof(bm_mesh_result)), ws)) {
		set_error("bm_mesh_quads: the workspace overlaps the volume, the quads or the result");
		return BM_EINVAL;
	}
	if (!device_span_ok(gpu.device, volume, span) || !device_span_ok(gpu.device, workspace, need) || (quad_bytes > 0 && !device_span_ok(gpu.device, quads, quad_bytes)) ||
		!device_span_ok(gpu.device, result, sizeof(bm_mesh_result))) {
		set_error("bm_mesh_quads: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	return launch_staged<4>(3, kernel_ms, [&](hipEvent_t* marks) { launch_mesh_quads(d, volume, quads, quads ? capacity : 0, result, workspace, stream, marks); });
}

int mesh_triangles(const Gpu& gpu, const bm_quad* quads, int64_t n, float* triangles, hipStream_t stream) {
	if (n < 0 || n > (int64_t{1} << 32)) { set_error("bm_mesh_triangles: a quad count below 0 or above 2^32"); return BM_EINVAL; }
	if (n == 0) return 0;
	if (!quads || !triangles) { set_error("bm_mesh_triangles: null buffer"); return BM_EINVAL; }
	if (!aligned(quads, 4) || !aligned(triangles, 4)) { set_error("bm_mesh_triangles: quads and triangles must be 4-byte aligned"); return BM_EINVAL; }
	const size_t quad_bytes = static_cast<size_t>(n) * sizeof(bm_quad), tri_bytes = static_cast<size_t>(n) * 18 * sizeof(float);
	if (spans_overlap(span_of(quads, quad_bytes), span_of(triangles, tri_bytes))) { set_error("bm_mesh_triangles: the triangles overlap the quads"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(gpu.device));
	if (!device_span_ok(gpu.device, quads, quad_bytes) || !device_span_ok(gpu.device, triangles, tri_bytes)) {
		set_error("bm_mesh_triangles: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	launch_mesh_triangles(quads, static_cast<uint64_t>(n), triangles, stream);
	BM_HIP(hipGetLastError());
	return 0;
}

// ---- voxels -> distances (bm_distance_field, bm_distance_mask): kernels on the caller's stream over the caller's buffers; nothing of the world is read
int distance_field(const Gpu& gpu, const bm_distance_params* params, const uint8_t* volume, uint32_t* dist, bm_distance_result* result, void* workspace,
				   size_t workspace_bytes, hipStream_t stream, float* kernel_ms) {
	if (!params) { set_error("bm_distance_field: null params"); return BM_EINVAL; }
	const DistanceParamsView pv = distance_params_view(*params);
	if (const char* why = distance_params_problem(pv)) { set_error(std::string("bm_distance_field: ") + why); return BM_EINVAL; }
	if (!volume || !dist || !result || !workspace) { set_error("bm_distance_field: null volume, field, result or workspace"); return BM_EINVAL; }
	const DistanceDims d = distance_dims(pv);
	const size_t need = distance_workspace_bytes(d);
	if (workspace_bytes < need) { set_error("bm_distance_field: the workspace is smaller than bm_distance_workspace_bytes"); return BM_EINVAL; }
	if (!aligned(dist, 4) || !aligned(result, 8) || !aligned(workspace, 16)) {
		set_error("bm_distance_field: the field must be 4-byte, the result 8-byte and the workspace 16-byte aligned");
		return BM_EINVAL;
	}
	const size_t span = static_cast<size_t>(distance_span(d)), field_bytes = static_cast<size_t>(d.voxels) * sizeof(uint32_t);
	const Span ws = span_of(workspace, need), field = span_of(dist, field_bytes);
	BM_HIP(hipSetDevice(gpu.device));
	// (a volume whose pitches carry it past its allocation has no extent to overlap anything with, see mesh_quads)
	const bool volume_ok = device_span_ok(gpu.device, volume, span);
	if ((volume_ok && spans_overlap(span_of(volume, span), ws)) || spans_overlap(field, ws) || spans_overlap(span_of(result, sizeof(bm_distance_result)), ws)) {
		set_error("bm_distance_field: the workspace overlaps the volume, the field or the result");
		return BM_EINVAL;
	}
	if ((volume_ok && spans_overlap(span_of(volume, span), field)) || spans_overlap(span_of(result, sizeof(bm_distance_result)), field)) {
		set_error("bm_distance_field: the field overlaps the volume or the result");
		return BM_EINVAL;
	}
	if (!volume_ok || !device_span_ok(gpu.device, workspace, need) || !device_span_ok(gpu.device, dist, field_bytes) ||
		!device_span_ok(gpu.device, result, sizeof(bm_distance_result))) {
		set_error("bm_distance_field: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	return launch_staged<4>(3, kernel_ms, [&](hipEvent_t* marks) { launch_distance_field(d, volume, dist, result, workspace, stream, marks); });
}

int distance_mask(const Gpu& gpu, uint64_t count, const uint32_t* dist, uint32_t limit_sq, uint32_t flags, uint8_t* volume_out, hipStream_t stream) {
	if (count == 0 || count > static_cast<uint64_t>(kDistanceMaxVoxels)) { set_error("bm_distance_mask: a count of 0 or above 2^31 - 2"); return BM_EINVAL; }
	if (flags & ~kDistanceMaskAbove) { set_error("bm_distance_mask: unknown flag"); return BM_EINVAL; }
	if (!dist || !volume_out) { set_error("bm_distance_mask: null buffer"); return BM_EINVAL; }
	if (!aligned(dist, 4)) { set_error("bm_distance_mask: the field must be 4-byte aligned"); return BM_EINVAL; }
	const size_t field_bytes = static_cast<size_t>(count) * sizeof(uint32_t);
	if (spans_overlap(span_of(dist, field_bytes), span_of(volume_out, static_cast<size_t>(count)))) { set_error("bm_distance_mask: the output overlaps the field"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(gpu.device));
	if (!device_span_ok(gpu.device, dist, field_bytes) || !device_span_ok(gpu.device, volume_out, static_cast<size_t>(count))) {
		set_error("bm_distance_mask: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	launch_distance_mask(dist, count, limit_sq, flags & kDistanceMaskAbove, volume_out, stream);
	BM_HIP(hipGetLastError());
	return 0;
}

// ---- voxels + seeds -> shortest face-step distances (bm_travel_field, bm_travel_paths): kernels on the caller's stream over the caller's
// buffers; nothing of the world is read.  The host loop of the rounds is here: batches of rounds, and between them one word read back.
int travel_field(const Gpu& gpu, const bm_travel_params* params, const uint8_t* volume, const int32_t* seeds, int64_t n, uint32_t* field, bm_travel_result* result,
				 void* workspace, size_t workspace_bytes, hipStream_t stream, uint32_t batch, float* stage_ms, uint32_t* counts) {
	if (!params) { set_error("bm_travel_field: null params"); return BM_EINVAL; }
	const TravelParamsView pv = travel_params_view(*params);
	if (const char* why = travel_params_problem(pv)) { set_error(std::string("bm_travel_field: ") + why); return BM_EINVAL; }
	if (n < 0 || n > 0x7FFFFFFF) { set_error("bm_travel_field: a negative number of seeds, or more than 2^31 - 1"); return BM_EINVAL; }
	if (!volume || !field || !result || !workspace || (n > 0 && !seeds)) { set_error("bm_travel_field: null volume, seeds, field, result or workspace"); return BM_EINVAL; }
	const TravelDims d = travel_dims(pv);
	const size_t need = travel_workspace_bytes(d);
	if (workspace_bytes < need) { set_error("bm_travel_field: the workspace is smaller than bm_travel_workspace_bytes"); return BM_EINVAL; }
	if (!aligned(field, 4) || !aligned(seeds, 4) || !aligned(result, 8) || !aligned(workspace, 16)) {
		set_error("bm_travel_field: the field and the seeds must be 4-byte, the result 8-byte and the workspace 16-byte aligned");
		return BM_EINVAL;
	}
	const size_t span = static_cast<size_t>(travel_span(d)), field_bytes = static_cast<size_t>(d.voxels) * sizeof(uint32_t), seed_bytes = static_cast<size_t>(n) * 12;
	const Span ws = span_of(workspace, need), fs = span_of(field, field_bytes), ss = span_of(seeds, seed_bytes), rs = span_of(result, sizeof(bm_travel_result));
	BM_HIP(hipSetDevice(gpu.device));
	// (a volume whose pitches carry it past its allocation has no extent to overlap anything with, see mesh_quads)
	const bool volume_ok = device_span_ok(gpu.device, volume, span);
	if ((volume_ok && spans_overlap(span_of(volume, span), ws)) || spans_overlap(fs, ws) || spans_overlap(ss, ws) || spans_overlap(rs, ws)) {
		set_error("bm_travel_field: the workspace overlaps the volume, the seeds, the field or the result");
		return BM_EINVAL;
	}
	if ((volume_ok && spans_overlap(span_of(volume, span), fs)) || spans_overlap(ss, fs) || spans_overlap(rs, fs)) {
		set_error("bm_travel_field: the field overlaps the volume, the seeds or the result");
		return BM_EINVAL;
	}
	if (!volume_ok || !device_span_ok(gpu.device, workspace, need) || !device_span_ok(gpu.device, field, field_bytes) || (n > 0 && !device_span_ok(gpu.device, seeds, seed_bytes)) ||
		!device_span_ok(gpu.device, result, sizeof(bm_travel_result))) {
		set_error("bm_travel_field: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	if (batch == 0) batch = kTravelBatch;
	StageMarks<4> marks;
	if (stage_ms) {
		if (int e = marks.create(4)) return e;
	}
	auto stamp = [&](int i) { if (stage_ms) (void)hipEventRecord(marks.marks()[i], stream); };
	stamp(0);
	launch_travel_setup(d, volume, seeds, static_cast<uint32_t>(n), field, workspace, stream);
	stamp(1);
	// Round k settles every voxel whose shortest path crosses at most k - 1 tile faces (travel.h), a path of s steps crosses at most s,
	// and no path is longer than the limit or has more steps than the volume has voxels: the list is empty after that many rounds + 2.
	const uint64_t cap = static_cast<uint64_t>(pv.max_steps != 0 && pv.max_steps < d.voxels ? pv.max_steps : d.voxels) + 2;
	const uint8_t* tail = static_cast<const uint8_t*>(workspace) + travel_tail_offset(d);
	uint64_t done = 0;
	uint32_t looks = 0, listed = n > 0 ? 1u : 0u; // (without seeds no list ever holds a tile)
	while (listed != 0) {
		if (done >= cap) { set_error("bm_travel_field: internal error: tiles are still listed after every round the field can need"); return BM_ESTATE; }
		const uint32_t rounds = static_cast<uint32_t>(cap - done < batch ? cap - done : batch);
		launch_travel_rounds(d, field, workspace, static_cast<uint32_t>(done) + 1u, rounds, stream);
		done += rounds;
		// the next list's count: what round done + 1 would read
		BM_HIP(hipMemcpyAsync(&listed, tail + 4 * (kTravelTailCountWord + (done + 1) % 3), 4, hipMemcpyDeviceToHost, stream));
		BM_HIP(hipStreamSynchronize(stream));
		++looks;
	}
	stamp(2);
	launch_travel_finish(d, field, result, workspace, stream);
	stamp(3);
	BM_HIP(hipGetLastError());
	BM_HIP(hipStreamSynchronize(stream)); // the call returns when the field and the record stand
	if (counts) {
		counts[0] = static_cast<uint32_t>(done);
		counts[1] = looks;
	}
	if (stage_ms) return marks.read(3, stage_ms);
	return 0;
}

int travel_paths(const Gpu& gpu, const int32_t extent[3], const uint32_t* field, const int32_t* starts, int64_t n, int32_t capacity, int32_t* path, int32_t* lengths,
				 hipStream_t stream) {
	if (!extent) { set_error("bm_travel_paths: null extent"); return BM_EINVAL; }
	if (const char* why = travel_extent_problem(extent)) { set_error(std::string("bm_travel_paths: ") + why); return BM_EINVAL; }
	if (n < 0 || n > 0x7FFFFFFF) { set_error("bm_travel_paths: a negative number of starts, or more than 2^31 - 1"); return BM_EINVAL; }
	if (capacity < 1) { set_error("bm_travel_paths: a capacity below 1"); return BM_EINVAL; }
	if (!field || (n > 0 && (!starts || !path || !lengths))) { set_error("bm_travel_paths: null field, starts, path or lengths"); return BM_EINVAL; }
	if (!all_aligned(4, field, starts, path, lengths)) { set_error("bm_travel_paths: the field, the starts, the path and the lengths must be 4-byte aligned"); return BM_EINVAL; }
	if (static_cast<uint64_t>(n) * static_cast<uint64_t>(capacity) > (uint64_t{1} << 40)) { set_error("bm_travel_paths: more than 2^40 path voxels"); return BM_EINVAL; }
	const TravelDims d = travel_field_dims(extent);
	const size_t field_bytes = static_cast<size_t>(d.voxels) * sizeof(uint32_t), start_bytes = static_cast<size_t>(n) * 12, path_bytes = start_bytes * static_cast<size_t>(capacity),
				 length_bytes = static_cast<size_t>(n) * 4;
	const Span fs = span_of(field, field_bytes), ss = span_of(starts, start_bytes), ps = span_of(path, path_bytes), ls = span_of(lengths, length_bytes);
	if (spans_overlap(ps, fs) || spans_overlap(ps, ss) || spans_overlap(ls, fs) || spans_overlap(ls, ss) || spans_overlap(ps, ls)) {
		set_error("bm_travel_paths: the path or the lengths buffer overlaps the field, the starts or the other of the two");
		return BM_EINVAL;
	}
	BM_HIP(hipSetDevice(gpu.device));
	if (!device_span_ok(gpu.device, field, field_bytes) ||
		(n > 0 && (!device_span_ok(gpu.device, starts, start_bytes) || !device_span_ok(gpu.device, path, path_bytes) || !device_span_ok(gpu.device, lengths, length_bytes)))) {
		set_error("bm_travel_paths: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	if (n == 0) return 0;
	launch_travel_paths(d, field, starts, static_cast<uint32_t>(n), capacity, path, lengths, stream);
	BM_HIP(hipGetLastError());
	return 0;
}

// ---- voxels + drains -> spill levels and pools (bm_water_field, bm_water_mask): kernels on the caller's stream over the caller's buffers;
// nothing of the world is read.  The refusals and the host loop of the rounds are those of travel_field.
int water_field(const Gpu& gpu, const bm_water_params* params, const uint8_t* volume, const int32_t* drains, int64_t n, uint32_t* field, bm_water_result* result,
				void* workspace, size_t workspace_bytes, hipStream_t stream, uint32_t batch, float* stage_ms, uint32_t* counts) {
	if (!params) { set_error("bm_water_field: null params"); return BM_EINVAL; }
	const TravelParamsView pv = water_params_view(*params);
	if (const char* why = water_params_problem(pv)) { set_error(std::string("bm_water_field: ") + why); return BM_EINVAL; }
	if (n < 0 || n > 0x7FFFFFFF) { set_error("bm_water_field: a negative number of drains, or more than 2^31 - 1"); return BM_EINVAL; }
	if (!volume || !field || !result || !workspace || (n > 0 && !drains)) { set_error("bm_water_field: null volume, drains, field, result or workspace"); return BM_EINVAL; }
	const TravelDims d = water_dims(pv);
	const size_t need = travel_workspace_bytes(d);
	if (workspace_bytes < need) { set_error("bm_water_field: the workspace is smaller than bm_water_workspace_bytes"); return BM_EINVAL; }
	if (!aligned(field, 4) || !aligned(drains, 4) || !aligned(result, 8) || !aligned(workspace, 16)) {
		set_error("bm_water_field: the field and the drains must be 4-byte, the result 8-byte and the workspace 16-byte aligned");
		return BM_EINVAL;
	}
	const size_t span = static_cast<size_t>(travel_span(d)), field_bytes = static_cast<size_t>(d.voxels) * sizeof(uint32_t), drain_bytes = static_cast<size_t>(n) * 12;
	const Span ws = span_of(workspace, need), fs = span_of(field, field_bytes), ss = span_of(drains, drain_bytes), rs = span_of(result, sizeof(bm_water_result));
	BM_HIP(hipSetDevice(gpu.device));
	// (a volume whose pitches carry it past its allocation has no extent to overlap anything with, see mesh_quads)
	const bool volume_ok = device_span_ok(gpu.device, volume, span);
	if ((volume_ok && spans_overlap(span_of(volume, span), ws)) || spans_overlap(fs, ws) || spans_overlap(ss, ws) || spans_overlap(rs, ws)) {
		set_error("bm_water_field: the workspace overlaps the volume, the drains, the field or the result");
		return BM_EINVAL;
	}
	if ((volume_ok && spans_overlap(span_of(volume, span), fs)) || spans_overlap(ss, fs) || spans_overlap(rs, fs)) {
		set_error("bm_water_field: the field overlaps the volume, the drains or the result");
		return BM_EINVAL;
	}
	if (!volume_ok || !device_span_ok(gpu.device, workspace, need) || !device_span_ok(gpu.device, field, field_bytes) || (n > 0 && !device_span_ok(gpu.device, drains, drain_bytes)) ||
		!device_span_ok(gpu.device, result, sizeof(bm_water_result))) {
		set_error("bm_water_field: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	if (batch == 0) batch = kTravelBatch;
	StageMarks<4> marks;
	if (stage_ms) {
		if (int e = marks.create(4)) return e;
	}
	auto stamp = [&](int i) { if (stage_ms) (void)hipEventRecord(marks.marks()[i], stream); };
	stamp(0);
	launch_water_setup(d, params->sea_level, params->flags & kWaterFaces, volume, drains, static_cast<uint32_t>(n), field, workspace, stream);
	stamp(1);
	// Round k settles every voxel whose best path crosses at most k - 1 tile faces (water.h), and a best path without a repeated voxel
	// crosses fewer faces than the volume has voxels: the list is empty after that many rounds + 2.
	const uint64_t cap = static_cast<uint64_t>(d.voxels) + 2;
	const uint8_t* tail = static_cast<const uint8_t*>(workspace) + travel_tail_offset(d);
	uint64_t done = 0;
	uint32_t looks = 0, listed = 0;
	// whether anything is an outlet is known on the device only: the first list's count, what round 1 would read
	BM_HIP(hipMemcpyAsync(&listed, tail + 4 * (kTravelTailCountWord + 1), 4, hipMemcpyDeviceToHost, stream));
	BM_HIP(hipStreamSynchronize(stream));
	++looks;
	while (listed != 0) {
		if (done >= cap) { set_error("bm_water_field: internal error: tiles are still listed after every round the field can need"); return BM_ESTATE; }
		const uint32_t rounds = static_cast<uint32_t>(cap - done < batch ? cap - done : batch);
		launch_water_rounds(d, field, workspace, static_cast<uint32_t>(done) + 1u, rounds, stream);
		done += rounds;
		// the next list's count: what round done + 1 would read
		BM_HIP(hipMemcpyAsync(&listed, tail + 4 * (kTravelTailCountWord + (done + 1) % 3), 4, hipMemcpyDeviceToHost, stream));
		BM_HIP(hipStreamSynchronize(stream));
		++looks;
	}
	stamp(2);
	launch_water_finish(d, field, result, workspace, stream);
	stamp(3);
	BM_HIP(hipGetLastError());
	if (counts) {
		counts[0] = static_cast<uint32_t>(done);
		counts[1] = looks;
		BM_HIP(hipMemcpyAsync(&counts[2], tail + 4 * kWaterTailVisitsWord, 4, hipMemcpyDeviceToHost, stream));
	}
	BM_HIP(hipStreamSynchronize(stream)); // the call returns when the field and the record stand
	if (stage_ms) return marks.read(3, stage_ms);
	return 0;
}

int water_mask(const Gpu& gpu, const int32_t extent[3], const uint32_t* field, uint32_t min_depth, uint8_t* mask, hipStream_t stream) {
	if (!extent) { set_error("bm_water_mask: null extent"); return BM_EINVAL; }
	if (const char* why = travel_extent_problem(extent)) { set_error(std::string("bm_water_mask: ") + why); return BM_EINVAL; }
	if (min_depth < 1) { set_error("bm_water_mask: a min_depth below 1"); return BM_EINVAL; }
	if (!field || !mask) { set_error("bm_water_mask: null field or mask"); return BM_EINVAL; }
	if (!aligned(field, 4)) { set_error("bm_water_mask: the field must be 4-byte aligned"); return BM_EINVAL; }
	const size_t voxels = static_cast<size_t>(extent[0]) * static_cast<size_t>(extent[1]) * static_cast<size_t>(extent[2]);
	if (spans_overlap(span_of(field, voxels * sizeof(uint32_t)), span_of(mask, voxels))) { set_error("bm_water_mask: the mask overlaps the field"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(gpu.device));
	if (!device_span_ok(gpu.device, field, voxels * sizeof(uint32_t)) || !device_span_ok(gpu.device, mask, voxels)) {
		set_error("bm_water_mask: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	launch_water_mask(extent, field, min_depth, mask, stream);
	BM_HIP(hipGetLastError());
	return 0;
}

// ---- labels + chosen records -> the settled volume (bm_settle): kernels on the caller's stream over the caller's buffers; nothing of the
// world is read.  The host loop of the rounds is here: batches of rounds, and between them one small copy read back.
int settle(const Gpu& gpu, const int32_t extent[3], const int32_t* labels, const bm_component* comps, int64_t n, const uint8_t* chosen, uint8_t* out, int32_t* drops,
		   bm_settle_result* result, void* workspace, size_t workspace_bytes, uint32_t flags, hipStream_t stream, uint32_t batch, float* stage_ms, uint32_t* counts) {
	if (!extent) { set_error("bm_settle: null extent"); return BM_EINVAL; }
	if (const char* why = settle_extent_problem(extent)) { set_error(std::string("bm_settle: ") + why); return BM_EINVAL; }
	if (flags != 0) { set_error("bm_settle: unknown flag"); return BM_EINVAL; }
	if (n < 0 || n > kSettleMaxVoxels) { set_error("bm_settle: a negative number of records, or more than 2^31 - 2"); return BM_EINVAL; }
	if (!labels || !out || !result || !workspace || (n > 0 && (!comps || !chosen || !drops))) {
		set_error("bm_settle: null labels, records, chosen, out, drops, result or workspace");
		return BM_EINVAL;
	}
	const SettleDims d = settle_dims(extent, n);
	const size_t need = settle_workspace_bytes(d);
	if (workspace_bytes < need) { set_error("bm_settle: the workspace is smaller than bm_settle_workspace_bytes"); return BM_EINVAL; }
	if (!aligned(labels, 4) || !aligned(workspace, 4) || !aligned(result, 8) || (n > 0 && (!aligned(drops, 4) || !aligned(comps, 8)))) {
		set_error("bm_settle: labels, drops and workspace must be 4-byte, the records and the result 8-byte aligned");
		return BM_EINVAL;
	}
	const size_t label_bytes = static_cast<size_t>(d.voxels) * 4, out_bytes = d.voxels, comp_bytes = static_cast<size_t>(n) * sizeof(bm_component),
				 chosen_bytes = static_cast<size_t>(n), drop_bytes = static_cast<size_t>(n) * 4;
	const Span ws = span_of(workspace, need), ls = span_of(labels, label_bytes), os = span_of(out, out_bytes), rs = span_of(result, sizeof(bm_settle_result));
	const Span cs = span_of(comps, comp_bytes), hs = span_of(chosen, chosen_bytes), ds = span_of(drops, drop_bytes);
	if (spans_overlap(os, ls)) { set_error("bm_settle: out overlaps labels"); return BM_EINVAL; }
	if (spans_overlap(ls, ws) || spans_overlap(os, ws) || spans_overlap(rs, ws) || (n > 0 && (spans_overlap(cs, ws) || spans_overlap(hs, ws) || spans_overlap(ds, ws)))) {
		set_error("bm_settle: the workspace overlaps labels, the records, chosen, out, the drops or the result");
		return BM_EINVAL;
	}
	BM_HIP(hipSetDevice(gpu.device));
	if (!device_span_ok(gpu.device, labels, label_bytes) || !device_span_ok(gpu.device, out, out_bytes) || !device_span_ok(gpu.device, result, sizeof(bm_settle_result)) ||
		!device_span_ok(gpu.device, workspace, need) ||
		(n > 0 && (!device_span_ok(gpu.device, comps, comp_bytes) || !device_span_ok(gpu.device, chosen, chosen_bytes) || !device_span_ok(gpu.device, drops, drop_bytes)))) {
		set_error("bm_settle: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	if (batch == 0) batch = kSettleBatch;
	StageMarks<4> marks;
	if (stage_ms) {
		if (int e = marks.create(4)) return e;
	}
	auto stamp = [&](int i) { if (stage_ms) (void)hipEventRecord(marks.marks()[i], stream); };
	stamp(0);
	launch_settle_setup(d, chosen, workspace, stream);
	stamp(1);
	// After round r every piece whose shortest chain has at most r contacts is final, a chain has at most as many contacts as there are
	// chosen records, and the round after the last change counts none: chosen + 1 rounds at most, and one to spare.  Until the first
	// look has brought the number of chosen records, n stands in for it.
	const uint8_t* tail = reinterpret_cast<const uint8_t*>(settle_tail_at(d, workspace));
	uint64_t done = 0, cap = static_cast<uint64_t>(n) + 2;
	uint32_t looks = 0, seen[4] = {0, 0, 0, 0}, changes = 1; // seen: the tail's three counts and `chosen`
	while (changes != 0) {
		if (done >= cap) { set_error("bm_settle: internal error: drops still fall after every round the pieces can need"); return BM_ESTATE; }
		const uint32_t rounds = static_cast<uint32_t>(cap - done < batch ? cap - done : batch);
		launch_settle_rounds(d, labels, comps, chosen, workspace, static_cast<uint32_t>(done) + 1u, rounds, stream);
		done += rounds;
		BM_HIP(hipMemcpyAsync(seen, tail + 4 * kSettleTailCountWord, sizeof(seen), hipMemcpyDeviceToHost, stream));
		BM_HIP(hipStreamSynchronize(stream));
		++looks;
		changes = seen[done % 3]; // what round `done` counted
		cap = static_cast<uint64_t>(seen[3]) + 2;
	}
	stamp(2);
	launch_settle_move(d, labels, comps, chosen, out, drops, result, workspace, stream);
	stamp(3);
	BM_HIP(hipGetLastError());
	BM_HIP(hipStreamSynchronize(stream)); // the call returns when out, the drops and the record stand
	if (counts) {
		counts[0] = static_cast<uint32_t>(done);
		counts[1] = looks;
	}
	if (stage_ms) return marks.read(3, stage_ms);
	return 0;
}

// ---- ground navigation (bm_foot_room, bm_foot_field, bm_foot_paths): kernels on the caller's stream over the caller's buffers; nothing of
// the world is read.  The host loop of the rounds is that of travel_field: batches of rounds, and between them one word read back.
int foot_room(const Gpu& gpu, const bm_foot_params* params, const uint8_t* volume, uint8_t* room, hipStream_t stream) {
	if (!params) { set_error("bm_foot_room: null params"); return BM_EINVAL; }
	const FootParamsView pv = foot_params_view(*params);
	if (const char* why = foot_params_problem(pv)) { set_error(std::string("bm_foot_room: ") + why); return BM_EINVAL; }
	if (!volume || !room) { set_error("bm_foot_room: null volume or room"); return BM_EINVAL; }
	const FootDims d = foot_dims(pv);
	const size_t span = static_cast<size_t>(foot_span(d));
	BM_HIP(hipSetDevice(gpu.device));
	// (a volume whose pitches carry it past its allocation has no extent to overlap anything with, see mesh_quads)
	const bool volume_ok = device_span_ok(gpu.device, volume, span);
	if (volume_ok && spans_overlap(span_of(volume, span), span_of(room, d.voxels))) { set_error("bm_foot_room: the room volume overlaps the byte volume"); return BM_EINVAL; }
	if (!volume_ok || !device_span_ok(gpu.device, room, d.voxels)) {
		set_error("bm_foot_room: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	launch_foot_room(d, volume, room, stream);
	BM_HIP(hipGetLastError());
	return 0;
}

int foot_field(const Gpu& gpu, const bm_foot_params* params, const uint8_t* room, const int32_t* seeds, int64_t n, uint32_t* field, bm_foot_result* result, void* workspace,
			   size_t workspace_bytes, hipStream_t stream, uint32_t batch, float* stage_ms, uint32_t* counts) {
	if (!params) { set_error("bm_foot_field: null params"); return BM_EINVAL; }
	const FootParamsView pv = foot_params_view(*params);
	if (const char* why = foot_params_problem(pv)) { set_error(std::string("bm_foot_field: ") + why); return BM_EINVAL; }
	if (n < 0 || n > 0x7FFFFFFF) { set_error("bm_foot_field: a negative number of seeds, or more than 2^31 - 1"); return BM_EINVAL; }
	if (!room || !field || !result || !workspace || (n > 0 && !seeds)) { set_error("bm_foot_field: null room, seeds, field, result or workspace"); return BM_EINVAL; }
	const FootDims d = foot_dims(pv);
	const size_t need = foot_workspace_bytes(d);
	if (workspace_bytes < need) { set_error("bm_foot_field: the workspace is smaller than bm_foot_workspace_bytes"); return BM_EINVAL; }
	if (!aligned(field, 4) || !aligned(seeds, 4) || !aligned(result, 8) || !aligned(workspace, 16)) {
		set_error("bm_foot_field: the field and the seeds must be 4-byte, the result 8-byte and the workspace 16-byte aligned");
		return BM_EINVAL;
	}
	const size_t room_bytes = d.voxels, field_bytes = static_cast<size_t>(d.voxels) * sizeof(uint32_t), seed_bytes = static_cast<size_t>(n) * 12;
	const Span ws = span_of(workspace, need), fs = span_of(field, field_bytes), ss = span_of(seeds, seed_bytes), rs = span_of(result, sizeof(bm_foot_result)),
			   os = span_of(room, room_bytes);
	if (spans_overlap(fs, ws) || spans_overlap(ss, ws) || spans_overlap(rs, ws)) {
		set_error("bm_foot_field: the workspace overlaps the seeds, the field or the result");
		return BM_EINVAL;
	}
	if (spans_overlap(ss, fs) || spans_overlap(rs, fs)) { set_error("bm_foot_field: the field overlaps the seeds or the result"); return BM_EINVAL; }
	if (spans_overlap(os, fs) || spans_overlap(os, ws) || spans_overlap(os, rs)) {
		set_error("bm_foot_field: the room volume overlaps the field, the workspace or the result");
		return BM_EINVAL;
	}
	BM_HIP(hipSetDevice(gpu.device));
	if (!device_span_ok(gpu.device, room, room_bytes) || !device_span_ok(gpu.device, workspace, need) || !device_span_ok(gpu.device, field, field_bytes) ||
		(n > 0 && !device_span_ok(gpu.device, seeds, seed_bytes)) || !device_span_ok(gpu.device, result, sizeof(bm_foot_result))) {
		set_error("bm_foot_field: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	if (batch == 0) batch = kFootBatch;
	StageMarks<4> marks;
	if (stage_ms) {
		if (int e = marks.create(4)) return e;
	}
	auto stamp = [&](int i) { if (stage_ms) (void)hipEventRecord(marks.marks()[i], stream); };
	stamp(0);
	launch_foot_setup(d, room, seeds, static_cast<uint32_t>(n), field, workspace, stream);
	stamp(1);
	// Round k gives the value k, every round but the last appends a stand that was not in the queue, and no value is above the limit:
	// the front is empty after that many rounds + 2.
	const uint64_t cap = static_cast<uint64_t>(pv.max_steps != 0 && pv.max_steps < d.queue ? pv.max_steps : d.queue) + 2;
	const uint8_t* tail = static_cast<const uint8_t*>(workspace) + foot_tail_offset(d);
	uint64_t done = 0;
	uint32_t looks = 0, front = n > 0 ? 1u : 0u; // (without seeds no level ever holds a stand)
	while (front != 0) {
		if (done >= cap) { set_error("bm_foot_field: internal error: the front is not empty after every round the field can need"); return BM_ESTATE; }
		const uint32_t rounds = static_cast<uint32_t>(cap - done < batch ? cap - done : batch);
		launch_foot_rounds(d, room, field, workspace, static_cast<uint32_t>(done) + 1u, rounds, stream);
		done += rounds;
		// the size of the next front, level `done`: what round done + 1 would read
		BM_HIP(hipMemcpyAsync(&front, tail + 4 * (kFootTailCountWord + done % 3), 4, hipMemcpyDeviceToHost, stream));
		BM_HIP(hipStreamSynchronize(stream));
		++looks;
	}
	stamp(2);
	launch_foot_finish(d, field, result, workspace, static_cast<uint32_t>(done), stream);
	stamp(3);
	BM_HIP(hipGetLastError());
	BM_HIP(hipStreamSynchronize(stream)); // the call returns when the field and the record stand
	if (counts) {
		counts[0] = static_cast<uint32_t>(done);
		counts[1] = looks;
	}
	if (stage_ms) return marks.read(3, stage_ms);
	return 0;
}

int foot_paths(const Gpu& gpu, const bm_foot_params* params, const uint8_t* room, const uint32_t* field, const int32_t* starts, int64_t n, int32_t capacity, int32_t* path,
			   int32_t* lengths, hipStream_t stream) {
	if (!params) { set_error("bm_foot_paths: null params"); return BM_EINVAL; }
	const FootParamsView pv = foot_params_view(*params);
	if (const char* why = foot_params_problem(pv)) { set_error(std::string("bm_foot_paths: ") + why); return BM_EINVAL; }
	if (n < 0 || n > 0x7FFFFFFF) { set_error("bm_foot_paths: a negative number of starts, or more than 2^31 - 1"); return BM_EINVAL; }
	if (capacity < 1) { set_error("bm_foot_paths: a capacity below 1"); return BM_EINVAL; }
	if (!room || !field || (n > 0 && (!starts || !path || !lengths))) { set_error("bm_foot_paths: null room, field, starts, path or lengths"); return BM_EINVAL; }
	if (!all_aligned(4, field, starts, path, lengths)) { set_error("bm_foot_paths: the field, the starts, the path and the lengths must be 4-byte aligned"); return BM_EINVAL; }
	if (static_cast<uint64_t>(n) * static_cast<uint64_t>(capacity) > (uint64_t{1} << 40)) { set_error("bm_foot_paths: more than 2^40 path voxels"); return BM_EINVAL; }
	const FootDims d = foot_dims(pv);
	const size_t room_bytes = d.voxels, field_bytes = static_cast<size_t>(d.voxels) * sizeof(uint32_t), start_bytes = static_cast<size_t>(n) * 12,
				 path_bytes = start_bytes * static_cast<size_t>(capacity), length_bytes = static_cast<size_t>(n) * 4;
	const Span os = span_of(room, room_bytes), fs = span_of(field, field_bytes), ss = span_of(starts, start_bytes), ps = span_of(path, path_bytes),
			   ls = span_of(lengths, length_bytes);
	if (spans_overlap(ps, fs) || spans_overlap(ps, ss) || spans_overlap(ls, fs) || spans_overlap(ls, ss) || spans_overlap(ps, ls)) {
		set_error("bm_foot_paths: the path or the lengths buffer overlaps the field, the starts or the other of the two");
		return BM_EINVAL;
	}
	if (spans_overlap(os, ps) || spans_overlap(os, ls)) { set_error("bm_foot_paths: the room volume overlaps the path or the lengths"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(gpu.device));
	if (!device_span_ok(gpu.device, room, room_bytes) || !device_span_ok(gpu.device, field, field_bytes) ||
		(n > 0 && (!device_span_ok(gpu.device, starts, start_bytes) || !device_span_ok(gpu.device, path, path_bytes) || !device_span_ok(gpu.device, lengths, length_bytes)))) {
		set_error("bm_foot_paths: a buffer does not lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	if (n == 0) return 0;
	launch_foot_paths(d, room, field, starts, static_cast<uint32_t>(n), capacity, path, lengths, stream);
	BM_HIP(hipGetLastError());
	return 0;
}

int pixel_rays(const Gpu& gpu, const bm_camera* cam, int width, int height, bm_ray* rays, hipStream_t stream) {
	if (!cam || !rays || width < 1 || height < 1 || width > 65535 || height > 65535 || !aligned(rays, 16)) {
		set_error("bm_camera_pixel_rays_device: bad argument (null, a size outside 1 ... 65535, or rays not 16-byte aligned)");
		return BM_EINVAL;
	}
	const CameraBasis basis = camera_basis(cam->position, cam->direction, cam->up, width, height); // the frames' basis, as bm_camera_pixel_rays takes it
	PixelRayBasis b;
	for (int k = 0; k < 3; ++k) { b.right[k] = basis.right[k]; b.up[k] = basis.up[k]; b.dir[k] = basis.dir[k]; b.origin[k] = basis.origin[k]; }
	b.width = width; b.height = height;
	BM_HIP(hipSetDevice(gpu.device));
	launch_pixel_rays(b, rays, stream);
	BM_HIP(hipGetLastError());
	return 0;
}

// ---- temporal accumulation (bm_reproject): like the filter, nothing of the world is read and nothing is kept
int reproject(const Gpu& gpu, const bm_reproject_params* params, const bm_camera* cam, const bm_camera* cam_prev, const float* accum, const bm_ray_hit* hits,
			  const void* history_prev, void* history_out, hipStream_t stream) {
	if (!params || !cam || !accum || !hits || !history_out) { set_error("bm_reproject: null argument"); return BM_EINVAL; }
	if (history_prev && !cam_prev) { set_error("bm_reproject: a previous history needs the camera it was made with"); return BM_EINVAL; }
	const ReprojectParamsView pv = {params->width, params->height, params->max_history, params->flags, params->reserved};
	if (const char* why = reproject_params_problem(pv)) { set_error(std::string("bm_reproject: ") + why); return BM_EINVAL; }
	if (!all_aligned(16, accum, hits, history_prev, history_out)) { set_error("bm_reproject: buffers must be 16-byte aligned"); return BM_EINVAL; }
	const size_t history = history_bytes(params->width, params->height), image = history / 20 * 16;
	const Span written = span_of(history_out, history);
	if ((history_prev && spans_overlap(span_of(history_prev, history), written)) || spans_overlap(span_of(accum, image), written) || spans_overlap(span_of(hits, 2 * image), written)) {
		set_error("bm_reproject: history_out overlaps an input (taps read neighbours: ping-pong two histories)");
		return BM_EINVAL;
	}
	ReprojectCameras cams;
	cams.cur = camera_basis(cam->position, cam->direction, cam->up, params->width, params->height);
	// (without a history the previous camera is not read; the current one stands in so that the argument holds defined values)
	const bm_camera* before = history_prev ? cam_prev : cam;
	cams.prev = reproject_prev_camera(camera_basis(before->position, before->direction, before->up, params->width, params->height));
	cams.width = params->width; cams.height = params->height;
	BM_HIP(hipSetDevice(gpu.device));
	launch_reproject(cams, params->max_history, accum, hits, history_prev, history_out, stream);
	BM_HIP(hipGetLastError());
	return 0;
}

} // namespace bm
