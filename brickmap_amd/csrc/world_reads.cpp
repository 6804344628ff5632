// world_reads.cpp -- see world_reads.h
#include "world_reads.h"

#include <climits>
#include <string>

#include "device_ops.h"
#include "kernels.h"

namespace bm {

template <class T, class Launch> int WorldReads::issue_frame(hipStream_t stream, T* turn, Launch&& launch) {
	if (int e = ready_()) return e;
	if (int e = order_->begin(stream)) return e; // bricks uploaded on the load stream must be visible to this read
	FrameOrder::Ending frame(*order_, stream);
	if (turn) { if (int e = turn->order(stream)) return e; }
	if (int e = launch(DeviceScene(*view_))) return e;
	BM_HIP(hipGetLastError());
	if (turn) { if (int e = turn->pass(stream)) return e; }
	(void)frame.end(); // what process_load_queue orders itself behind
	return 0;
}

template <class B> int WorldReads::reserve_behind(Turn& turn, B& scratch, size_t bytes) {
	if (scratch.bytes() >= bytes) return 0;
	if (int e = turn.wait()) return e;
	return scratch.reserve(scratch_grown(bytes));
}

int WorldReads::stage_patches(const PatchList& list) {
	const PatchList::Layout at = list.layout();
	if (at.n == 0) return 0;
	if (int e = patches_.wait()) return e; // the host rewrites the pinned list: the previous call's copy has run
	if (int e = reserve_behind(patches_, h_patch_, at.bytes)) return e;
	if (int e = reserve_behind(patches_, d_patch_, at.bytes)) return e;
	list.fill(h_patch_);
	return 0;
}

// ---------------------------------------------------------------- dense regions (bm_scene_read_region)
int WorldReads::read_region(const bm_region& r, uint8_t* voxels, int where, hipStream_t stream) {
	const WorldDims& d = world_->dims;
	int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
	const bool inside = World::region_bounds(d, r, lo, hi);
	if (where == BM_VOXELS_HOST) {
		outside_slabs(r.lo, r.hi, inside, lo, hi, [&](int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1) {
			for (int64_t z = z0; z < z1; ++z)
				for (int64_t y = y0; y < y1; ++y) std::memset(voxels + region_offset(r, x0, y, z), 0, static_cast<size_t>(x1 - x0));
		});
		if (inside) world_->store_region(lo, hi, r.lo, voxels, r.row_pitch, r.slice_pitch, 16);
		return 0;
	}
	const PatchList list(*world_, residency_->book(), inside, lo, hi);
	const PatchList::Layout at = list.layout();
	if (int e = stage_patches(list)) return e;
	return issue_frame(stream, static_cast<Turn*>(nullptr), [&](const DeviceScene& view) -> int {
		outside_slabs(r.lo, r.hi, inside, lo, hi, [&](int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1) {
			launch_region_zero(voxels + region_offset(r, x0, y0, z0), r.row_pitch, r.slice_pitch, x1 - x0, y1 - y0, z1 - z0, stream);
		});
		if (!inside) return 0;
		const RegionDims rd = region_dims(d, r, lo, hi);
		launch_region_unpack(voxels, view.index_grid, view.pool_base, view.brick_arena, rd, stream);
		if (at.n == 0) return 0;
		BM_HIP(hipMemcpyAsync(d_patch_, h_patch_, at.bytes, hipMemcpyHostToDevice, stream));
		launch_region_patch(voxels, reinterpret_cast<const int*>(d_patch_.get()), reinterpret_cast<const uint32_t*>(d_patch_ + at.o_bricks), static_cast<uint32_t>(at.n), rd, stream);
		return patches_.pass(stream);
	});
}

// ---------------------------------------------------------------- connected components (bm_scene_label_region / _components / _mask)
int WorldReads::check_label_box(const char* who, const int32_t lo[3], const int32_t hi[3], LabelDims* d, bool* empty) {
	const char* why = bm::check_label_box(lo, hi, world_->dims.supergrid_xy, d, empty);
	if (why) { set_error(std::string(who) + ": " + why); return BM_EINVAL; }
	return 0;
}

int WorldReads::label_region(const int32_t lo[3], const int32_t hi[3], uint32_t flags, int32_t* labels, uint64_t* count, hipStream_t stream) {
	LabelDims ld;
	bool empty = false;
	if (flags != 0) { set_error("bm_scene_label_region: unknown flags (must be 0)"); return BM_EINVAL; }
	if (int e = check_label_box("bm_scene_label_region", lo, hi, &ld, &empty)) return e;
	if (!count || (!empty && !labels)) { set_error("bm_scene_label_region: null label volume or count"); return BM_EINVAL; }
	if (!aligned(count, 8) || (!empty && !aligned(labels, 4))) {
		set_error("bm_scene_label_region: labels must be 4-byte aligned, count 8-byte aligned");
		return BM_EINVAL;
	}
	if (int e = ready_()) return e;
	const size_t voxels = static_cast<size_t>(ld.nx) * ld.ny * ld.nz;
	if (!device_span_ok(device_, count, sizeof(uint64_t)) ||
		(!empty && !device_span_ok(device_, labels, voxels * sizeof(int32_t)))) {
		set_error("bm_scene_label_region: the label volume's whole span and the count must lie inside one allocation each of the scene's device");
		return BM_EINVAL;
	}
	const bool inside = !empty && label_clip(world_->dims, lo, hi, &ld);
	const PatchList list(*world_, residency_->book(), inside, ld.lo, ld.hi);
	const PatchList::Layout at = list.layout();
	if (int e = stage_patches(list)) return e;
	if (int e = label_marks_.create()) return e;
	return issue_frame(stream, &label_, [&](const DeviceScene& view) -> int {
		BM_HIP(hipMemsetAsync(count, 0, sizeof(uint64_t), stream));
		label_clock_.begun();
		if (empty) return 0;
		uint8_t* const bytes_out = reinterpret_cast<uint8_t*>(labels);
		const LabelPitch pitch(ld);
		outside_slabs(lo, hi, inside, ld.lo, ld.hi, [&](int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1) {
			launch_region_zero(bytes_out + pitch.offset(ld, x0, y0, z0), pitch.row, pitch.slice, (x1 - x0) * 4, y1 - y0, z1 - z0, stream);
		});
		if (!inside) return 0;
		if (at.n > 0) BM_HIP(hipMemcpyAsync(d_patch_, h_patch_, at.bytes, hipMemcpyHostToDevice, stream));
		launch_label_region(view, reinterpret_cast<uint32_t*>(labels), count, ld, reinterpret_cast<const int*>(d_patch_.get()),
							reinterpret_cast<const uint32_t*>(d_patch_.get() + at.o_bricks), static_cast<uint32_t>(at.n), stream, label_marks_.marks());
		label_clock_.launched();
		return at.n > 0 ? patches_.pass(stream) : 0;
	});
}

int WorldReads::last_label_ms(float* local_ms, float* merge_ms, float* flatten_ms) {
	if (!local_ms || !merge_ms || !flatten_ms) { set_error("null argument"); return BM_EINVAL; }
	if (const char* why = label_clock_.refused()) { set_error(why); return BM_ESTATE; }
	BM_HIP(hipSetDevice(device_));
	float ms[3];
	if (int e = label_marks_.read(3, ms)) return e;
	*local_ms = ms[0]; *merge_ms = ms[1]; *flatten_ms = ms[2];
	return 0;
}

int WorldReads::label_components(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, bm_component* comps, int64_t capacity, hipStream_t stream) {
	LabelDims ld;
	bool empty = false;
	if (int e = check_label_box("bm_scene_label_components", lo, hi, &ld, &empty)) return e;
	if (capacity < 0) { set_error("bm_scene_label_components: negative capacity"); return BM_EINVAL; }
	if (empty || capacity == 0) return 0;
	if (!labels || !comps) { set_error("bm_scene_label_components: null label volume or table"); return BM_EINVAL; }
	if (!aligned(labels, 4) || !aligned(comps, 8)) {
		set_error("bm_scene_label_components: labels must be 4-byte aligned, the table 8-byte aligned");
		return BM_EINVAL;
	}
	if (int e = ready_()) return e;
	const size_t voxels = static_cast<size_t>(ld.nx) * ld.ny * ld.nz;
	const size_t records = static_cast<size_t>(std::min<int64_t>(capacity, static_cast<int64_t>(voxels))); // (no more components than voxels)
	if (!device_span_ok(device_, labels, voxels * sizeof(int32_t)) ||
		!device_span_ok(device_, comps, records * sizeof(bm_component))) {
		set_error("bm_scene_label_components: the label volume and min(capacity, voxels) records must lie inside one allocation each of the scene's device");
		return BM_EINVAL;
	}
	label_clip(world_->dims, lo, hi, &ld);
	if (int e = reserve_behind(label_, d_label_tmp_, label_tmp_bytes(static_cast<uint32_t>(voxels)))) return e;
	if (int e = label_.order(stream)) return e;
	launch_label_components(reinterpret_cast<const uint32_t*>(labels), comps, static_cast<uint64_t>(capacity), ld, d_label_tmp_, stream);
	BM_HIP(hipGetLastError());
	return label_.pass(stream);
}

int WorldReads::label_mask(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, const bm_component* comps, int64_t n, const uint8_t* chosen, uint8_t* mask,
						   hipStream_t stream) {
	LabelDims ld;
	bool empty = false;
	if (int e = check_label_box("bm_scene_label_mask", lo, hi, &ld, &empty)) return e;
	if (n < 0) { set_error("bm_scene_label_mask: negative record count"); return BM_EINVAL; }
	if (empty) return 0;
	if (!labels || !mask || (n > 0 && (!comps || !chosen))) { set_error("bm_scene_label_mask: null buffer"); return BM_EINVAL; }
	if (!aligned(labels, 4) || !aligned(comps, 8)) {
		set_error("bm_scene_label_mask: labels must be 4-byte aligned, the table 8-byte aligned");
		return BM_EINVAL;
	}
	if (int e = ready_()) return e;
	const size_t voxels = static_cast<size_t>(ld.nx) * ld.ny * ld.nz;
	if (!device_span_ok(device_, labels, voxels * sizeof(int32_t)) || !device_span_ok(device_, mask, voxels) ||
		(n > 0 && (!device_span_ok(device_, comps, static_cast<size_t>(n) * sizeof(bm_component)) || !device_span_ok(device_, chosen, static_cast<size_t>(n))))) {
		set_error("bm_scene_label_mask: every buffer's whole span must lie inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	if (int e = label_.order(stream)) return e;
	launch_label_mask(reinterpret_cast<const uint32_t*>(labels), static_cast<uint32_t>(voxels), comps, static_cast<uint64_t>(n), chosen, mask, stream);
	BM_HIP(hipGetLastError());
	return label_.pass(stream);
}

// ---------------------------------------------------------------- ray queries (bm_scene_cast_rays)
int WorldReads::TicketRing::create() {
	if (tickets_) return 0;
	if (int e = tickets_.alloc(kQueryRing * 128)) return e;
	for (Event& ev : ev_) if (int e = ev.create(hipEventDisableTiming)) return e;
	return 0;
}

int WorldReads::TicketRing::order(hipStream_t stream) const {
	if (ring_.reused()) BM_HIP(hipStreamWaitEvent(stream, ev_[ring_.slot()], 0));
	return 0;
}

int WorldReads::TicketRing::pass(hipStream_t stream) {
	BM_HIP(hipEventRecord(ev_[ring_.slot()], stream));
	ring_.issued();
	return 0;
}

int WorldReads::cast_rays(int64_t n, const bm_ray* rays, bm_ray_hit* hits, uint32_t flags, const float* lod_origin, hipStream_t stream) {
	int campos[3] = {0, 0, 0};
	bool nothing = false;
	if (const char* why = check_cast_rays(n, rays, hits, flags, lod_origin, campos, &nothing)) { set_error(why); return BM_EINVAL; }
	if (nothing) return 0;
	if (int e = ready_()) return e;
	if (!query_blocks_per_cu_[0]) {
		if (int e = tickets_.create()) return e;
		query_blocks_per_cu_[0] = query_blocks_per_cu(false);
		query_blocks_per_cu_[1] = query_blocks_per_cu(true);
	}
	const bool request = !(flags & BM_QUERY_NO_REQUESTS);
	return issue_frame(stream, &tickets_, [&](DeviceScene view) -> int {
		if (!(flags & BM_QUERY_LOD)) view.lod_distance_8x8x8 = view.lod_distance_2x2x2 = INT_MAX; // exact: every brick at voxel level
		uint32_t* const ticket = tickets_.ticket();
		BM_HIP(hipMemsetAsync(ticket, 0, sizeof(uint32_t), stream));
		launch_query(view, campos, rays, hits, static_cast<uint32_t>(n), ticket, query_blocks_per_cu_[request ? 1 : 0] * *compute_units_, request, stream);
		return 0;
	});
}

// ---------------------------------------------------------------- volume queries (bm_scene_query_volumes)
int WorldReads::query_volumes(int64_t n, const bm_volume* volumes, bm_volume_result* results, uint32_t flags, hipStream_t stream) {
	bool nothing = false;
	if (const char* why = check_query_volumes(n, volumes, results, flags, &nothing)) { set_error(why); return BM_EINVAL; }
	if (nothing) return 0;
	if (int e = ready_()) return e;
	if (!volume_blocks_per_cu_[0]) {
		volume_blocks_per_cu_[0] = volume_blocks_per_cu(false);
		volume_blocks_per_cu_[1] = volume_blocks_per_cu(true);
	}
	if (int e = reserve_behind(volume_, d_volume_tmp_, volume_tmp_bytes(static_cast<uint32_t>(n)))) return e;
	const bool any = (flags & BM_VOLUME_ANY) != 0;
	return issue_frame(stream, &volume_, [&](const DeviceScene& view) -> int {
		launch_volume_query(view, volumes, results, static_cast<uint32_t>(n), any, d_volume_tmp_, volume_blocks_per_cu_[any ? 1 : 0] * *compute_units_, stream);
		return 0;
	});
}

} // namespace bm
