// world_changes.cpp -- see world_changes.h
#include "world_changes.h"

#include <algorithm>

#include "kernels.h"

namespace bm {

int WorldChanges::edit(int count, const bm_edit* edits, hipStream_t stream) {
	const WorldDims& d = world_->dims;
	std::vector<int> reached;
	{
		std::vector<uint8_t> seen(static_cast<size_t>(d.supercells), 0);
		std::vector<int> of_edit;
		for (int i = 0; i < count; ++i) {
			int lo[3], hi[3];
			if (!World::edit_bounds(d, edits[i], lo, hi)) continue;
			of_edit.clear();
			supercells_reached(d, lo, hi, &of_edit);
			for (const int sc : of_edit)
				if (!seen[sc]) { seen[sc] = 1; reached.push_back(sc); }
		}
	}
	if (reached.empty()) return 0;
	std::sort(reached.begin(), reached.end());
	BM_HIP(hipSetDevice(device_));
	if (int e = edit_staging_.wait()) return e; // the staging of the previous batch has been copied

	// ---- host world, supercell by supercell (voxels of different supercells are independent: batch order is kept within each)
	CellBatch batch;
	residency_->begin_batch();
	std::vector<uint32_t> old_words;
	std::vector<uint8_t> touched;
	for (const int sci : reached) {
		HostSupercell& c = world_->supercells[sci];
		int sx, sy, sz;
		d.supercell_coords(sci, &sx, &sy, &sz);
		old_words = c.indices;
		touched.assign(kCellsPerSupercell, 0);
		World::edit_supercell(d, c, sx, sy, sz, edits, count, touched.data());
		if (int e = stage(sci, old_words, touched.data(), batch)) return e;
	}
	if (int e = submit(batch, stream, edit_marks_.marks())) return e;
	edit_clocked_ = edit_clocked(edit_clocked_, batch.clocked());
	return 0;
}

int WorldChanges::stage(int sci, const std::vector<uint32_t>& old_words, const uint8_t* touched, CellBatch& b) {
	if (int e = residency_->rebind(sci, old_words, touched)) return e;
	b.add_supercell(world_->dims, sci, world_->supercells[sci], old_words, touched, residency_->book().pool(sci));
	return 0;
}

int WorldChanges::submit(CellBatch& b, hipStream_t stream, hipEvent_t* marks) {
	const uint32_t n = static_cast<uint32_t>(b.cells.size());
	if (n == 0) { // nothing inside the world changed a brick (e.g. clearing empty space)
		residency_->commit_batch();
		return 0;
	}
	const hipStream_t load_stream = *load_stream_;
	const std::vector<PoolMove>& moves = residency_->moves();
	const StagingLayout at(moves.size(), n);
	auto stage = [&]() -> int {
		if (at.bytes > d_edit_.bytes()) { // (the two grow together: h_edit_ is as large as d_edit_)
			BM_HIP(hipStreamSynchronize(load_stream)); // the previous batch's kernels may still read the device staging
			if (int e = h_edit_.reserve(StagingLayout::grown(at.bytes))) return e;
			if (int e = d_edit_.reserve(StagingLayout::grown(at.bytes))) return e;
		}
		if (int e = fields_->prepare_update(b.change, load_stream)) return e;
		at.fill(h_edit_, moves, b);
		return 0;
	};
	// behind every frame in flight (they read the words, pool bases, bricks and field this rewrites) and the caller's queued work
	auto queue = [&]() -> int {
		if (int e = order_->load_behind_caller(stream)) return e;
		BM_HIP(hipMemcpyAsync(d_edit_, h_edit_, at.bytes, hipMemcpyHostToDevice, load_stream));
		if (int e = edit_staging_.pass(load_stream)) return e; // the pinned staging is free again from here on
		BM_HIP(hipEventRecord(marks[0], load_stream));
		if (!moves.empty()) {
			launch_pool_moves(reinterpret_cast<const PoolMove*>(d_edit_.get()), static_cast<uint32_t>(moves.size()), residency_->arena_base(), residency_->pool_base(), load_stream);
			BM_HIP(hipGetLastError());
		}
		launch_edit_scatter(reinterpret_cast<const uint32_t*>(d_edit_ + at.o_cells), reinterpret_cast<const uint32_t*>(d_edit_ + at.o_words),
							reinterpret_cast<const uint32_t*>(d_edit_ + at.o_slots), reinterpret_cast<const uint32_t*>(d_edit_ + at.o_bricks), n, residency_->index_grid(),
							residency_->arena_base(), load_stream);
		BM_HIP(hipGetLastError());
		BM_HIP(hipEventRecord(marks[1], load_stream));
		// the field and the escape heights where some cell's occupancy changed; what that makes stale is rebuilt before the next frame that reads it
		if (int e = fields_->update(residency_->index_grid(), b.change, true, load_stream)) return e;
		BM_HIP(hipEventRecord(marks[2], load_stream));
		return 0;
	};
	int e = stage();
	if (!e) e = order_->publish_behind_frames(queue);
	if (residency_->report(e)) return e; // the host world is ahead of the device: refuse to go on
	residency_->commit_batch();
	return 0;
}

int WorldChanges::last_edit_ms(float* scatter_ms, float* field_ms) {
	if (!scatter_ms || !field_ms) { set_error("null argument"); return BM_EINVAL; }
	if (!edit_clocked_) { set_error("no edit has changed the scene yet"); return BM_ESTATE; }
	BM_HIP(hipSetDevice(device_));
	float ms[2];
	if (int e = edit_marks_.read(2, ms)) return e;
	edit_ms(edit_clocked_, ms, scatter_ms, field_ms);
	return 0;
}

int WorldChanges::write_region(const bm_region& r, int op, const uint8_t* voxels, int where, hipStream_t stream) {
	const WorldDims& d = world_->dims;
	const hipStream_t load_stream = *load_stream_;
	int lo[3], hi[3];
	if (!World::region_bounds(d, r, lo, hi)) return 0;
	if (int e = edit_staging_.wait()) return e;
	if (int e = region_marks_.create()) return e;
	hipEvent_t* const marks = region_marks_.marks();
	const RegionDims rd = region_dims(d, r, lo, hi);
	World::RegionSource src;
	for (int k = 0; k < 3; ++k) { src.c0[k] = rd.c0[k]; src.nc[k] = rd.nc[k]; src.origin[k] = r.lo[k]; }
	if (where == BM_VOXELS_DEVICE) {
		const size_t bytes = static_cast<size_t>(rd.nc[0]) * rd.nc[1] * rd.nc[2] * sizeof(Brick);
		if (bytes > d_region_.bytes()) { // (no earlier write still uses them: each waits for its copy)
			if (int e = d_region_.reserve(std::max<size_t>(bytes, 1 << 16))) return e;
			if (int e = h_region_.reserve(std::max<size_t>(bytes, 1 << 16))) return e;
		}
		if (int e = order_->load_behind_caller(stream)) return e; // the volume is whatever the caller's stream has written by now
		BM_HIP(hipEventRecord(marks[0], load_stream));
		launch_region_pack(voxels, reinterpret_cast<uint32_t*>(d_region_.get()), rd, load_stream);
		BM_HIP(hipGetLastError());
		BM_HIP(hipEventRecord(marks[1], load_stream));
		BM_HIP(hipMemcpyAsync(h_region_, d_region_, bytes, hipMemcpyDeviceToHost, load_stream));
		BM_HIP(hipEventRecord(marks[2], load_stream));
		BM_HIP(hipStreamSynchronize(load_stream));
		src.packed = h_region_;
	} else {
		src.voxels = voxels;
		src.row_pitch = r.row_pitch;
		src.slice_pitch = r.slice_pitch;
	}
	// ---- merge, on CPU threads: supercells are independent
	std::vector<int> reached;
	supercells_reached(d, lo, hi, &reached);
	std::vector<std::vector<uint32_t>> old_words(reached.size());
	std::vector<std::vector<uint8_t>> touched(reached.size());
	parallel_for(static_cast<int>(reached.size()), 16, [&](int i) {
		HostSupercell& c = world_->supercells[reached[i]];
		int sx, sy, sz;
		d.supercell_coords(reached[i], &sx, &sy, &sz);
		old_words[i] = c.indices;
		touched[i].assign(kCellsPerSupercell, 0);
		World::write_region_supercell(d, c, sx, sy, sz, lo, hi, op, src, touched[i].data());
	});
	CellBatch batch;
	residency_->begin_batch();
	for (size_t i = 0; i < reached.size(); ++i)
		if (int e = stage(reached[i], old_words[i], touched[i].data(), batch)) return e;
	region_clocked_ = region_clocked(where == BM_VOXELS_DEVICE, 0);
	if (int e = submit(batch, stream, marks + 3)) return e;
	region_clocked_ = region_clocked(where == BM_VOXELS_DEVICE, batch.clocked());
	return 0;
}

int WorldChanges::last_region_ms(float* pack_ms, float* copy_ms, float* scatter_ms, float* field_ms) {
	if (!pack_ms || !copy_ms || !scatter_ms || !field_ms) { set_error("null argument"); return BM_EINVAL; }
	if (!region_clocked_) { set_error("no region has been written yet"); return BM_ESTATE; }
	BM_HIP(hipSetDevice(device_));
	float ms[4] = {0.f, 0.f, 0.f, 0.f};
	if (region_clocked_ & kClockedPack) { if (int e = region_marks_.read(2, ms)) return e; }
	if (region_clocked_ & kClockedScatter) { if (int e = region_marks_.read(2, ms + 2, 3)) return e; }
	region_ms(region_clocked_, ms, pack_ms, copy_ms, scatter_ms, field_ms);
	return 0;
}

} // namespace bm
