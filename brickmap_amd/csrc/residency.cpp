// residency.cpp -- see residency.h
#include "residency.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <fstream>

#include "kernels.h"

namespace bm {

int Residency::init(DeviceScene* view) {
	view_ = view;
	for (int r = 0; r < 2; ++r) {
		if (int e = h_count_[r].alloc(sizeof(uint32_t))) return e;
		if (int e = d_load_count_[r].alloc(sizeof(uint32_t))) return e;
		BM_HIP(hipMemset(d_load_count_[r], 0, sizeof(uint32_t)));
	}
	return 0;
}

int Residency::alloc_queue() {
	BM_HIP(hipSetDevice(device_));
	const size_t n = static_cast<size_t>(queue_cap_);
	for (int r = 0; r < 2; ++r) {
		if (int e = h_positions_[r].alloc(n * 3 * sizeof(int))) return e; // Scene.cpp:30
		if (int e = d_load_queue_[r].alloc(n * 3 * sizeof(int))) return e; // Scene.cpp:186
		BM_HIP(hipMemset(d_load_queue_[r], 0, n * 3 * sizeof(int)));
		BM_HIP(hipMemset(d_load_count_[r], 0, sizeof(uint32_t)));
	}
	if (int e = h_bricks_.alloc(n * sizeof(Brick))) return e;             // Scene.cpp:31
	if (int e = h_indices_.alloc(n * sizeof(uint32_t))) return e;         // Scene.cpp:32
	if (int e = d_bricks_queue_.alloc(n * sizeof(Brick))) return e;       // Scene.cpp:189
	if (int e = d_indices_queue_.alloc(n * sizeof(uint32_t))) return e;   // Scene.cpp:190
	if (int e = d_positions_.alloc(n * 3 * sizeof(int))) return e;
	// a batch of n requests can make at most n pools grow
	if (int e = h_moves_.alloc(n * sizeof(PoolMove))) return e;
	if (int e = d_moves_.alloc(n * sizeof(PoolMove))) return e;
	book_.rings_reset();
	use_ring(0);
	snapshot_.clear();
	view_->queue_cap = static_cast<uint32_t>(queue_cap_);
	return 0;
}

void Residency::use_ring(int ring) {
	view_->load_queue = d_load_queue_[ring];
	view_->load_queue_count = d_load_count_[ring];
}

int Residency::set_queue_capacity(int cap) {
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	queue_cap_ = cap;
	return alloc_queue();
}

int Residency::set_streaming_mode(int overlapped, FrameOrder& order, hipStream_t load_stream) {
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	const int drain = book_.mode_change(overlapped != 0).drain;
	if (drain >= 0) {
		snapshot_.clear();
		book_.snapshot_read();
		const uint32_t count = std::min<uint32_t>(static_cast<uint32_t>(queue_cap_), *h_count_[drain]);
		if (count > 0) {
			if (int e = service_ring(drain, count, order, load_stream, nullptr)) return e;
		}
		BM_HIP(hipDeviceSynchronize());
	}
	if (book_.mode_change(overlapped != 0).carry) {
		BM_HIP(hipMemcpy(d_load_queue_[0], d_load_queue_[1], static_cast<size_t>(queue_cap_) * 3 * sizeof(int), hipMemcpyDeviceToDevice));
		BM_HIP(hipMemcpy(d_load_count_[0], d_load_count_[1], sizeof(uint32_t), hipMemcpyDeviceToDevice));
		BM_HIP(hipMemset(d_load_count_[1], 0, sizeof(uint32_t)));
	}
	book_.mode_changed(overlapped != 0);
	use_ring(book_.ring());
	return 0;
}

// ---------------------------------------------------------------- the device memory of a world
int Residency::alloc_index_grid() {
	const WorldDims& d = world_->dims;
	const size_t index_bytes = static_cast<size_t>(d.supercells) * kCellsPerSupercell * sizeof(uint32_t);
	if (int e = d_index_grid_.alloc(index_bytes)) return e;
	if (int e = d_pool_base_.alloc(static_cast<size_t>(d.supercells) * sizeof(uint32_t))) return e;
	BM_HIP(hipMemset(d_pool_base_, 0, static_cast<size_t>(d.supercells) * sizeof(uint32_t)));
	view_->index_grid = d_index_grid_;
	view_->pool_base = d_pool_base_;
	view_->brick_arena = nullptr;
	return 0;
}

int Residency::open_arena(uint64_t world_bricks) {
	const int e = arena_.open(device_, 4 * world_bricks + 32ull * static_cast<uint64_t>(world_->dims.supercells) + (1ull << 16));
	if (!e) view_->brick_arena = arena_.base();
	return e;
}

int Residency::arena_fit(uint64_t bricks) {
	arena_.reset();
	bool left_unmapped = false;
	const int e = arena_.reserve(std::max<uint64_t>(bricks, 1), true, &left_unmapped);
	// (frames are refused until bm_scene_reset_residency / bm_scene_preload_all succeeds: view_->brick_arena points at an unmapped range)
	if (left_unmapped) book_.report(e);
	view_->brick_arena = arena_.base();
	return e;
}

int Residency::pool_region(uint32_t bricks, uint32_t* offset) {
	const int e = arena_.region_alloc(bricks, offset);
	view_->brick_arena = arena_.base();
	return e;
}

void Residency::release() {
	(void)d_index_grid_.release();
	(void)d_pool_base_.release();
	arena_.close();
}

int Residency::said(int e) {
	if (e && book_.why()) set_error(book_.why());
	return e;
}

// ---------------------------------------------------------------- a new residency
int Residency::reset() {
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	const WorldDims& d = world_->dims;
	std::vector<uint32_t> words(static_cast<size_t>(d.supercells) * kCellsPerSupercell);
	std::vector<uint32_t> bases(d.supercells, 0u);
	// every supercell that holds bricks starts with a pool of kStartingPool bricks (Scene.cpp:157-175, variables.h:15)
	uint64_t initial = 0;
	for (int i = 0; i < d.supercells; ++i) initial += world_->supercells[i].bricks.empty() ? 0u : PoolBook::kStartingPool;
	if (int e = arena_fit(initial)) return e;
	book_.begin_rebuild(d.supercells);
	for (int i = 0; i < d.supercells; ++i) {
		const HostSupercell& c = world_->supercells[i];
		if (int e = book_.start_pool(i, c.bricks.size(), region_alloc())) return e;
		bases[i] = book_.pool(i).base;
		uint32_t* dst = &words[static_cast<size_t>(i) * kCellsPerSupercell];
		for (int j = 0; j < kCellsPerSupercell; ++j) dst[j] = PoolBook::device_word(c.indices[j], kNoDeviceSlot);
	}
	BM_HIP(hipMemcpy(d_index_grid_, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	BM_HIP(hipMemcpy(d_pool_base_, bases.data(), bases.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	for (int r = 0; r < 2; ++r) BM_HIP(hipMemset(d_load_count_[r], 0, sizeof(uint32_t)));
	rebuilt(false);
	return 0;
}

int Residency::preload_all(hipStream_t load_stream) {
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	const WorldDims& d = world_->dims;
	std::vector<uint32_t> words(static_cast<size_t>(d.supercells) * kCellsPerSupercell);
	std::vector<uint32_t> bases(d.supercells, 0u);
	// "all bricks pre-loaded" (BASELINE configs 1-2): every pool is its supercell's full host brick vector (PoolBook::adopt_exact), and the device
	// words are the host words (slot | loaded | lod, Scene.cpp:104)
	uint64_t total_bricks = 0;
	for (int i = 0; i < d.supercells; ++i) total_bricks += world_->supercells[i].bricks.size();
	if (int e = arena_fit(total_bricks)) return e;
	begin_adopt();
	for (int i = 0; i < d.supercells; ++i) {
		const HostSupercell& c = world_->supercells[i];
		bases[i] = arena_.claim_top(c.bricks.size());
		adopt(i, bases[i]);
		std::memcpy(&words[static_cast<size_t>(i) * kCellsPerSupercell], c.indices.data(), kCellsPerSupercell * sizeof(uint32_t));
		if (!c.bricks.empty())
			BM_HIP(hipMemcpy(arena_.base() + static_cast<size_t>(bases[i]) * kBrickWords, c.bricks.data(), c.bricks.size() * sizeof(Brick), hipMemcpyHostToDevice));
	}
	BM_HIP(hipMemcpy(d_pool_base_, bases.data(), bases.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	BM_HIP(hipMemcpyAsync(d_index_grid_, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, load_stream));
	if (int e = clear_ring_counts(load_stream)) return e;
	BM_HIP(hipStreamSynchronize(load_stream));
	rebuilt(true);
	return 0;
}

void Residency::adopted(uint64_t total_bricks) {
	arena_.claim_top(total_bricks);
	rebuilt(true);
}

void Residency::rebuilt(bool preloaded) {
	book_.rebuilt(preloaded);
	use_ring(0);
	snapshot_.clear();
}

int Residency::clear_ring_counts(hipStream_t stream) {
	for (int r = 0; r < 2; ++r) BM_HIP(hipMemsetAsync(d_load_count_[r], 0, sizeof(uint32_t), stream));
	return 0;
}

// ---------------------------------------------------------------- streaming
// Stage the first `count` requests of a ring (positions already in its pinned mirror), copy them up and scatter
// them into the arena / index grid on the load stream (Scene.cpp:215-229 + the upload kernel, kernel.cu:141-151,412-413).
// Which entries count, which slots they get and which pools grow: PoolBook::check_ring / ring_slots.
int Residency::service_ring(int ring, uint32_t count, FrameOrder& order, hipStream_t load_stream, uint32_t* serviced) {
	const auto t_host0 = std::chrono::steady_clock::now();
	const WorldDims& d = world_->dims;
	int* pos = h_positions_[ring];
	// (the positions come back from device memory: never index host arrays with an entry that cannot be a request)
	auto lookup = [&](int px, int py, int pz, int* sci, uint32_t* word, size_t* host_slots) {
		if (px < 0 || py < 0 || pz < 0 || px >= d.cells || py >= d.cells || pz >= d.cells_height) return false;
		*sci = d.supercell_id(px / kSupercell, py / kSupercell, pz / kSupercell);
		const HostSupercell& c = world_->supercells[*sci];
		*word = c.indices[cell_local_index(px, py, pz)];
		*host_slots = c.bricks.size();
		return true;
	};
	if (int e = said(book_.check_ring(pos, count, lookup))) return e;
	if (int e = order.wait_upload_on_host()) return e; // the staging buffers of the previous upload are free again once its copies have run
	uint32_t kept = 0;
	book_.begin_batch();
	auto staged = [&](uint32_t i, int sci, uint32_t host_word, uint32_t device_word) {
		std::memcpy(h_bricks_ + static_cast<size_t>(i) * kBrickWords, world_->supercells[sci].bricks[host_word & BM_BRICK_INDEX_BITS].data, sizeof(Brick));
		h_indices_[i] = device_word;
	};
	if (int e = said(book_.ring_slots(pos, count, lookup, region_alloc(), staged, &kept))) return e;
	const uint32_t n_moves = static_cast<uint32_t>(book_.moves().size());
	if (n_moves > 0) std::memcpy(h_moves_, book_.moves().data(), n_moves * sizeof(PoolMove));
	const bool compacted = kept != count; // stale entries were dropped: the scatter reads the kept positions from d_positions_
	auto queue = [&]() -> int {
		BM_HIP(hipMemcpyAsync(d_bricks_queue_, h_bricks_, static_cast<size_t>(kept) * sizeof(Brick), hipMemcpyHostToDevice, load_stream));    // :228
		BM_HIP(hipMemcpyAsync(d_indices_queue_, h_indices_, static_cast<size_t>(kept) * sizeof(uint32_t), hipMemcpyHostToDevice, load_stream)); // :229
		if (compacted) BM_HIP(hipMemcpyAsync(d_positions_, pos, static_cast<size_t>(kept) * 3 * sizeof(int), hipMemcpyHostToDevice, load_stream));
		// The scatter kernel rewrites index words that a frame still in flight may be reading and requesting through
		// (plain load + atomicOr): a word flipping to "loaded" between the two would be requested a second time; the move
		// kernel rewrites pool bases such a frame addresses bricks with.  In overlapped mode both therefore run behind every
		// frame in flight, whatever stream it is on; the copies above already overlap them.
		if (book_.overlapped()) { if (int e = order.load_behind_frames()) return e; }
		DeviceScene ring_view = *view_;
		ring_view.load_queue = compacted ? d_positions_.get() : d_load_queue_[ring].get();
		ring_view.load_queue_count = d_load_count_[ring];
		if (n_moves > 0) { // grown pools: copy their bricks to the new regions and publish the new bases, ahead of the scatter
			BM_HIP(hipMemcpyAsync(d_moves_, h_moves_, static_cast<size_t>(n_moves) * sizeof(PoolMove), hipMemcpyHostToDevice, load_stream));
			launch_pool_moves(d_moves_, n_moves, arena_.base(), d_pool_base_, load_stream);
			BM_HIP(hipGetLastError());
		}
		launch_upload(ring_view, d_bricks_queue_, d_indices_queue_, arena_.base(), kept, load_stream); // kernel.cu:412
		BM_HIP(hipGetLastError());
		BM_HIP(hipMemsetAsync(d_load_count_[ring], 0, sizeof(uint32_t), load_stream));              // kernel.cu:413
		return order.published(true);
	};
	if (int e = book_.report(queue())) return e; // the host bookkeeping is ahead of the device: refuse to go on
	book_.commit_batch();
	if (serviced) *serviced = kept;
	book_.batch_streamed(static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_host0).count()));
	return 0;
}

int Residency::process_load_queue(FrameOrder& order, hipStream_t load_stream, uint32_t* serviced) {
	const PoolBook::QueueStep step = book_.queue_step();
	if (!book_.overlapped()) {
		// ---- reference order (main.cpp:142-144): the frames that raised the requests have finished (kernel.cu:431), the host
		// reads the ring, stages, uploads; the next frame sees the bricks
		const int ring = step.service;
		if (int e = order.wait_frames_on_host()) return e; // every stream a frame was issued on
		BM_HIP(hipMemcpyAsync(h_count_[ring], d_load_count_[ring], sizeof(uint32_t), hipMemcpyDeviceToHost, load_stream)); // Scene.cpp:202
		BM_HIP(hipStreamSynchronize(load_stream));
		const uint32_t count = std::min<uint32_t>(static_cast<uint32_t>(queue_cap_), *h_count_[ring]);                    // Scene.cpp:203
		if (count == 0) return 0;
		BM_HIP(hipMemcpyAsync(h_positions_[ring], d_load_queue_[ring], static_cast<size_t>(count) * 3 * sizeof(int), hipMemcpyDeviceToHost, load_stream)); // :209
		BM_HIP(hipStreamSynchronize(load_stream));
		return service_ring(ring, count, order, load_stream, serviced);
	}
	// ---- overlapped mode: never wait for the GPU.  (1) service the ring that was copied out by the previous call,
	// (2) start copying out the ring the last frame wrote, behind that frame, on the load stream, (3) hand the other
	// ring to the next frame.  A brick requested in frame k is resident from frame k+2 on (reference order: from k+1 on).
	if (step.service >= 0) {
		if (int e = snapshot_.wait()) return e;
		book_.snapshot_read();
		const uint32_t count = std::min<uint32_t>(static_cast<uint32_t>(queue_cap_), *h_count_[step.service]);
		if (count > 0) {
			if (int e = service_ring(step.service, count, order, load_stream, serviced)) return e;
		}
	}
	if (int e = order.load_behind_frames()) return e; // the ring is complete once every frame that may append to it has ended
	const int ring = step.snapshot;
	// the count is not known on the host without waiting for the frame: a small kernel copies count + the entries that exist into
	// the pinned (device-mapped) mirrors -- min(count, capacity) x 12 bytes over PCIe instead of the ring's whole capacity
	{
		int* dev_positions = nullptr;
		uint32_t* dev_count = nullptr;
		BM_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&dev_positions), h_positions_[ring], 0));
		BM_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&dev_count), h_count_[ring], 0));
		launch_snapshot_ring(d_load_queue_[ring], d_load_count_[ring], dev_positions, dev_count, static_cast<uint32_t>(queue_cap_), load_stream);
		BM_HIP(hipGetLastError());
	}
	if (int e = snapshot_.pass(load_stream)) return e;
	book_.snapshot_taken();
	use_ring(book_.ring());
	return 0;
}

int Residency::rebind(int sci, const std::vector<uint32_t>& old_words, const uint8_t* touched) {
	const HostSupercell& c = world_->supercells[sci];
	return said(book_.rebind(sci, old_words.data(), c.indices.data(), touched, c.bricks.size(), region_alloc()));
}

// ---------------------------------------------------------------- readbacks
int Residency::dump(const char* path) { // Scene.cpp:254-258
	std::ofstream file(path ? path : "dump.txt");
	if (!file) { set_error("cannot open dump file"); return BM_EINVAL; }
	for (size_t i = 0; i < world_->supercells.size(); ++i) file << (static_cast<int>(i) < book_.pools() ? book_.pool(static_cast<int>(i)).high : 0u) << "\n";
	return 0;
}

void Residency::info(bool on_device, bm_scene_info* out) const {
	out->queue_capacity = queue_cap_;
	out->resident_bricks = book_.resident_bricks();
	out->index_bytes = on_device ? static_cast<uint64_t>(world_->dims.supercells) * kCellsPerSupercell * 4 : 0;
	out->brick_bytes = on_device ? arena_.capacity() * 64 : 0;
	out->pool_bytes = on_device ? arena_.pool_bricks() * 64 : 0;
	out->arena_growths = arena_.growths();
	out->arena_copy_growths = arena_.copy_growths();
	out->arena_virtual = arena_.is_virtual() ? 1 : 0;
	out->failed = book_.failed() ? 1 : 0;
	out->stream_batches = book_.stream_batches();
	out->stream_host_ns = book_.stream_host_ns();
}

int Residency::device_indices(int supercell, uint32_t* out4096) {
	if (supercell < 0 || supercell >= world_->dims.supercells || !out4096) { set_error("bad supercell"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	BM_HIP(hipMemcpy(out4096, d_index_grid_ + static_cast<size_t>(supercell) * kCellsPerSupercell, kCellsPerSupercell * 4, hipMemcpyDeviceToHost));
	return 0;
}

int Residency::device_brick(int supercell, uint32_t device_slot, uint32_t* out16) {
	if (supercell < 0 || supercell >= world_->dims.supercells || !out16 || device_slot >= book_.pool(supercell).high) {
		set_error("bad supercell or slot");
		return BM_EINVAL;
	}
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	BM_HIP(hipMemcpy(out16, arena_.base() + (static_cast<size_t>(book_.pool(supercell).base) + device_slot) * kBrickWords, sizeof(Brick), hipMemcpyDeviceToHost));
	return 0;
}

} // namespace bm
