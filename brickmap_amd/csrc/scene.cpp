// scene.cpp -- one GPU's scene: the world on the device, region reads, labels, queries and frame launch (residency and streaming: residency.cpp; edits and region writes: world_changes.cpp).
#include "scene.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "buffer_checks.h"
#include "label.h"

namespace bm {

// ---------------------------------------------------------------- errors
static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
const char* last_error() { return g_error.c_str(); }
int hip_fail(hipError_t e, const char* what, const char* file, int line) {
	// the reference prints "cuda_assert: <string> <file> <line>" and exits (assert_cuda.cpp:3-13);
	// the C-ABI reports instead and lets the caller decide.
	char buf[512];
	std::snprintf(buf, sizeof buf, "hip_assert: %s (%s) %s %d", hipGetErrorString(e), what, file, line);
	set_error(buf);
	return static_cast<int>(e);
}

// ---------------------------------------------------------------- lifetime
Scene::~Scene() {
	hipSetDevice(device_); // the members free themselves on it (scene.h: the arena synchronises before it unmaps, the streams go last)
}

int Scene::require_on_device() const {
	if (!on_device_) { set_error("scene not generated"); return BM_ESTATE; }
	return 0;
}

int Scene::require_not_failed() const {
	if (residency_.book().failed()) { set_error(PoolBook::kFailedWhy); return BM_ESTATE; }
	return 0;
}

int Scene::init(int grid_size, int grid_height) {
	if (!world.dims.set(grid_size, grid_height)) {
		set_error("grid_size and grid_height must be positive multiples of 128 voxels");
		return BM_EINVAL;
	}
	if (world.dims.cells > 1024 || world.dims.cells_height > 1024) { // candidates take 24-bit products of brick coordinates and of their distance to the camera (traverse.h)
		set_error("world too large: at most 8192 voxels along an axis (and see the cube-field limit: cubic worlds up to 5760 voxels a side)");
		return BM_EINVAL;
	}
	// the walk keeps a ray's cell as ONE 32-bit byte offset into the 8 planes of the octant cube field, whose rows are padded to a
	// power of two (traverse.h cell_offset; walk_fields.h lays it out): 8 x (cells_h + 2) x (cells + 2) x 2^shift bytes < 4 GiB
	if (!WalkFields::layout(world.dims).fits) { // (the slice-pitch limit cannot be what fails here: cells <= 1024 above)
		set_error("world too large: the octant cube field (8 planes of (cells_h + 2) x (cells + 2) rows padded to a power of two) must stay below 4 GiB -- cubic worlds up to 5760 voxels a side");
		return BM_EINVAL;
	}
	BM_HIP(hipSetDevice(device_));
	if (int e = load_stream_.create(hipStreamNonBlocking)) return e;
	for (int i = 0; i < kTimingRing; ++i) {
		if (int e = ev_start_[i].create()) return e;
		if (int e = ev_stop_[i].create()) return e;
	}
	if (int e = order_.init(load_stream_)) return e;
	if (int e = changes_.init()) return e;
	if (int e = residency_.init(&view_)) return e;
	if (int e = d_counters_.alloc(sizeof(DeviceCounters))) return e;
	BM_HIP(hipMemset(d_counters_, 0, sizeof(DeviceCounters)));
	if (int e = d_work_counter_.alloc(kWorkCounterBytes * kFrameRing)) return e; // one block of counters per frame in flight
	if (int e = d_frame_constants_.alloc(kFrameRing * sizeof(FrameConstants))) return e;
	if (int e = h_frame_constants_.alloc(kFrameRing * sizeof(FrameConstants))) return e;
	hipDeviceProp_t prop;
	BM_HIP(hipGetDeviceProperties(&prop, device_));
	compute_units_ = prop.multiProcessorCount; // main.cpp:97 sm_cores
	blocks_per_cu_[0] = blocks_per_cu_[1] = 0; // no cap: every instantiation of the fused kernel runs at its own occupancy (trace.hip launch_trace)
	if (tuning().blocks_per_cu > 0) blocks_per_cu_[0] = tuning().blocks_per_cu; // experiment knob: fewer resident waves per SIMD (1 block = 1 wave per SIMD)

	return residency_.alloc_queue();
}

void Scene::residency_rebuilt() {
	fields_.book().residency_rebuilt();
	order_.residency_rebuilt();
}

int Scene::set_streaming_mode(int overlapped) { return residency_.set_streaming_mode(overlapped, order_, load_stream_); }

int Scene::set_lod(int lod8, int lod2) {
	lod8_ = lod8;
	lod2_ = lod2;
	view_.lod_distance_8x8x8 = lod8;
	view_.lod_distance_2x2x2 = lod2;
	return 0;
}

int Scene::set_queue_capacity(int cap) {
	if (cap <= 0) { set_error("queue capacity must be positive"); return BM_EINVAL; }
	// resizing the ring drops what it holds while the REQUESTED bits of those bricks stay set (they would never be asked
	// for again): the capacity belongs to the scene's construction, like the reference's constexpr (variables.h:35)
	if (on_device_) { set_error("set the queue capacity before bm_scene_generate"); return BM_ESTATE; }
	return residency_.set_queue_capacity(cap);
}

void Scene::free_device() {
	residency_.release();
	fields_.release();
	on_device_ = false;
}

// device half of Scene::generate (Scene.cpp:152-190): one flat index grid, one pool-base word per supercell and one
// brick arena instead of 2 x supercells cudaMallocs and two pointer tables; plus the octant cube field of the walk.
int Scene::allocate_device() {
	BM_HIP(hipSetDevice(device_));
	free_device();
	const WorldDims& d = world.dims;
	uint64_t run = 0;
	for (int i = 0; i < d.supercells; ++i) run += world.supercells[i].bricks.size();
	if (run >= (1ull << 32)) { set_error("world has more than 2^32 bricks"); return BM_EINVAL; }
	if (int e = residency_.alloc_index_grid()) return e;
	if (int e = residency_.open_arena(run)) return e;
	if (int e = fields_.allocate(d, &view_)) return e;
	{ // the host builds the field with tight rows (world.cpp) and every slice is copied row by row
		std::vector<uint8_t> field;
		world.build_cube_field(field, 8);
		if (int e = fields_.upload(field.data())) return e;
	}
	set_view_dims();
	on_device_ = true;
	if (int e = reset_residency()) return e;
	// the escape heights alone (the field is the host's), from the index words reset_residency has just written: which words are non-zero never changes with residency
	if (int e = fields_.update(residency_.index_grid(), FieldChange::whole(d), false, load_stream_)) return e;
	BM_HIP(hipStreamSynchronize(load_stream_));
	return 0;
}

void Scene::set_view_dims() {
	const WorldDims& d = world.dims;
	view_.cells = d.cells;
	view_.cells_height = d.cells_height;
	view_.sg_xy = d.supergrid_xy;
	view_.sg_xy2 = d.supergrid_xy * d.supergrid_xy;
	view_.grid_size_f = static_cast<float>(d.grid_size);
	view_.grid_height_f = static_cast<float>(d.grid_height);
	view_.lod_distance_8x8x8 = lod8_;
	view_.lod_distance_2x2x2 = lod2_;
}

int Scene::generate(int threads) {
	world.generate(threads);
	return allocate_device();
}

int Scene::generate_supercell(int sx, int sy, int sz) {
	const WorldDims& d = world.dims;
	if (sx < 0 || sy < 0 || sz < 0 || sx >= d.supergrid_xy || sy >= d.supergrid_xy || sz >= d.supergrid_z) {
		set_error("supercell coordinates out of range");
		return BM_EINVAL;
	}
	// Once the world is on the device its pools hold bricks in request order and the index words name those slots:
	// rebuilding a host supercell would reset its slot counter under them (the regenerated content is identical anyway --
	// the terrain is a pure function of the coordinates).  The reference never calls it after generate() either.
	if (on_device_) { set_error("bm_scene_generate_supercell: the scene is on the device (call it before bm_scene_generate)"); return BM_ESTATE; }
	world.generate_supercell(sx, sy, sz);
	return 0;
}

int Scene::reset_residency() {
	if (int e = require_on_device()) return e;
	if (int e = residency_.reset()) return e;
	residency_rebuilt();
	return 0;
}

int Scene::preload_all() {
	if (int e = require_on_device()) return e;
	if (int e = residency_.preload_all(load_stream_)) return e;
	residency_rebuilt();
	return 0;
}

// ---------------------------------------------------------------- dense voxels -> scene (bm_scene_load_voxels)
// The canonical build of a dense volume (world.h load_voxels), on the device in the preloaded state.  Host memory: World::load_voxels
// on CPU threads, then the generate route's allocate_device + preload_all.  Device memory: load.hip packs the volume where it lies --
// classify and number fill the index grid and the pool bases, the brick total comes back to size the arena exactly, pack writes the
// bricks, the cube-field passes of edit.hip run over the whole grid, and words and bricks are copied back into the host world, which
// ends up the object the host route builds.  Everything runs on the load stream behind the work queued on the caller's stream.
int Scene::load_voxels(const uint8_t* voxels, size_t bytes, int where, hipStream_t stream) {
	const WorldDims& d = world.dims;
	const size_t need = static_cast<size_t>(d.grid_size) * d.grid_size * d.grid_height;
	if (!voxels) { set_error("bm_scene_load_voxels: null volume"); return BM_EINVAL; }
	if (bytes != need) { set_error("bm_scene_load_voxels: the volume must hold grid_size^2 * grid_height bytes (" + std::to_string(need) + ")"); return BM_EINVAL; }
	if (where != BM_VOXELS_HOST && where != BM_VOXELS_DEVICE) { set_error("bm_scene_load_voxels: `where` is BM_VOXELS_HOST or BM_VOXELS_DEVICE"); return BM_EINVAL; }
	if (static_cast<uint64_t>(d.supercells) * kCellsPerSupercell >= (1ull << 32)) { set_error("world has more than 2^32 bricks"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device_));
	if (where == BM_VOXELS_DEVICE) { // the kernels read [voxels, voxels + bytes): it has to be memory of this device, all of it
		if (!device_span_ok(device_, voxels, bytes)) {
			set_error("bm_scene_load_voxels: BM_VOXELS_DEVICE needs `bytes` bytes of memory of the scene's device");
			return BM_EINVAL;
		}
	}
	BM_HIP(hipDeviceSynchronize()); // no frame, edit or upload in flight from here on: the old world (if any) can go
	load_clocked_ = 0;
	if (where == BM_VOXELS_HOST) {
		world.load_voxels(voxels, 16);
		if (int e = allocate_device()) return e;
		return preload_all();
	}
	const int e = load_voxels_device(voxels, stream);
	if (e) { // no half-built world: the scene is back to "created"
		(void)hipDeviceSynchronize();
		free_device();
		world.supercells.clear();
		world.generated = false;
	}
	return e;
}

int Scene::load_voxels_device(const uint8_t* voxels, hipStream_t stream) {
	const WorldDims& d = world.dims;
	free_device();
	world.generated = false;
	if (int e = load_marks_.create()) return e;
	hipEvent_t* const marks = load_marks_.marks();
	if (int e = residency_.alloc_index_grid()) return e;
	if (int e = fields_.allocate(d, &view_)) return e;
	set_view_dims();
	LoadDims ld{static_cast<uint32_t>(d.grid_size), static_cast<uint32_t>(d.supergrid_xy), static_cast<uint32_t>(d.supergrid_xy * d.supergrid_xy),
				static_cast<uint32_t>(d.supercells)};
	// temporaries: one count per supercell + the 64-bit total; the intermediate planes of the field passes
	DeviceBuffer<uint32_t> counts;
	if (int e = counts.alloc((static_cast<size_t>(d.supercells) + 2) * sizeof(uint32_t))) return e;
	uint32_t* d_total = counts + d.supercells;
	// the field comes from the update of edit.hip with the box = every cell, into the field the allocation set to 255
	const FieldChange all = FieldChange::whole(d);
	if (int e = fields_.prepare_update(all, nullptr)) return e; // (load_voxels has synchronised the device: no stream to wait for, unlike a change batch)
	if (int e = order_.load_behind_caller(stream)) return e; // the volume is whatever the caller's stream has written by now
	// ---- classify + number
	uint32_t* const index_grid = residency_.index_grid();
	uint32_t* const pool_base = residency_.pool_base();
	BM_HIP(hipEventRecord(marks[0], load_stream_));
	launch_load_classify(voxels, index_grid, ld, load_stream_);
	BM_HIP(hipGetLastError());
	launch_load_number(index_grid, counts, pool_base, d_total, ld, load_stream_);
	BM_HIP(hipGetLastError());
	BM_HIP(hipEventRecord(marks[1], load_stream_));
	uint32_t total_words[2] = {0, 0};
	BM_HIP(hipMemcpyAsync(total_words, d_total, sizeof total_words, hipMemcpyDeviceToHost, load_stream_));
	BM_HIP(hipStreamSynchronize(load_stream_)); // the one host round trip: the arena is sized by what the volume holds
	const uint64_t total = total_words[0] | (static_cast<uint64_t>(total_words[1]) << 32);
	if (total >= (1ull << 32)) { set_error("world has more than 2^32 bricks"); return BM_EINVAL; }
	if (int e = residency_.open_arena(total)) return e;
	if (int e = residency_.arena_fit(total)) return e;
	// ---- pack
	BM_HIP(hipEventRecord(marks[2], load_stream_));
	launch_load_pack(voxels, index_grid, pool_base, residency_.arena_base(), ld, load_stream_);
	BM_HIP(hipGetLastError());
	BM_HIP(hipEventRecord(marks[3], load_stream_));
	// ---- field
	if (int e = fields_.update(index_grid, all, true, load_stream_)) return e;
	BM_HIP(hipEventRecord(marks[4], load_stream_));
	// ---- mirror: the host world becomes what World::load_voxels builds, in the state preload_all leaves it in
	std::vector<uint32_t> words(static_cast<size_t>(d.supercells) * kCellsPerSupercell), bases(d.supercells);
	std::vector<Brick> bricks(total);
	BM_HIP(hipMemcpyAsync(words.data(), index_grid, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, load_stream_));
	BM_HIP(hipMemcpyAsync(bases.data(), pool_base, bases.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, load_stream_));
	if (total) BM_HIP(hipMemcpyAsync(bricks.data(), residency_.arena_base(), total * sizeof(Brick), hipMemcpyDeviceToHost, load_stream_));
	if (int e = residency_.clear_ring_counts(load_stream_)) return e;
	BM_HIP(hipEventRecord(marks[5], load_stream_));
	BM_HIP(hipStreamSynchronize(load_stream_));
	world.supercells.clear();
	world.supercells.resize(d.supercells);
	residency_.begin_adopt();
	parallel_for(d.supercells, 16, [&](int i) {
		HostSupercell& c = world.supercells[i];
		const uint32_t* w = &words[static_cast<size_t>(i) * kCellsPerSupercell];
		const uint64_t end = i + 1 < d.supercells ? bases[i + 1] : total;
		c.indices.assign(w, w + kCellsPerSupercell);
		c.bricks.assign(bricks.begin() + bases[i], bricks.begin() + static_cast<ptrdiff_t>(end));
		residency_.adopt(i, bases[i]);
	});
	world.generated = true;
	residency_.adopted(total);
	on_device_ = true;
	residency_rebuilt();
	load_clocked_ = kClockedCall;
	return 0;
}

int Scene::last_load_ms(float* pack_ms, float* field_ms, float* mirror_ms) {
	if (!pack_ms || !field_ms || !mirror_ms) { set_error("null argument"); return BM_EINVAL; }
	if (!load_clocked_) { set_error("no volume has been loaded from device memory yet"); return BM_ESTATE; }
	BM_HIP(hipSetDevice(device_));
	float classify = 0.f, rest[3];
	if (int e = load_marks_.read(1, &classify)) return e;
	if (int e = load_marks_.read(3, rest, 2)) return e;
	*pack_ms = classify + rest[0]; // without the host's round trip between them (the arena is mapped there)
	*field_ms = rest[1];
	*mirror_ms = rest[2];
	return 0;
}

int Scene::host_voxels(uint8_t* dst, size_t capacity, size_t* bytes) {
	const WorldDims& d = world.dims;
	const size_t need = static_cast<size_t>(d.grid_size) * d.grid_size * d.grid_height;
	if (bytes) *bytes = need;
	if (!dst) return 0;
	if (!world.generated) { set_error("world not generated"); return BM_ESTATE; }
	if (capacity < need) { set_error("voxel buffer too small"); return BM_EINVAL; }
	world.store_voxels(dst, 16);
	return 0;
}

// ---------------------------------------------------------------- streaming and readbacks: residency.cpp
int Scene::process_load_queue(uint32_t* serviced) {
	if (serviced) *serviced = 0;
	if (int e = require_on_device()) return e;
	if (int e = require_not_failed()) return e;
	BM_HIP(hipSetDevice(device_));
	return residency_.process_load_queue(order_, load_stream_, serviced);
}

int Scene::dump(const char* path) { return residency_.dump(path); }

int Scene::info(bm_scene_info* out) {
	if (!out) { set_error("null argument"); return BM_EINVAL; }
	const WorldDims& d = world.dims;
	std::memset(out, 0, sizeof *out);
	out->grid_size = d.grid_size; out->grid_height = d.grid_height;
	out->supergrid_xy = d.supergrid_xy; out->supergrid_z = d.supergrid_z; out->supercells = d.supercells;
	out->lod_distance_8x8x8 = lod8_; out->lod_distance_2x2x2 = lod2_;
	out->generated = world.generated ? 1 : 0;
	out->on_device = on_device_ ? 1 : 0;
	out->total_bricks = world.generated ? world.total_bricks() : 0;
	out->cube_field_bytes = on_device_ ? fields_.cube_field_bytes() : 0;
	out->escape_bytes = on_device_ ? fields_.escape_bytes() : 0;
	out->sun_plane_bytes = on_device_ ? fields_.sun_plane_bytes() : 0;
	residency_.info(on_device_, out);
	return 0;
}

int Scene::device_indices(int supercell, uint32_t* out4096) {
	if (int e = require_on_device()) return e;
	return residency_.device_indices(supercell, out4096);
}

int Scene::device_brick(int supercell, uint32_t device_slot, uint32_t* out16) {
	if (int e = require_on_device()) return e;
	return residency_.device_brick(supercell, device_slot, out16);
}

// ---------------------------------------------------------------- voxel edits and region writes: world_changes.cpp
int Scene::edit(int count, const bm_edit* edits, hipStream_t stream) {
	std::string why;
	if (!World::validate_edits(edits, count, &why)) { set_error("bm_scene_edit: " + why); return BM_EINVAL; }
	if (!on_device_) { set_error("bm_scene_edit: scene not generated"); return BM_ESTATE; }
	if (int e = require_not_failed()) return e;
	return changes_.edit(count, edits, stream);
}

int Scene::last_edit_ms(float* scatter_ms, float* field_ms) { return changes_.last_edit_ms(scatter_ms, field_ms); }

// ---------------------------------------------------------------- dense regions (bm_scene_write_region / bm_scene_read_region)
namespace {
// the parts of the box [blo, bhi) that lie outside its clipped part [lo, hi) (all of it when `inside` is false), as up to six boxes
template <class F> void for_outside_slabs(const int32_t blo[3], const int32_t bhi[3], bool inside, const int lo[3], const int hi[3], F f) {
	if (!inside) { f(blo[0], bhi[0], blo[1], bhi[1], blo[2], bhi[2]); return; }
	if (blo[2] < lo[2]) f(blo[0], bhi[0], blo[1], bhi[1], blo[2], lo[2]);
	if (hi[2] < bhi[2]) f(blo[0], bhi[0], blo[1], bhi[1], hi[2], bhi[2]);
	if (blo[1] < lo[1]) f(blo[0], bhi[0], blo[1], lo[1], lo[2], hi[2]);
	if (hi[1] < bhi[1]) f(blo[0], bhi[0], hi[1], bhi[1], lo[2], hi[2]);
	if (blo[0] < lo[0]) f(blo[0], lo[0], lo[1], hi[1], lo[2], hi[2]);
	if (hi[0] < bhi[0]) f(hi[0], bhi[0], lo[1], hi[1], lo[2], hi[2]);
}
int64_t region_offset(const bm_region& r, int64_t x, int64_t y, int64_t z) { return (z - r.lo[2]) * r.slice_pitch + (y - r.lo[1]) * r.row_pitch + (x - r.lo[0]); }
} // namespace

// what write_region and read_region refuse, before anything changes; *r gets its pitches filled in, *span the bytes of the volume
int Scene::check_region(const char* who, const bm_region* region, const void* voxels, int where, bm_region* r, uint64_t* span) {
	const std::string at = std::string(who) + ": ";
	if (!region || !voxels) { set_error(at + "null region or volume"); return BM_EINVAL; }
	*r = *region;
	std::string why;
	if (!World::validate_region(r, &why, span)) { set_error(at + why); return BM_EINVAL; }
	if (where != BM_VOXELS_HOST && where != BM_VOXELS_DEVICE) { set_error(at + "`where` is BM_VOXELS_HOST or BM_VOXELS_DEVICE"); return BM_EINVAL; }
	if (!on_device_) { set_error(at + "scene not generated"); return BM_ESTATE; }
	if (int e = require_not_failed()) return e;
	BM_HIP(hipSetDevice(device_));
	if (where == BM_VOXELS_DEVICE && *span > 0 && !device_span_ok(device_, voxels, *span)) {
		set_error(at + "BM_VOXELS_DEVICE needs the volume's whole span inside one allocation of the scene's device");
		return BM_EINVAL;
	}
	return 0;
}

int Scene::write_region(const bm_region* region, int op, const uint8_t* voxels, int where, hipStream_t stream) {
	bm_region r;
	uint64_t span = 0;
	if (op != BM_REGION_REPLACE && op != BM_EDIT_SET && op != BM_EDIT_CLEAR) { set_error("bm_scene_write_region: unknown op"); return BM_EINVAL; }
	if (int e = check_region("bm_scene_write_region", region, voxels, where, &r, &span)) return e;
	return changes_.write_region(r, op, voxels, where, stream);
}

int Scene::last_region_ms(float* pack_ms, float* copy_ms, float* scatter_ms, float* field_ms) { return changes_.last_region_ms(pack_ms, copy_ms, scatter_ms, field_ms); }

int Scene::stage_absent_bricks(bool inside, const int lo[3], const int hi[3], size_t* count, size_t* bricks_at, size_t* total) {
	const WorldDims& d = world.dims;
	std::vector<int> cells;
	std::vector<Brick> bricks;
	if (inside && !residency_.book().preloaded())
		for (int cz = lo[2] >> 3; cz <= (hi[2] - 1) >> 3; ++cz)
			for (int cy = lo[1] >> 3; cy <= (hi[1] - 1) >> 3; ++cy)
				for (int cx = lo[0] >> 3; cx <= (hi[0] - 1) >> 3; ++cx) {
					const int sci = d.supercell_id(cx / kSupercell, cy / kSupercell, cz / kSupercell);
					const HostSupercell& c = world.supercells[sci];
					const uint32_t word = c.indices[cell_local_index(cx, cy, cz)];
					if (!residency_.book().absent(sci, word)) continue;
					cells.insert(cells.end(), {cx, cy, cz});
					bricks.push_back(c.bricks[word & BM_BRICK_INDEX_BITS]);
				}
	const size_t n = bricks.size(), o_bricks = (n * 3 * sizeof(int) + 63) / 64 * 64, bytes = o_bricks + n * sizeof(Brick);
	if (n > 0) {
		if (int e = region_read_.wait()) return e; // the previous read's list has been used
		if (int e = h_patch_.reserve(std::max<size_t>(bytes, 1 << 16))) return e;
		if (int e = d_patch_.reserve(std::max<size_t>(bytes, 1 << 16))) return e;
		std::memcpy(h_patch_, cells.data(), n * 3 * sizeof(int));
		std::memcpy(h_patch_ + o_bricks, bricks.data(), n * sizeof(Brick));
	}
	*count = n; *bricks_at = o_bricks; *total = bytes;
	return 0;
}

// The host world is authoritative, so a host read is World::store_region.  A device read is issued like a query: the unpack kernel reads
// the device words and bricks; bricks that are not resident (a streaming scene) are staged from the host world and written by a second
// small launch; what lies outside the world is zeroed.
int Scene::read_region(const bm_region* region, uint8_t* voxels, int where, hipStream_t stream) {
	bm_region r;
	uint64_t span = 0;
	if (int e = check_region("bm_scene_read_region", region, voxels, where, &r, &span)) return e;
	if (span == 0) return 0;
	const WorldDims& d = world.dims;
	int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
	const bool inside = World::region_bounds(d, r, lo, hi);
	if (where == BM_VOXELS_HOST) {
		for_outside_slabs(r.lo, r.hi, inside, lo, hi, [&](int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1) {
			for (int64_t z = z0; z < z1; ++z)
				for (int64_t y = y0; y < y1; ++y) std::memset(voxels + region_offset(r, x0, y, z), 0, static_cast<size_t>(x1 - x0));
		});
		if (inside) world.store_region(lo, hi, r.lo, voxels, r.row_pitch, r.slice_pitch, 16);
		return 0;
	}
	size_t n = 0, o_bricks = 0, bytes = 0;
	if (int e = stage_absent_bricks(inside, lo, hi, &n, &o_bricks, &bytes)) return e;
	DeviceScene view;
	if (int e = begin_frame(stream, &view, nullptr)) return e;
	FrameOrder::Ending frame(order_, stream);
	for_outside_slabs(r.lo, r.hi, inside, lo, hi, [&](int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1) {
		launch_region_zero(voxels + region_offset(r, x0, y0, z0), r.row_pitch, r.slice_pitch, x1 - x0, y1 - y0, z1 - z0, stream);
	});
	if (inside) {
		const RegionDims rd = region_dims(d, r, lo, hi);
		launch_region_unpack(voxels, view.index_grid, view.pool_base, view.brick_arena, rd, stream);
		if (n > 0) {
			BM_HIP(hipMemcpyAsync(d_patch_, h_patch_, bytes, hipMemcpyHostToDevice, stream));
			launch_region_patch(voxels, reinterpret_cast<const int*>(d_patch_.get()), reinterpret_cast<const uint32_t*>(d_patch_ + o_bricks), static_cast<uint32_t>(n), rd, stream);
			if (int e = region_read_.pass(stream)) return e;
		}
	}
	BM_HIP(hipGetLastError());
	(void)frame.end();
	return 0;
}

// ---------------------------------------------------------------- connected components (bm_scene_label_region / _components / _mask)
int Scene::check_label_box(const char* who, const int32_t lo[3], const int32_t hi[3], LabelDims* d, bool* empty) {
	const std::string at = std::string(who) + ": ";
	if (!lo || !hi) { set_error(at + "null box"); return BM_EINVAL; }
	int64_t n[3];
	for (int k = 0; k < 3; ++k) {
		n[k] = static_cast<int64_t>(hi[k]) - lo[k];
		if (n[k] < 0) { set_error(at + "hi < lo"); return BM_EINVAL; }
	}
	*empty = n[0] == 0 || n[1] == 0 || n[2] == 0;
	// (64 bits: each factor is below 2^32, so the first product is below 2^63 once n[0] has passed, and the second is formed only below 2^31 * 2^32)
	if (!*empty && (n[0] > kLabelMaxVoxels || n[0] * n[1] > kLabelMaxVoxels || n[0] * n[1] * n[2] > kLabelMaxVoxels)) { set_error(at + "the box holds more than 2^31 - 2 voxels"); return BM_EINVAL; }
	*d = LabelDims{};
	for (int k = 0; k < 3; ++k) d->org[k] = lo[k];
	d->nx = static_cast<uint32_t>(n[0]); d->ny = static_cast<uint32_t>(n[1]); d->nz = static_cast<uint32_t>(n[2]);
	d->sg_xy = static_cast<uint32_t>(world.dims.supergrid_xy);
	d->sg_xy2 = d->sg_xy * d->sg_xy;
	return 0;
}

namespace {
// the box clipped to the world, as World::region_bounds gives it, and the cells it overlaps
bool label_clip(const WorldDims& wd, const int32_t lo[3], const int32_t hi[3], LabelDims* d) {
	bm_region r{};
	for (int k = 0; k < 3; ++k) { r.lo[k] = lo[k]; r.hi[k] = hi[k]; }
	int clo[3] = {0, 0, 0}, chi[3] = {0, 0, 0};
	const bool inside = World::region_bounds(wd, r, clo, chi);
	for (int k = 0; k < 3; ++k) {
		d->lo[k] = inside ? clo[k] : 0;
		d->hi[k] = inside ? chi[k] : 0;
		d->c0[k] = inside ? clo[k] >> 3 : 0;
		d->nc[k] = inside ? ((chi[k] - 1) >> 3) - d->c0[k] + 1 : 0;
	}
	return inside;
}
} // namespace

// Issued like a device read of the same box (read_region): zero what lies outside the world, label the cells the device holds and then
// the staged ones, merge across cell faces, flatten and count.  Only the caller's volume is written.
int Scene::label_region(const int32_t lo[3], const int32_t hi[3], uint32_t flags, int32_t* labels, uint64_t* count, hipStream_t stream) {
	const char* who = "bm_scene_label_region";
	LabelDims ld;
	bool empty = false;
	if (flags != 0) { set_error("bm_scene_label_region: unknown flags (must be 0)"); return BM_EINVAL; }
	if (int e = check_label_box(who, lo, hi, &ld, &empty)) return e;
	if (!count || (!empty && !labels)) { set_error("bm_scene_label_region: null label volume or count"); return BM_EINVAL; }
	if (!aligned(count, 8) || (!empty && !aligned(labels, 4))) {
		set_error("bm_scene_label_region: labels must be 4-byte aligned, count 8-byte aligned");
		return BM_EINVAL;
	}
	if (int e = require_on_device()) return e;
	if (int e = require_not_failed()) return e;
	BM_HIP(hipSetDevice(device_));
	const size_t voxels = static_cast<size_t>(ld.nx) * ld.ny * ld.nz;
	if (!device_span_ok(device_, count, sizeof(uint64_t)) ||
		(!empty && !device_span_ok(device_, labels, voxels * sizeof(int32_t)))) {
		set_error("bm_scene_label_region: the label volume's whole span and the count must lie inside one allocation each of the scene's device");
		return BM_EINVAL;
	}
	const bool inside = !empty && label_clip(world.dims, lo, hi, &ld);
	size_t n = 0, o_bricks = 0, bytes = 0;
	if (int e = stage_absent_bricks(inside, ld.lo, ld.hi, &n, &o_bricks, &bytes)) return e;
	if (int e = label_marks_.create()) return e;
	DeviceScene view;
	if (int e = begin_frame(stream, &view, nullptr)) return e;
	FrameOrder::Ending frame(order_, stream);
	if (int e = label_.order(stream)) return e;
	BM_HIP(hipMemsetAsync(count, 0, sizeof(uint64_t), stream));
	label_clocked_ = 0;
	if (!empty) {
		uint8_t* bytes_out = reinterpret_cast<uint8_t*>(labels);
		const int64_t row = static_cast<int64_t>(ld.nx) * 4, slice = row * ld.ny;
		for_outside_slabs(lo, hi, inside, ld.lo, ld.hi, [&](int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1) {
			launch_region_zero(bytes_out + (z0 - lo[2]) * slice + (y0 - lo[1]) * row + (x0 - lo[0]) * 4, row, slice, (x1 - x0) * 4, y1 - y0, z1 - z0, stream);
		});
		if (inside) {
			if (n > 0) BM_HIP(hipMemcpyAsync(d_patch_, h_patch_, bytes, hipMemcpyHostToDevice, stream));
			launch_label_region(view, reinterpret_cast<uint32_t*>(labels), count, ld, reinterpret_cast<const int*>(d_patch_.get()),
								reinterpret_cast<const uint32_t*>(d_patch_.get() + o_bricks), static_cast<uint32_t>(n), stream, label_marks_.marks());
			label_clocked_ = kClockedCall;
			if (n > 0) { if (int e = region_read_.pass(stream)) return e; }
		}
	}
	BM_HIP(hipGetLastError());
	if (int e = label_.pass(stream)) return e;
	(void)frame.end();
	return 0;
}

int Scene::last_label_ms(float* local_ms, float* merge_ms, float* flatten_ms) {
	if (!local_ms || !merge_ms || !flatten_ms) { set_error("null argument"); return BM_EINVAL; }
	if (!label_clocked_) { set_error("the last bm_scene_label_region launched nothing, or there was none"); return BM_ESTATE; }
	BM_HIP(hipSetDevice(device_));
	float ms[3];
	if (int e = label_marks_.read(3, ms)) return e;
	*local_ms = ms[0]; *merge_ms = ms[1]; *flatten_ms = ms[2];
	return 0;
}

// Reads the label volume alone, so it is not a frame: ordered on its stream, and behind the label call before it (the root counts are
// one buffer, which grows only once that call has finished).
int Scene::label_components(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, bm_component* comps, int64_t capacity, hipStream_t stream) {
	const char* who = "bm_scene_label_components";
	LabelDims ld;
	bool empty = false;
	if (int e = check_label_box(who, lo, hi, &ld, &empty)) return e;
	if (capacity < 0) { set_error("bm_scene_label_components: negative capacity"); return BM_EINVAL; }
	if (empty || capacity == 0) return 0;
	if (!labels || !comps) { set_error("bm_scene_label_components: null label volume or table"); return BM_EINVAL; }
	if (!aligned(labels, 4) || !aligned(comps, 8)) {
		set_error("bm_scene_label_components: labels must be 4-byte aligned, the table 8-byte aligned");
		return BM_EINVAL;
	}
	if (int e = require_on_device()) return e;
	if (int e = require_not_failed()) return e;
	BM_HIP(hipSetDevice(device_));
	const size_t voxels = static_cast<size_t>(ld.nx) * ld.ny * ld.nz;
	const size_t records = static_cast<size_t>(std::min<int64_t>(capacity, static_cast<int64_t>(voxels))); // (no more components than voxels)
	if (!device_span_ok(device_, labels, voxels * sizeof(int32_t)) ||
		!device_span_ok(device_, comps, records * sizeof(bm_component))) {
		set_error("bm_scene_label_components: the label volume and min(capacity, voxels) records must lie inside one allocation each of the scene's device");
		return BM_EINVAL;
	}
	label_clip(world.dims, lo, hi, &ld);
	const size_t need = label_tmp_bytes(static_cast<uint32_t>(voxels));
	if (d_label_tmp_.bytes() < need) {
		if (int e = label_.wait()) return e;
		if (int e = d_label_tmp_.reserve(std::max<size_t>(need, 1 << 16))) return e;
	}
	if (int e = label_.order(stream)) return e;
	launch_label_components(reinterpret_cast<const uint32_t*>(labels), comps, static_cast<uint64_t>(capacity), ld, d_label_tmp_, stream);
	BM_HIP(hipGetLastError());
	return label_.pass(stream);
}

int Scene::label_mask(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, const bm_component* comps, int64_t n, const uint8_t* chosen, uint8_t* mask,
					  hipStream_t stream) {
	const char* who = "bm_scene_label_mask";
	LabelDims ld;
	bool empty = false;
	if (int e = check_label_box(who, lo, hi, &ld, &empty)) return e;
	if (n < 0) { set_error("bm_scene_label_mask: negative record count"); return BM_EINVAL; }
	if (empty) return 0;
	if (!labels || !mask || (n > 0 && (!comps || !chosen))) { set_error("bm_scene_label_mask: null buffer"); return BM_EINVAL; }
	if (!aligned(labels, 4) || !aligned(comps, 8)) {
		set_error("bm_scene_label_mask: labels must be 4-byte aligned, the table 8-byte aligned");
		return BM_EINVAL;
	}
	if (int e = require_on_device()) return e;
	if (int e = require_not_failed()) return e;
	BM_HIP(hipSetDevice(device_));
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

// ---- the sun plane and the view plane (walk_fields.h; field_book.h decides): each is built on the load stream by the production launch that is
// about to read it, unless it stands.  *usable: the launch's frames with the book's key may read the plane.
int Scene::ensure_sun_plane(const FrameConstants& fc, bool* usable) {
	FieldBook::SunStep s = fields_.book().sun_launch(fc.cone_dir, fc.cone_extent, residency_.book().preloaded());
	*usable = s.step == FieldBook::kStands;
	if (s.step != FieldBook::kBuildSlice && s.step != FieldBook::kBuildPlane) return 0;
	bool ready = false;
	if (int e = fields_.prepare(&s, load_stream_, &ready)) return e;
	if (!ready) return 0;
	// behind every frame in flight (their shadow rays read the plane) and, on the load stream, behind the field and escape updates it reads
	if (int e = order_.publish_behind_frames([&] { return fields_.build(s, residency_.index_grid(), residency_.pool_base(), residency_.arena_base(), load_stream_); })) return e;
	*usable = true;
	return 0;
}

int Scene::ensure_view_plane(const std::vector<FrameConstants>& fcs, bool* usable) {
	const FieldBook::ViewStep v = fields_.book().view_launch(fcs, static_cast<int>(fcs.size()));
	*usable = v.step == FieldBook::kStands;
	if (v.step != FieldBook::kBuildPlane) return 0;
	if (int e = order_.publish_behind_frames([&] { return fields_.build(v, load_stream_); })) return e; // (their primary rays read the plane)
	*usable = true;
	return 0;
}

int Scene::host_cube_field(uint8_t* dst, size_t capacity, size_t* bytes) {
	const WorldDims& d = world.dims;
	const size_t need = 8 * WalkFields::tight_plane_bytes(d);
	if (bytes) *bytes = need;
	if (!dst) return 0;
	if (!world.generated) { set_error("world not generated"); return BM_ESTATE; }
	if (capacity < need) { set_error("cube field buffer too small"); return BM_EINVAL; }
	std::vector<uint8_t> f;
	world.build_cube_field(f, 8);
	std::memcpy(dst, f.data(), need);
	return 0;
}

// ---------------------------------------------------------------- frame launch (launch_kernels, kernel.cu:366-439)
int Scene::render(const bm_camera* cam, const bm_frame_params* fp, float* accum, uint32_t* dbg, hipStream_t stream) {
	return render_frames(1, cam, fp, &accum, dbg ? &dbg : nullptr, stream);
}

// `count` consecutive frames -- the reference's per-frame loop (main.cpp:117-147: one launch_kernels call per frame) -- as ONE launch
// of the persistent kernel (trace.hip "FRAME RING"): frame i's constants, ticket counters and buffers are entry first + i of the
// scene's rings, and every wave walks from frame to frame by itself.
int Scene::render_frames(int count, const bm_camera* cams, const bm_frame_params* fps, float* const* accums, uint32_t* const* dbgs, hipStream_t stream) {
	if (int e = require_on_device()) return e;
	LaunchPlan plan; // every decision that needs no device: frame_plan.cpp
	if (int e = plan_launch(count, cams, fps, accums, dbgs, world.dims.cells, world.dims.cells_height, &plan)) return e;
	std::vector<FrameConstants>& fcs = plan.frames;
	const FrameConstants& fc = fcs[0];
	BM_HIP(hipSetDevice(device_));
	// the sun plane, for the first frame's sun: built now if it is not there; frames of the launch with another sun keep their octant planes
	if (!plan.instrumented && !(fc.flags & BM_FLAG_PRIMARY_ONLY) && fc.spp >= 1) {
		bool usable = false;
		if (int e = ensure_sun_plane(fc, &usable)) return e;
		if (usable)
			for (FrameConstants& f : fcs)
				if (std::memcmp(f.cone_dir, fields_.book().sun_key(), 3 * sizeof(float)) == 0 && f.cone_extent == fields_.book().sun_key()[3]) f.shadow_field_off = 8u * view_.cf_plane;
	}
	// the view plane, for the first frame's origin: built now if the camera rests there; frames of the launch from another origin keep their octant planes
	if (BM_VIEWFIELD != 0 && !plan.instrumented) {
		bool usable = false;
		if (int e = ensure_view_plane(fcs, &usable)) return e;
		if (usable)
			for (FrameConstants& f : fcs)
				if (std::memcmp(f.origin, fields_.book().view_key(), sizeof f.origin) == 0 && f.lens_radius == 0.0f) f.view_field_off = 9u * view_.cf_plane;
	}
	// `stream` is used as given: nullptr is HIP's default stream (what the reference's <<<>>> launches use), which is
	// ordered with the caller's other default-stream work (e.g. torch's fill kernels on the accumulation buffer).
	if (int e = require_not_failed()) return e;
	if (int e = order_.begin(stream)) return e; // bricks uploaded on the load stream must be visible to these frames
	FrameOrder::Ending frame(order_, stream);
	// ---- `count` consecutive entries of the frame ring (constants + ticket counters) and a clock slot, once the launches that used them
	// last have finished (launch_book.h FrameRing: the slot's previous user, then the younger owners of the entries)
	const auto ring = frame_ring_.plan(count);
	for (int w = 0; w < ring.waits; ++w) BM_HIP(hipEventSynchronize(ev_stop_[ring.wait_slot[w]]));
	const int first = ring.first, slot = ring.slot;
	uint32_t* const work_counter = d_work_counter_ + static_cast<size_t>(first) * (kWorkCounterBytes / sizeof(uint32_t));
#ifdef BM_PHASE_TIMING
	DeviceCounters* const counters = d_counters_; // profiling build: the plain kernel reports its phase timers too
#else
	DeviceCounters* const counters = (fc.flags & BM_FLAG_COUNTERS) ? d_counters_.get() : nullptr;
#endif
	auto enqueue = [&]() -> int {
		BM_HIP(hipMemsetAsync(work_counter, 0, kWorkCounterBytes * static_cast<size_t>(plan.counter_blocks), stream)); // ticket counters of the persistent kernel
		std::memcpy(h_frame_constants_ + first, fcs.data(), sizeof(FrameConstants) * static_cast<size_t>(count));
		BM_HIP(hipMemcpyAsync(d_frame_constants_ + first, h_frame_constants_ + first, sizeof(FrameConstants) * static_cast<size_t>(count), hipMemcpyHostToDevice, stream));
		BM_HIP(hipEventRecord(ev_start_[slot], stream));
		launch_trace(view_, d_frame_constants_ + first, counters, work_counter, plan.instrumented, fc.xcd_handout != 0, fc.helpers != 0, plan.ring_mode, plan.workgroups,
					 compute_units_, blocks_per_cu_[plan.instrumented ? 1 : 0], stream);
		BM_HIP(hipGetLastError());
		BM_HIP(hipEventRecord(ev_stop_[slot], stream));
		return frame.end(); // what process_load_queue orders itself behind
	};
	if (int e = enqueue()) {
		// part of the launch may be queued, and nothing records that it uses the ring entries and the pinned constants: wait for it
		// here, so that no later launch writes them under a copy that is still pending
		(void)hipStreamSynchronize(stream);
		return e;
	}
	frame_ring_.issued(ring);
	return 0;
}

// ---- ray queries (bm_scene_cast_rays).  Issued through the frames' bookkeeping: the stream is ordered behind pending uploads and
// edits (begin_frame), and process_load_queue orders itself behind the query (end_frame).  The kernel only reads the world, apart
// from the request atomics, so it may run beside frames.
int Scene::cast_rays(int64_t n, const bm_ray* rays, bm_ray_hit* hits, uint32_t flags, const float* lod_origin, hipStream_t stream) {
	if (flags & ~(BM_QUERY_LOD | BM_QUERY_NO_REQUESTS)) { set_error("bm_scene_cast_rays: unknown flag"); return BM_EINVAL; }
	if (n < 0 || n > (int64_t{1} << 28)) { set_error("bm_scene_cast_rays: n must be 0 ... 2^28"); return BM_EINVAL; }
	if (n == 0) return 0;
	if (!rays || !hits) { set_error("bm_scene_cast_rays: null ray or hit buffer"); return BM_EINVAL; }
	int campos[3] = {0, 0, 0};
	if (flags & BM_QUERY_LOD) {
		if (!lod_origin) { set_error("bm_scene_cast_rays: BM_QUERY_LOD needs lod_origin"); return BM_EINVAL; }
		for (int i = 0; i < 3; ++i) {
			if (!(std::fabs(lod_origin[i]) < 16777216.f)) { set_error("bm_scene_cast_rays: lod_origin must be finite and below 2^24"); return BM_EINVAL; }
			campos[i] = static_cast<int>(lod_origin[i] / 8.f); // as fill_frame_constants: ivec3(camera.position / 8.f)
		}
	}
	if (int e = require_on_device()) return e;
	if (int e = require_not_failed()) return e;
	BM_HIP(hipSetDevice(device_));
	if (!d_query_tickets_) {
		if (int e = d_query_tickets_.alloc(kQueryRing * 128)) return e;
		for (Event& ev : ev_query_) if (int e = ev.create(hipEventDisableTiming)) return e;
		query_blocks_per_cu_[0] = query_blocks_per_cu(false);
		query_blocks_per_cu_[1] = query_blocks_per_cu(true);
	}
	const bool request = !(flags & BM_QUERY_NO_REQUESTS);
	DeviceScene view;
	if (int e = begin_frame(stream, &view, nullptr)) return e;
	FrameOrder::Ending frame(order_, stream);
	if (!(flags & BM_QUERY_LOD)) view.lod_distance_8x8x8 = view.lod_distance_2x2x2 = INT_MAX; // exact: every brick at voxel level
	const int slot = query_ring_.slot();
	uint32_t* ticket = d_query_tickets_ + slot * 32;
	if (query_ring_.reused()) BM_HIP(hipStreamWaitEvent(stream, ev_query_[slot], 0));
	BM_HIP(hipMemsetAsync(ticket, 0, sizeof(uint32_t), stream));
	launch_query(view, campos, rays, hits, static_cast<uint32_t>(n), ticket, query_blocks_per_cu_[request ? 1 : 0] * compute_units_, request, stream);
	BM_HIP(hipGetLastError());
	BM_HIP(hipEventRecord(ev_query_[slot], stream));
	query_ring_.issued();
	(void)frame.end();
	return 0;
}

// ---- volume queries (bm_scene_query_volumes).  Issued like a ray query; the kernels only read the world.  The item offsets are one
// buffer, so a query is ordered behind the previous one (on whatever stream that ran), and the buffer grows only once that has finished.
int Scene::query_volumes(int64_t n, const bm_volume* volumes, bm_volume_result* results, uint32_t flags, hipStream_t stream) {
	if (flags & ~BM_VOLUME_ANY) { set_error("bm_scene_query_volumes: unknown flag"); return BM_EINVAL; }
	if (n < 0 || n > (int64_t{1} << 24)) { set_error("bm_scene_query_volumes: n must be 0 ... 2^24"); return BM_EINVAL; }
	if (n == 0) return 0;
	if (!volumes || !results) { set_error("bm_scene_query_volumes: null volume or result buffer"); return BM_EINVAL; }
	if (!aligned(volumes, 4) || !aligned(results, 8)) {
		set_error("bm_scene_query_volumes: volumes must be 4-byte aligned, results 8-byte aligned");
		return BM_EINVAL;
	}
	if (int e = require_on_device()) return e;
	if (int e = require_not_failed()) return e;
	BM_HIP(hipSetDevice(device_));
	if (!volume_blocks_per_cu_[0]) {
		volume_blocks_per_cu_[0] = volume_blocks_per_cu(false);
		volume_blocks_per_cu_[1] = volume_blocks_per_cu(true);
	}
	const size_t need = volume_tmp_bytes(static_cast<uint32_t>(n));
	if (d_volume_tmp_.bytes() < need) {
		if (int e = volume_.wait()) return e;
		if (int e = d_volume_tmp_.reserve(std::max<size_t>(need, 1 << 16))) return e;
	}
	const bool any = (flags & BM_VOLUME_ANY) != 0;
	DeviceScene view;
	if (int e = begin_frame(stream, &view, nullptr)) return e;
	FrameOrder::Ending frame(order_, stream);
	if (int e = volume_.order(stream)) return e;
	launch_volume_query(view, volumes, results, static_cast<uint32_t>(n), any, d_volume_tmp_, volume_blocks_per_cu_[any ? 1 : 0] * compute_units_, stream);
	BM_HIP(hipGetLastError());
	if (int e = volume_.pass(stream)) return e;
	(void)frame.end();
	return 0;
}

int Scene::begin_frame(hipStream_t stream, DeviceScene* view, DeviceCounters** counters) {
	if (int e = require_on_device()) return e;
	BM_HIP(hipSetDevice(device_));
	if (int e = require_not_failed()) return e;
	if (int e = order_.begin(stream)) return e; // bricks uploaded on the load stream must be visible to this frame
	if (view) *view = view_;
	if (counters) *counters = d_counters_;
	return 0;
}

void Scene::end_frame(hipStream_t stream) { (void)order_.end(stream); }

int Scene::synchronize() {
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	return 0;
}

int Scene::last_render_ms(float* ms) {
	if (!ms) { set_error("null argument"); return BM_EINVAL; }
	if (frame_ring_.clock().launches() == 0) { set_error("no frame rendered yet"); return BM_ESTATE; }
	BM_HIP(hipSetDevice(device_));
	const int slot = frame_ring_.clock().last_slot();
	BM_HIP(hipEventSynchronize(ev_stop_[slot]));
	BM_HIP(hipEventElapsedTime(ms, ev_start_[slot], ev_stop_[slot]));
	return 0;
}

int Scene::render_times(float* ms, int capacity, int* count) {
	if (!ms || !count || capacity <= 0) { set_error("bad argument"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device_));
	const int n = frame_ring_.clock().recent(capacity);
	for (int k = 0; k < n; ++k) {
		const int slot = frame_ring_.clock().recent_slot(n, k);
		BM_HIP(hipEventSynchronize(ev_stop_[slot]));
		BM_HIP(hipEventElapsedTime(&ms[k], ev_start_[slot], ev_stop_[slot]));
	}
	*count = n;
	return 0;
}

int Scene::counters_read(bm_counters* out) {
	if (!out) { set_error("null argument"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	static_assert(sizeof(bm_counters) == sizeof(DeviceCounters::v), "counter blocks must match");
	BM_HIP(hipMemcpy(out, d_counters_, sizeof(bm_counters), hipMemcpyDeviceToHost));
	return 0;
}

int Scene::sched_stats_read(bm_sched_stats* out) {
	if (!out) { set_error("null argument"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	static_assert(sizeof(bm_sched_stats) == sizeof(DeviceCounters::sched) + sizeof(DeviceCounters::cycles), "scheduler stat blocks must match");
	BM_HIP(hipMemcpy(out, reinterpret_cast<const char*>(d_counters_.get()) + offsetof(DeviceCounters, sched), sizeof(bm_sched_stats), hipMemcpyDeviceToHost));
	return 0;
}

int Scene::sched_detail_read(uint64_t* out8) {
	if (!out8) { set_error("null argument"); return BM_EINVAL; }
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	BM_HIP(hipMemcpy(out8, reinterpret_cast<const char*>(d_counters_.get()) + offsetof(DeviceCounters, detail), 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
	return 0;
}

int Scene::counters_reset() {
	BM_HIP(hipSetDevice(device_));
	BM_HIP(hipDeviceSynchronize());
	BM_HIP(hipMemset(d_counters_, 0, sizeof(DeviceCounters)));
	return 0;
}

} // namespace bm
