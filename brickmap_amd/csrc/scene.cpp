// scene.cpp -- one GPU's scene: lifetime, the world on the device, loads and frame launch (residency and streaming: residency.cpp; edits and region writes: world_changes.cpp; region reads, labels and queries: world_reads.cpp).
#include "scene.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

int Scene::ready() const {
	if (int e = require_on_device()) return e;
	if (int e = require_not_failed()) return e;
	BM_HIP(hipSetDevice(device_));
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
	if (int e = ready()) return e;
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

// ---------------------------------------------------------------- what only reads the world: world_reads.cpp
int Scene::read_region(const bm_region* region, uint8_t* voxels, int where, hipStream_t stream) {
	bm_region r;
	uint64_t span = 0;
	if (int e = check_region("bm_scene_read_region", region, voxels, where, &r, &span)) return e;
	if (span == 0) return 0;
	return reads_.read_region(r, voxels, where, stream);
}

int Scene::label_region(const int32_t lo[3], const int32_t hi[3], uint32_t flags, int32_t* labels, uint64_t* count, hipStream_t stream) { return reads_.label_region(lo, hi, flags, labels, count, stream); }

int Scene::last_label_ms(float* local_ms, float* merge_ms, float* flatten_ms) { return reads_.last_label_ms(local_ms, merge_ms, flatten_ms); }

int Scene::label_components(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, bm_component* comps, int64_t capacity, hipStream_t stream) {
	return reads_.label_components(lo, hi, labels, comps, capacity, stream);
}

int Scene::label_mask(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, const bm_component* comps, int64_t n, const uint8_t* chosen, uint8_t* mask,
					  hipStream_t stream) {
	return reads_.label_mask(lo, hi, labels, comps, n, chosen, mask, stream);
}

int Scene::cast_rays(int64_t n, const bm_ray* rays, bm_ray_hit* hits, uint32_t flags, const float* lod_origin, hipStream_t stream) { return reads_.cast_rays(n, rays, hits, flags, lod_origin, stream); }

int Scene::query_volumes(int64_t n, const bm_volume* volumes, bm_volume_result* results, uint32_t flags, hipStream_t stream) { return reads_.query_volumes(n, volumes, results, flags, stream); }

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
