// scene.h -- device-resident brickmap scene for one GPU: lifetime, the world on the device, loads and frame launch; what else changes the world
// (world_changes.h) and what only reads it (world_reads.h) it holds as members and forwards to.
// Mirrors the device half of the reference's Scene (src/Scene.cpp:29-36,152-194,200-258) and the
// host orchestration of launch_kernels (src/kernel.cu:366-439).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/brickmap.h"
#include "device_ops.h"
#include "device_types.h"
#include "error.h"
#include "frame_order.h"
#include "frame_plan.h"
#include "hip_owned.h"
#include "kernels.h"
#include "launch_book.h"
#include "residency.h"
#include "walk_fields.h"
#include "world.h"
#include "world_changes.h"
#include "world_reads.h"

namespace bm {

class Scene {
public:
	explicit Scene(int device)
		: device_(device), fields_(device), residency_(device, &world), changes_(device, &world, &residency_, &fields_, &order_, &load_stream_),
		  reads_(device, &world, &residency_, &order_, &view_, &compute_units_, [this] { return ready(); }) {}
	~Scene();

	int init(int grid_size, int grid_height); // Scene::Scene: streams + pinned staging
	int set_lod(int lod8, int lod2);
	int set_queue_capacity(int cap);
	int set_streaming_mode(int overlapped);
	int generate(int threads);                // Scene::generate
	int generate_supercell(int sx, int sy, int sz);
	int preload_all();
	int reset_residency();
	int process_load_queue(uint32_t* serviced); // Scene::process_load_queue + upload
	int dump(const char* path);
	int info(bm_scene_info* out);
	int device_indices(int supercell, uint32_t* out4096);
	int device_brick(int supercell, uint32_t device_slot, uint32_t* out16);
	// voxel edits (edit.hip / world_changes.h): host world first, then one scatter + the cube-field update on the load stream
	int edit(int count, const bm_edit* edits, hipStream_t stream);
	int host_cube_field(uint8_t* dst, size_t capacity, size_t* bytes);
	int last_edit_ms(float* scatter_ms, float* field_ms); // device time of the last batch that changed something
	// the cube field, the escape table and the planes derived from them: walk_fields.h has their readbacks and build statistics
	WalkFields& fields() { return fields_; }
	WalkFields* fields_on_device() { return require_on_device() ? nullptr : &fields_; } // null + message unless the world is on the device
	// dense regions (region.hip; world_changes.h writes, world_reads.h reads): a box of voxels written into / read out of the live scene
	int write_region(const bm_region* region, int op, const uint8_t* voxels, int where, hipStream_t stream);
	int read_region(const bm_region* region, uint8_t* voxels, int where, hipStream_t stream);
	int last_region_ms(float* pack_ms, float* copy_ms, float* scatter_ms, float* field_ms);
	// dense voxels -> scene (load.hip / scene.cpp "dense voxels -> scene"): replaces whatever world the scene holds; preloaded afterwards
	int load_voxels(const uint8_t* voxels, size_t bytes, int where, hipStream_t stream);
	int host_voxels(uint8_t* dst, size_t capacity, size_t* bytes);
	int last_load_ms(float* pack_ms, float* field_ms, float* mirror_ms); // device time of the last load from device memory
	// what only reads the world (world_reads.h): ray queries (query.hip), volume queries (volume.hip) and connected components (label.hip), issued
	// like a frame and asynchronous to the host; label_components and label_mask only read the caller's label volume
	int cast_rays(int64_t n, const bm_ray* rays, bm_ray_hit* hits, uint32_t flags, const float* lod_origin, hipStream_t stream);
	int query_volumes(int64_t n, const bm_volume* volumes, bm_volume_result* results, uint32_t flags, hipStream_t stream);
	int label_region(const int32_t lo[3], const int32_t hi[3], uint32_t flags, int32_t* labels, uint64_t* count, hipStream_t stream);
	int label_components(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, bm_component* comps, int64_t capacity, hipStream_t stream);
	int label_mask(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, const bm_component* comps, int64_t n, const uint8_t* chosen, uint8_t* mask,
				   hipStream_t stream);
	int last_label_ms(float* local_ms, float* merge_ms, float* flatten_ms);
	int render(const bm_camera* cam, const bm_frame_params* fp, float* accum, uint32_t* dbg, hipStream_t stream);
	// `count` consecutive frames as one launch (the frame ring, trace.hip); dbgs may be null, and so may any of its entries
	int render_frames(int count, const bm_camera* cams, const bm_frame_params* fps, float* const* accums, uint32_t* const* dbgs, hipStream_t stream);
	int synchronize();
	int last_render_ms(float* ms);
	int render_times(float* ms, int capacity, int* count); // durations of the most recent launches, oldest first
	int counters_read(bm_counters* out);
	int counters_reset();
	int sched_stats_read(bm_sched_stats* out);
	int sched_detail_read(uint64_t* out8);

	// Hooks for a frame issued by other code on this scene (the wavefront mode): begin_frame orders `stream` behind
	// pending brick uploads (frame_order.h) and hands out the current device view; end_frame records the "frame done" event process_load_queue waits for.
	int begin_frame(hipStream_t stream, DeviceScene* view, DeviceCounters** counters);
	void end_frame(hipStream_t stream);
	int compute_units() const { return compute_units_; }
	Gpu gpu() const { return {device_, compute_units_}; } // what the stateless operators (device_ops.h) need of a scene

	World world;
	int device() const { return device_; }

private:
	int allocate_device();
	int ensure_sun_plane(const FrameConstants& fc, bool* usable); // builds the sun plane for the frame's cone unless it stands; *usable: shadow rays of that cone may read it
	int ensure_view_plane(const std::vector<FrameConstants>& fcs, bool* usable); // builds the view plane for the first frame's origin if the camera rests there; *usable: the plane stands for that origin
	void set_view_dims();
	int load_voxels_device(const uint8_t* voxels, hipStream_t stream);
	int check_region(const char* who, const bm_region* region, const void* voxels, int where, bm_region* r, uint64_t* span); // what write_region and read_region refuse
	void free_device();
	int require_on_device() const;  // BM_ESTATE + message unless the world is on the device
	int require_not_failed() const; // BM_ESTATE + message once a streaming batch has failed
	int ready() const;              // both, in this order, then the scene's device is the current one: what a call that is about to use the device asks first
	void residency_rebuilt(); // residency_ has written a new index grid: the fields and the ordering hear of it

	int device_;
	bool on_device_ = false;
	// the owners below free what they hold when the scene goes, in reverse order of declaration: the streams last
	Stream load_stream_; // Scene.cpp:34 (the reference's kernel stream, :35, has no counterpart: frames run on the caller's streams)
	// Who waits for whom.  Frames and the queries issued like them, on any stream, against what rewrites the world on the load stream: order_
	// (frame_order.h) owns those events and every decision about them.  The entries of the frame ring and the clocks of the launches:
	// frame_ring_ (launch_book.h) says which entries a launch takes and which earlier launches it waits for; the events stand here, indexed by
	// its clock slots.  A scratch or staging buffer that one call at a time may use: a Turn (hip_owned.h) beside the buffer.  Which brick is
	// resident where, the request rings and the upload batches: residency_ (residency.h; pool_book.h takes the decisions, the failed flag among them).
	// The device half of an edit or a region write, its staging and its stage clocks: changes_ (world_changes.h; change_book.h takes the decisions).
	// The calls that only read the world -- region reads, labels, ray and volume queries --, their scratch and the Turns beside it: reads_
	// (world_reads.h; read_book.h takes the decisions).
	FrameOrder order_;
	static constexpr int kTimingRing = 256; // hipEvent pairs around the most recent render launches
	Event ev_start_[kTimingRing], ev_stop_[kTimingRing];

	// what the walk reads instead of index words: the cube field with the sun and the view plane, the escape table with the shadow heights, their
	// scratch and the book of which derived plane stands and what makes it stale (walk_fields.h; every flag is explained in field_book.h)
	WalkFields fields_;
	Residency residency_;
	WorldChanges changes_;
	WorldReads reads_;
	DeviceBuffer<DeviceCounters> d_counters_;
	// the frame ring: constants and ticket counters of the frames in flight -- a launch takes as many consecutive entries as it has frames
	static constexpr int kFrameRing = 1024; // (a launch takes at most kMaxFramesPerLaunch, frame_plan.h)
	DeviceBuffer<FrameConstants> d_frame_constants_; // kFrameRing device copies
	PinnedBuffer<FrameConstants> h_frame_constants_; // pinned source of the copies
	DeviceBuffer<uint32_t> d_work_counter_; // chunk counters of the persistent trace kernel: kFrameRing blocks of kWorkCounterBytes, zeroed before the launch that uses them
	FrameRing<kFrameRing, kTimingRing, kMaxFramesPerLaunch> frame_ring_;
	int compute_units_ = 0, blocks_per_cu_[2] = {0, 0};
	// The stage clock of a load from device memory (StageMarks, made on first use) with the stages the last load recorded (kClocked*, change_book.h:
	// 0 = nothing to report): marks 0, 1 around classify + number, 2 ... 5 around pack, field and mirror (the host's round trip lies between 1 and 2).
	StageMarks<6> load_marks_;
	unsigned load_clocked_ = 0;
	int lod8_ = 600000, lod2_ = 100000;          // variables.h:24-27
	DeviceScene view_{};
};

} // namespace bm
