/*
 * brickmap.h -- C-ABI of libbrickmap_hip.so: the MI355X (gfx950) brickmap path tracer.
 *
 * This is the drop-in boundary for ONE hot path of stijnherfst/BrickMap: the per-frame
 * path-trace launch (reference src/launch.h:6, src/kernel.cu:366-439) plus the Scene
 * object that feeds it (reference src/Scene.h:7-44, src/Scene.cpp:29-258).  Plain C types
 * only; every entry point returns 0 on success or a non-zero hipError_t / BM_E* code and
 * leaves a message for bm_last_error_string().  (The reference aborts the process inside
 * its cuda() macro, src/assert_cuda.cpp:3-13; the C++ mirror in brickmap.hpp keeps that
 * behaviour on top of these return codes.)
 *
 * Not thread-safe per scene; one scene per GPU (the reference is single-threaded,
 * src/main.cpp:117-182).  All file:line citations are into the reference's src/.
 */
#ifndef BRICKMAP_H
#define BRICKMAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BM_API __attribute__((visibility("default")))

/* error codes outside the hipError_t range */
#define BM_EINVAL 10001 /* bad argument                                   */
#define BM_ESTATE 10002 /* call made in the wrong state (e.g. not generated) */

/* index-word layout, variables.h:29-33 */
#define BM_BRICK_INDEX_BITS 0x00000FFFu
#define BM_BRICK_LOD_BITS 0x000FF000u
#define BM_BRICK_REQUESTED_BIT 0x20000000u
#define BM_BRICK_UNLOADED_BIT 0x40000000u
#define BM_BRICK_LOADED_BIT 0x80000000u

/* frame flags */
#define BM_FLAG_PRIMARY_ONLY 1u /* BASELINE config 1: extend the primary ray only          */
#define BM_FLAG_COUNTERS 2u     /* accumulate the traversal counters (instrumented kernel)  */
#define BM_FLAG_SAMPLE_ITEMS 4u /* schedule (4x4 chunk, sample) work items instead of pixels: samples of a pixel run on
                                   different lanes and are summed with float atomics (order not fixed).  debug_dev then
                                   holds an order-independent digest per pixel: words 4-7 are the SUMS (mod 2^32) over the
                                   samples of the per-sample path hashes / ray counts / cell counts (zero the buffer first),
                                   words 0-3 the first-hit record of the launch's first sample.
                                   For shards with few pixels and many samples, e.g. 1/N row bands of a multi-GPU frame; also the
                                   faster mode of any frame with several samples per pixel (1080p at 4 spp: 3.7 ms against 4.4,
                                   4K at 4 spp: 23.0 against 24.0 -- shorter items, shorter tail) when a fixed summation order is not needed */

/* (8u: retired -- the K-slot schedule of rounds 4-5, tools/variants/kslot.patch; unknown bits are refused with BM_EINVAL) */

#define BM_FLAG_ORDERED 16u     /* every pixel's events are accumulated in path order by the one lane that owns it and written back with
                                   one plain store: a frame's sums are reproducible bit for bit.  WITHOUT this flag (the default) a wave
                                   may hand a path's shadow ray to one of its idle lanes (csrc/trace.hip HELP): the same rays are
                                   traced, the unoccluded sun light is added to the pixel with float atomics like the reference's
                                   connect does (kernel.cu:341-343), and radiance is equal up to summation order (~1e-7 relative); and a
                                   frame with several samples per pixel is scheduled as (4x4 chunk, sample) work items, as if
                                   BM_FLAG_SAMPLE_ITEMS were set (1080p at 4 spp: 3.4 ms against 4.0).
                                   Frames that write hit records (debug_dev != NULL, without BM_FLAG_RAY_DIGEST) and primary-only frames are always ordered. */

#define BM_FLAG_RAY_DIGEST 32u  /* with debug_dev: the frame keeps its production plan (helper lanes, (chunk, sample) items -- NOT forced ordered) and
                                   debug_dev holds an order-independent digest per pixel instead of hash chains in path order: words 4 / 5 are the
                                   SUMS (mod 2^32) over the pixel's extend / shadow rays of keyed per-ray hashes -- key = sample << 8 | segment of
                                   the ray's path; extend: hit, distance bits, normal | level, brick id, voxel id; shadow: occluded, occluder --
                                   word 6 the ray counts, word 7 the cells visited, words 0-3 the first-hit record of the launch's first sample;
                                   each added by the lane that traced the ray (zero the buffer first).  What pins the TIMED instantiation's hits
                                   to the oracle bit for bit (oracle.c render_pixel holds the same sums).  spp * segments < 65536 per launch. */

typedef struct bm_scene bm_scene; /* Scene + its GPUScene view (Scene.h:7-44), one GPU */

/* camera.h:3-10 -- only the fields the kernels read (launch_kernels:384-385,416). */
typedef struct bm_camera {
	float position[3];    /* default (512,512,300)                      */
	float direction[3];   /* unit; Camera::update, camera.cpp:48-54      */
	float up[3];          /* default (0,0,1)                             */
	float focal_distance; /* default 1                                   */
	float lens_radius;    /* default 0                                   */
} bm_camera;

/*
 * One launch = `spp` complete paths per pixel of this shard's rows (the reference advances
 * every path one bounce per launch_kernels call; see DESIGN.md "Canonical path").
 * Sample s of pixel p (p = y*width + x, global) draws its random numbers exactly as the
 * reference does for queue slot  slot = p + (sample_base+s)*width*height  in frame
 * `base_frame + bounce` (kernel.cu:165,252).
 * Row sharding: global row y belongs to shard (y / band_rows) % shard_count; a shard's rows
 * are packed in increasing y into its local buffer.  (height, 0, 1) renders everything.
 */
typedef struct bm_frame_params {
	int32_t width, height;
	int32_t spp;
	int32_t sample_base;
	int32_t max_bounces;  /* kernel.cu:13 MAX_BOUNCES = 3 -> at most 4 segments per path */
	uint32_t base_frame;  /* kernel.cu:369 `frame` starts at 1                          */
	uint32_t flags;       /* BM_FLAG_*                                                  */
	int32_t band_rows, shard_rank, shard_count;
	float sun_position[2]; /* variables.cpp:3 default (0.05, 0.1)                        */
} bm_frame_params;

typedef struct bm_scene_info {
	int32_t grid_size, grid_height; /* voxels (variables.h:7-8, runtime here)            */
	int32_t supergrid_xy, supergrid_z, supercells;
	int32_t queue_capacity;         /* variables.h:35 brick_load_queue_size, default 1024 */
	int32_t lod_distance_8x8x8, lod_distance_2x2x2; /* variables.h:24-27                  */
	int32_t generated, on_device;
	uint64_t total_bricks;          /* non-empty bricks on the host                      */
	uint64_t resident_bricks;       /* bricks currently in the device arena              */
	uint64_t index_bytes, brick_bytes; /* device allocations: index grid; brick arena as allocated (grows by residency) */
	uint64_t pool_bytes;            /* part of the arena handed to supercell pools (16-brick pools that double, Scene.cpp:231-251) */
	uint64_t cube_field_bytes;      /* octant cube field of the walk (8 bytes per brick cell; the sun plane is counted in sun_plane_bytes) */
	uint64_t arena_growths;         /* times the brick arena grew while bricks were resident (pool growth, Scene.cpp:231-251)      */
	uint64_t arena_copy_growths;    /* ... of which by device synchronisation + reallocation + copy: 0 when the arena is a virtual
	                                   address range that physical chunks are mapped into (arena_virtual)                        */
	int32_t arena_virtual;          /* 1: hipMemAddressReserve / hipMemMap arena (grows without copy or synchronisation)          */
	int32_t failed;                 /* 1: a streaming batch could not be completed; frames are refused until the residency is reset */
	uint64_t stream_batches;        /* upload batches queued since the residency was last reset                                   */
	uint64_t stream_host_ns;        /* host time spent staging them (validate, copy bricks to pinned memory, hand out slots, queue) */
	uint64_t escape_bytes;          /* escape heights of the walk: 8 octants x one 32-bit entry per cell column, in rows padded like the cube field's                    */
	uint64_t sun_plane_bytes;       /* the sun plane of shadow rays: a ninth plane of the cube field's size (not part of cube_field_bytes) plus the scratch of its
	                                   builds so far (32 bytes per cell of a slab, 4 per cell column); 0 for a scene that has no ninth plane */
} bm_scene_info;

/* one voxel edit (bm_scene_edit).  Voxel coordinates are integers; a batch applies its edits in order. */
#define BM_EDIT_SET 1    /* the shape's voxels become solid */
#define BM_EDIT_CLEAR 2  /* the shape's voxels become empty */
#define BM_EDIT_BOX 1    /* voxels v with lo <= v < hi on every axis (half-open)                          */
#define BM_EDIT_SPHERE 2 /* voxels v with sum over the axes of (v - center)^2 <= radius^2 (64-bit integers) */
typedef struct bm_edit {
	int32_t op;         /* BM_EDIT_SET / BM_EDIT_CLEAR     */
	int32_t shape;      /* BM_EDIT_BOX / BM_EDIT_SPHERE    */
	int32_t lo[3];      /* box: first voxel                */
	int32_t hi[3];      /* box: one past the last voxel    */
	int32_t center[3];  /* sphere: centre voxel            */
	int32_t radius;     /* sphere: radius in voxels, >= 0  */
} bm_edit;

/* traversal counters (BM_FLAG_COUNTERS); same order as oracle/oracle.c orc_counters */
typedef struct bm_counters {
	uint64_t index_loads, brick_tests, byte_tests, voxel_steps, extend_rays, shadow_rays, requests, paths;
} bm_counters;

/* wave-scheduler statistics of the instrumented kernel (BM_FLAG_COUNTERS): how often each phase of the
 * per-wave scheduler ran and with how many of the 64 lanes active */
typedef struct bm_sched_stats {
	uint64_t step_runs, step_lanes;           /* phase A: brick-grid DDA moves       */
	uint64_t candidate_runs, candidate_lanes; /* phase B: index word + bitmask DDA   */
	uint64_t shade_runs, shade_lanes;         /* phase C: shade / next primary ray   */
	uint64_t connect_runs, connect_lanes;     /* shade passes that also held finished shadow rays (connect), and how many */
	/* shader-clock ticks spent in each phase and in the whole scheduler loop, summed over waves */
	uint64_t step_cycles, candidate_cycles, shade_cycles;
	uint64_t drain_cycles;                    /* from a wave's last (failed) refill to its exit: the end-of-frame drain */
	uint64_t total_cycles;
	uint64_t jump_runs, jump_lanes;           /* phase A, cube jumps (step_* count the single moves) */
	uint64_t waves;
} bm_sched_stats;

/* ---- errors (replaces assert_cuda.h:5 / assert_cuda.cpp:3-13) */
BM_API const char* bm_last_error_string(void);
BM_API int bm_device_count(int* count);
BM_API int bm_device_name(int device, char* buf, size_t buflen, int* compute_units);

/* ---- Scene (Scene.h:7-44) */
/* Scene::Scene (Scene.cpp:29-36): pinned staging + load_stream/kernel_stream on `device`. */
BM_API int bm_scene_create(int device, int grid_size, int grid_height, bm_scene** out);
BM_API void bm_scene_destroy(bm_scene* scene);
/* variables.h:24-27,35 made runtime; call before bm_scene_generate. */
BM_API int bm_scene_set_lod(bm_scene* scene, int lod_distance_8x8x8, int lod_distance_2x2x2);
BM_API int bm_scene_set_queue_capacity(bm_scene* scene, int capacity);
/* 0 (default): bm_scene_process_load_queue waits for the frame and services its requests at once (reference order,
 * main.cpp:142-144).  1: overlapped -- two request rings alternate; the call services the ring copied out by the
 * previous call and starts the asynchronous copy-out of the last frame's ring on the load stream, so the host never
 * waits for the GPU (a brick requested in frame k is resident from frame k+2 on; reference order: from frame k+1 on). */
BM_API int bm_scene_set_streaming_mode(bm_scene* scene, int overlapped);
/* Scene::generate (Scene.cpp:118-194): CPU world build on `threads` host threads, then the
 * device allocations in the reference's initial state (nothing resident: unloaded|lod). */
BM_API int bm_scene_generate(bm_scene* scene, int threads);
/* Scene::generate_supercell (Scene.cpp:44-116): rebuild one supercell on the host.  Only before bm_scene_generate has put
 * the world on the device (BM_ESTATE afterwards: the pools hold bricks in request order and the index words name those
 * slots; the reference never regenerates a supercell of a live scene either). */
BM_API int bm_scene_generate_supercell(bm_scene* scene, int sx, int sy, int sz);
/* BASELINE configs 1-2 "all bricks pre-loaded": device words = host words, arena = every host brick. */
BM_API int bm_scene_preload_all(bm_scene* scene);
/* back to the reference's initial residency (Scene.cpp:157-175) */
BM_API int bm_scene_reset_residency(bm_scene* scene);
/* Scene::process_load_queue (Scene.cpp:200-252) fused with the upload kernel of the next
 * launch_kernels (kernel.cu:141-151,407-414): read the request ring, stage bricks in pinned
 * memory, async H2D on the load stream, scatter into arena + index grid, reset the count.
 * *serviced = number of bricks made resident. */
BM_API int bm_scene_process_load_queue(bm_scene* scene, uint32_t* serviced);
/* Scene::dump (Scene.cpp:254-258): one line per supercell = resident brick count. */
BM_API int bm_scene_dump(bm_scene* scene, const char* path);
BM_API int bm_scene_get_info(bm_scene* scene, bm_scene_info* info);
/* test/inspection doors: host supercell content and the device index block */
BM_API int bm_scene_host_supercell(bm_scene* scene, int supercell, uint32_t* indices4096, uint32_t* brick_count,
                                   uint32_t* bricks, uint32_t brick_capacity);
BM_API int bm_scene_device_indices(bm_scene* scene, int supercell, uint32_t* indices4096);
/* the 64-byte brick stored at `device_slot` (the 12-bit slot of a DEVICE index word) of a supercell's arena region */
BM_API int bm_scene_device_brick(bm_scene* scene, int supercell, uint32_t device_slot, uint32_t* brick16);
BM_API int bm_scene_column_heights(bm_scene* scene, int sx, int sy, float* heights128x128);

/* ---- voxel edits of a live scene (no reference counterpart: the reference builds its world once, Scene.cpp:118-147).
 * Apply `count` edits, in order, to a scene after bm_scene_generate.  Shapes are clipped to the world (one wholly outside is a
 * no-op); a malformed edit (unknown op or shape, hi < lo, radius < 0) is BM_EINVAL and the scene is left unchanged -- the whole
 * batch is checked first.  The host world stays authoritative: every brick's bits, LoD mask (Scene.cpp:95) and index word
 * (slot | loaded | lod << 12, Scene.cpp:104) are what the generator would store for that content, a brick that becomes empty gets
 * word 0 and frees its slot, a cell that gains voxels gets a brick (freed slots first: slots stay below 4096).  On the device a
 * resident brick is rewritten in place; a new brick is uploaded at once in a preloaded scene (bm_scene_preload_all) and becomes
 * unloaded | lod in a streaming one (requested again, like a changed brick that is not resident).  The octant cube field is
 * recomputed on the GPU where the batch can change it and equals bm_scene_host_cube_field byte for byte.  The edit runs on the
 * scene's load stream behind every frame in flight and behind the work queued on `hip_stream` so far; frames issued before it
 * see the old world, frames issued after it the new one.  A request for a brick that an edit emptied is skipped. */
BM_API int bm_scene_edit(bm_scene* scene, int count, const bm_edit* edits, void* hip_stream);
/* single voxels: xyz[n][3] voxel coordinates, values[n] != 0 -> solid, 0 -> empty; otherwise as bm_scene_edit (a voxel outside the
 * world is a no-op) */
BM_API int bm_scene_set_voxels(bm_scene* scene, int n, const int32_t* xyz, const uint8_t* values, void* hip_stream);
/* the device's octant cube field, read back in the tight layout of bm_host_cube_field (waits for the device); *bytes = size
 * needed (dst = NULL to query) */
BM_API int bm_scene_device_cube_field(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes);
/* the cube field built on the host from the scene's current host world (bm_host_cube_field's layout) */
BM_API int bm_scene_host_cube_field(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes);
/* the device's escape heights (waits for the device): per direction octant o (bit 0 / 1 / 2 = direction negative in x / y / z) and
 * brick-cell column (x, y), dst[(o * cells + y) * cells + x] = the threshold E of the walk's escape rule -- octants 0-3: the highest
 * occupied cell z over the columns x' >= x (octant bit 0 clear; x' <= x if set), y' likewise, -1 if there is none: a ray of the octant
 * in a cell above E is a miss; octants 4-7: the lowest such z, cells_height if none: a miss below E.  *count = entries (8 * cells^2),
 * also when dst is null.  Kept exact by bm_scene_load_voxels, edits and region writes, like the cube field. */
BM_API int bm_scene_escape_table(bm_scene* scene, int32_t* dst, size_t capacity, size_t* count);
/* ---- the sun plane: a ninth plane of the cube field that only shadow rays read, built for the cone of ONE sun (the first production frame
 * that needs it builds it on the device; it is rebuilt before the next such frame after the sun or the world has changed, and scenes
 * whose ninth plane could not be allocated, suns below the horizon and cones that touch an octant boundary or a diagonal do without).
 * bm_scene_sun_plane copies the plane as it was last built (waits for the device): dst[(z * X + y) * X + x] over the bordered grid, X =
 * cells + 2 (border bytes 255), one byte per brick cell -- 0: the cell holds a brick; 255: no ray of the cone can hit anything from here
 * on; n: no ray of the cone, from anywhere in the cell, enters an occupied cell before one of its axes has moved n cells.  *bytes = the
 * size needed, 0 when no plane has been built (also when dst is null).  plan12 (may be null) gets the plan it was built for: valid,
 * octant, dominant axis, minor axes m1 and m2, bins moved per slab along m1 (least, most) and along m2 (least, most), whether clear
 * heights were built, rise per slab in 1/256 cells, bins per cell. */
BM_API int bm_scene_sun_plane(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes, int32_t* plan12);
/* ---- shadow heights: with the sun plane, and for the same cone, the scene keeps per brick-cell column the height below which no ray of
 * the cone can reach the sun (only for cones whose dominant axis is horizontal, and only while every brick is resident: a scene that
 * streams its bricks in has none, its table is zero); production shadow rays that start below it end at once, occluded.  Rebuilt with the plane, and alone after a change that left every cell's occupancy as it was.  bm_scene_shadow_heights
 * copies the 32-bit table entries as last built (waits for the device): dst[y * cells + x] = 0 where the column has no dark cell,
 * otherwise the sun plane's byte offset of the first slice that is not dark, 8 * plane + (Zd + 1) * slice pitch.  *count = entries needed
 * (cells^2; 0 when nothing has been built), also when dst is null; *bytes = device memory of the table's slice and the build's scratch (not
 * part of escape_bytes or sun_plane_bytes); plan4: valid, least and most rise per slab, height units per cell. */
BM_API int bm_scene_shadow_heights(bm_scene* scene, uint32_t* dst, size_t capacity, size_t* count, uint64_t* bytes, int32_t* plan4);
/* how often the sun plane has been built since the scene was created, and the device time of the last build in ms (0 before the first;
 * waits for that build).  A rebuild of the shadow heights alone (above) is not counted as a build, but last_build_ms is then its time. */
BM_API int bm_scene_sun_plane_stats(bm_scene* scene, uint64_t* builds, float* last_build_ms);
/* ---- the view plane: a tenth plane of the cube field that only primary rays read, built for ONE camera position (the origin of the first
 * frame of a production launch) once the camera rests there: the launch holds at least two frames from that origin, or the production
 * launch before it started from it.  Rebuilt on the same terms after the world has changed; positions outside the world box, cameras
 * with a lens and scenes whose tenth plane could not be allocated do without, and a camera that moves every frame never builds one.
 * bm_scene_view_plane copies the plane as it was last built (waits for the device), in the sun plane's layout: 0: the cell holds a brick;
 * 255: no ray from the origin that visits the cell can hit anything from here on; n: no such ray enters an occupied cell before one of
 * its axes has moved n cells.  *bytes = the size needed, 0 when no plane stands (also when dst is null); origin3 (may be null) gets the
 * origin it was built for.  The plane takes one more plane of the cube field's size (cube_field_bytes / 8), counted nowhere else.
 * bm_scene_view_plane_stats: how often it has been built, and the device time of the last build in ms (0 before the first; waits for it). */
BM_API int bm_scene_view_plane(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes, float* origin3);
BM_API int bm_scene_view_plane_stats(bm_scene* scene, uint64_t* builds, float* last_build_ms);
/* device time of the last batch that changed the scene (hipEvents on the load stream): the scatter (pool moves, bricks, words)
 * and the cube-field update with the escape-height update behind it (0 when no cell's occupancy changed); waits for that batch */
BM_API int bm_scene_last_edit_ms(bm_scene* scene, float* scatter_ms, float* field_ms);

/* ---- a scene from the caller's own voxels (no reference counterpart: the reference's only world is its terrain).
 * voxels: a dense volume V[z][y][x], x fastest, (grid_height, grid_size, grid_size), one byte per voxel, non-zero = solid; `bytes`
 * must be grid_size^2 * grid_height.  The scene becomes the CANONICAL BUILD of V -- what bm_scene_generate would store if the
 * terrain were V: a brick for every cell that holds a solid voxel (bit x + 8 y + 64 z, Scene.cpp:91-93), host slots 0, 1, 2 ... in
 * ascending local cell index, word = slot | loaded | lod << 12 (Scene.cpp:95,104), no free slots -- and is on the device in the
 * state bm_scene_generate + bm_scene_preload_all leave it in, the octant cube field included; the host world is populated and
 * authoritative, so resetting residency, edits, queries and frames work on it as on a generated scene.  Allowed right after
 * bm_scene_create and on a scene that holds a world (which it replaces).  The call waits for the device first and returns when
 * the scene is ready; the volume is only read during the call.
 *  - BM_VOXELS_HOST: the volume is host memory; built on CPU threads and uploaded.
 *  - BM_VOXELS_DEVICE: the volume is memory of the scene's device; packed there by the kernels of csrc/load.hip without crossing
 *    to the host, behind the work queued on hip_stream so far (the stream that produced the volume).  The cube field is computed
 *    on the GPU; words and bricks are copied back into the host world.
 * A null volume, a wrong byte count, an unknown `where` or (BM_VOXELS_DEVICE) a pointer that is not `bytes` bytes of that device's
 * memory: BM_EINVAL, and the scene keeps the world it held.  A world of 2^32 bricks or more is refused as by bm_scene_generate. */
#define BM_VOXELS_HOST   0
#define BM_VOXELS_DEVICE 1
BM_API int bm_scene_load_voxels(bm_scene* scene, const uint8_t* voxels, size_t bytes, int where, void* hip_stream);
/* the host world as a dense volume of 0 / 1 in the layout above (host only); *bytes = size needed (dst = NULL to query) */
BM_API int bm_scene_host_voxels(bm_scene* scene, uint8_t* dst, size_t capacity, size_t* bytes);
/* device time of the last BM_VOXELS_DEVICE load (hipEvents on the load stream): pack = classify + number + pack kernels (without the
 * host's round trip that sizes the arena), the cube-field passes with the escape-height build behind them, and the copy back into the host world.  BM_ESTATE when the last load
 * was not from device memory. */
BM_API int bm_scene_last_load_ms(bm_scene* scene, float* pack_ms, float* field_ms, float* mirror_ms);

/* ---- dense voxel regions of a live scene: write a box of arbitrary voxels into it, read one out (no reference counterpart).
 * The volume is V[z][y][x], one byte per voxel, non-zero = solid; x is contiguous, rows and slices lie at the given pitches, so a
 * sub-box of a larger array or tensor is passed without a copy.  `where` says where V lies: BM_VOXELS_HOST, or BM_VOXELS_DEVICE for
 * memory of the scene's device (packed / unpacked there by the kernels of csrc/region.hip).
 *  - Clipping: the box is clipped to the world like an edit's shape.  A write ignores the volume's voxels outside the world; a read
 *    returns them as 0.  A box wholly outside the world is a no-op for a write and all zeros for a read; an empty box (hi == lo on some
 *    axis) is a no-op.
 *  - Refusals, BM_EINVAL with the scene as it was: hi < lo on an axis, an unknown op or `where`, a null pointer, a pitch smaller than
 *    the extent it spans (row_pitch < hi.x - lo.x, slice_pitch < row_pitch * (hi.y - lo.y)), and for BM_VOXELS_DEVICE a pointer whose
 *    span of (nz - 1) * slice_pitch + (ny - 1) * row_pitch + nx bytes does not lie inside one allocation of the scene's device.  A scene
 *    that is not on the device, or a failed one: BM_ESTATE.  Everything is checked before anything changes.
 *  - Result of a write, per brick cell, supercells independent, cells in ascending local index: with cover = the clipped box's voxels
 *    in the cell, new = (old & ~cover) | (V & cover) for BM_REGION_REPLACE, old | (V & cover) for BM_EDIT_SET, old & ~(V & cover) for
 *    BM_EDIT_CLEAR.  A cell with new == old is NOT TOUCHED: word, brick, slot and device state stay, the requested flag included (so
 *    writing the same region every step causes no churn; bm_scene_edit marks every cell its shapes reach).  An empty cell that gains
 *    voxels takes a freed slot (last freed first), else a new one; a brick that becomes empty gets word 0 and frees its slot; else the
 *    cell keeps its slot.  This is what bm_scene_edit gives for the batch that, cell by cell, sets the voxels of new & ~old and then
 *    clears those of old & ~new.  The changed cells reach the device exactly as an edit's do (residency rule, pool growth, scatter,
 *    cube-field update where occupancy changed).
 *  - Ordering: a write is ordered like bm_scene_edit (frames and queries issued before it see the old world, those issued after it
 *    the new one; the volume is read behind the work queued on hip_stream so far, and is no longer needed when the call returns).  A
 *    read is issued like a query on hip_stream: it sees every edit, write and upload issued before it; later edits and
 *    bm_scene_process_load_queue order themselves behind it; a device read is asynchronous to the host in a preloaded scene.
 *  - A device write packs the box into one 64-byte brick per covered cell on the GPU, copies those to the host (the call's one
 *    round trip: 1/8 of the volume's bytes; the host world is authoritative and hands out the slots) and merges there.  Temporary
 *    memory: 64 bytes per covered cell on the device and in pinned memory, kept and grown on demand. */
typedef struct bm_region {
	int32_t lo[3], hi[3];   /* voxels v with lo <= v < hi on (x, y, z), half-open like BM_EDIT_BOX */
	int64_t row_pitch;      /* bytes from one x-row to the next y; 0 = tight (hi.x - lo.x) */
	int64_t slice_pitch;    /* bytes from one z-slice to the next; 0 = tight (row_pitch * (hi.y - lo.y)) */
} bm_region;
#define BM_REGION_REPLACE 0 /* the region's voxels become exactly the volume's; BM_EDIT_SET: solid where V is non-zero; BM_EDIT_CLEAR: empty where V is non-zero */
BM_API int bm_scene_write_region(bm_scene* scene, const bm_region* region, int op, const uint8_t* voxels, int where, void* hip_stream);
BM_API int bm_scene_read_region(bm_scene* scene, const bm_region* region, uint8_t* voxels, int where, void* hip_stream);
/* times of the last bm_scene_write_region that reached the device, in ms (hipEvents on the load stream; waits for that write): the
 * pack kernel and the copy of the packed bricks to the host (both 0 for BM_VOXELS_HOST), the scatter and the cube-field update with the escape-height update behind it (0 when
 * no cell changed / no cell's occupancy changed).  BM_ESTATE before the first write. */
BM_API int bm_scene_last_region_ms(bm_scene* scene, float* pack_ms, float* copy_ms, float* scatter_ms, float* field_ms);

/* ---- ray queries against the live scene (no reference counterpart: the reference only traces inside its frame kernels).
 * What does a ray hit -- the voxel under the cursor, the ground under a walking camera, line of sight, collision probes.
 * A query walks exactly as the frames' extend kernel does (csrc/traverse.h), so a hit equals the reference's intersect_voxel bit
 * for bit: distance, entry normal, level and cell. */
typedef struct bm_ray {         /* 32 bytes */
	float origin[3];
	float direction[3];         /* need not be unit length; the hit point is origin + distance * direction */
	float tmax;                 /* hits with distance > tmax are reported as misses; +inf = unbounded */
	uint32_t reserved;          /* 0 (a ray with another value is reported as a miss) */
} bm_ray;
typedef struct bm_ray_hit {     /* 32 bytes */
	float distance;             /* +inf on a miss */
	float normal[3];            /* entry face of the hit cell; (0,0,0) for a ray that starts inside a solid voxel, and on a miss */
	int32_t voxel[3];           /* level 2: the voxel hit; level 1: first voxel of the 4^3 block; levels 0 and 3: first voxel of the brick; -1 on a miss */
	int32_t level;              /* -1 miss, 0 brick-LoD hit, 1 2^3-LoD hit, 2 voxel hit, 3 unresolved: the brick is not resident */
} bm_ray_hit;
#define BM_QUERY_LOD         1u /* resolve with the frames' LoD rule around lod_origin (campos = int(lod_origin / 8), as in fill_frame_constants) */
#define BM_QUERY_NO_REQUESTS 2u /* a non-resident brick is reported as level 3 but not requested, and no index word is written */
/* The first hit of each of n rays (rays_dev, hits_dev: device memory, n records each; hit i belongs to ray i).
 *  - Default (exact): every brick is walked at voxel level, whatever its distance; with BM_QUERY_LOD the frames' LoD rule applies
 *    around lod_origin (voxel coordinates), with the scene's LoD distances (bm_scene_set_lod).
 *  - A brick that is not resident gives level 3 at its entry distance and is requested through the frames' protocol (unless
 *    BM_QUERY_NO_REQUESTS); the next bm_scene_process_load_queue services it, so a preloaded scene always answers exactly.
 *  - tmax: the result equals the unbounded query's filtered by distance <= tmax.  The walk stops at the first brick cell whose
 *    entry distance is beyond tmax and files no request for it.
 *  - A zero or non-finite direction, or a non-finite origin, is a miss (checked before the walk); zero components are fine.
 *  - Ordering: issued like a frame on hip_stream -- it sees every edit and upload issued before it, on any stream, and
 *    bm_scene_process_load_queue orders itself behind it; asynchronous to the host.  It only reads the world (apart from request
 *    atomics), so it may run beside frames.
 *  - n == 0 is a no-op.  n < 0, n > 2^28, NULL buffers, unknown flags, or BM_QUERY_LOD with a NULL or non-finite lod_origin: BM_EINVAL;
 *    a scene not on the device, or a failed one: BM_ESTATE.  Nothing is launched on error. */
BM_API int bm_scene_cast_rays(bm_scene* scene, int64_t n, const bm_ray* rays_dev, bm_ray_hit* hits_dev, uint32_t flags,
                              const float lod_origin[3], void* hip_stream);
/* host only: pixel rays of a camera for a width x height frame -- the frames' primary_ray without jitter and lens: ray i starts at
 * the camera position and passes through continuous pixel position (px[i], py[i]); (x + 0.5, y + 0.5) is pixel (x, y)'s centre.
 * direction = normalize(dir + right * ni + up * nj) in the operation order of csrc/traverse.h primary_ray, with the camera basis of the
 * frames; tmax = +inf. */
BM_API int bm_camera_pixel_rays(const bm_camera* camera, int width, int height, int64_t n, const float* px, const float* py, bm_ray* out);

/* the same rays for EVERY pixel of a width x height frame, written on the device: ray y * width + x passes through the centre of pixel
 * (x, y), bit for bit what bm_camera_pixel_rays gives for (x + 0.5, y + 0.5) -- same operation order, tmax = +inf.  rays_dev: width * height
 * records of device memory, 16-byte aligned.  Asynchronous on hip_stream; reads nothing of the world.  (What a frame's guide query would
 * otherwise build on the host and upload: two million rays per 1080p frame.) */
BM_API int bm_camera_pixel_rays_device(bm_scene* scene, const bm_camera* camera, int width, int height, bm_ray* rays_dev, void* hip_stream);

/* ---- denoising a frame of few samples (no reference counterpart: the reference only accumulates, so a moving camera shows raw 1-spp
 * noise): an edge-avoiding a-trous filter guided by the first hit of every pixel's centre ray (bm_camera_pixel_rays_device +
 * bm_scene_cast_rays with BM_QUERY_LOD around the camera: the geometry the frame sees).  All arithmetic is fp32 IEEE + - * / sqrt in a
 * fixed order, without contraction, so bm_denoise and bm_host_denoise agree bit for bit (csrc/denoise.h holds the rules once).
 * Per pixel of the width x height image, row-major: the accumulation value (R, G, B, n) and one bm_ray_hit.
 *  - radiance c = (R/n, G/n, B/n) when n > 0, else 0; luminance l(c) = (0.2126 r + 0.7152 g) + 0.0722 b.
 *  - surface key: a pixel is SPECIAL when n <= 0, level is -1 or 3, or the normal is (0, 0, 0); else, with a = the first axis whose normal
 *    component is not zero, s = normal[a] > 0 and size = 1 / 4 / 8 for levels 2 / 1 / 0: plane = voxel[a] + (s ? size : 0), the plane of
 *    the entry face, and key = plane * 8 + a * 2 + s.  Pixels that see one face plane from one side share a key, whatever their LoD.
 *  - special pixels are never filtered and never a tap: their output is (c, 1).
 *  - a tap q of pixel p counts when it lies inside the image and key_q == key_p; other taps are skipped (nothing is added).  Every sum
 *    runs left to right within a row of taps starting from 0.0f; the row sums are added top to bottom onto 0.0f.
 *  - variance pass, 7 x 7 taps at stride 1: N = taps, S1 = sum l_q, S2 = sum l_q * l_q, var_p = max(0, S2/N - (S1/N) * (S1/N)).
 *  - a-trous pass i = 0 ... iterations - 1, 5 x 5 taps at stride 2^i, h = (1/16, 1/4, 3/8, 1/4, 1/16): den_p = sigma_l * sqrt(var_p) + 1e-4;
 *    per tap x = |l(c_p) - l(c_q)| / den_p, t = 1 + x, w = (h[dy] * h[dx]) / (t * t); W += w, C += w * c_q, V += (w * w) * var_q;
 *    then c_p = C / W, var_p = V / (W * W).
 *  - output (c, 1) per pixel, so bm_resolve takes it unchanged; iterations == 0 gives the unfiltered (c, 1).
 * The guides of a gathered frame: denoise the whole frame, not a row shard of it. */
typedef struct bm_denoise_params {
	int32_t width, height;
	int32_t iterations;   /* 0 ... 8; 5 is a good default */
	float sigma_l;        /* finite, > 0; 4 is a good default */
	uint32_t flags;       /* 0 */
	uint32_t reserved;    /* 0 */
} bm_denoise_params;
/* bytes of device memory bm_denoise needs beside its images: two float4 images and the keys, 36 bytes per pixel */
BM_API int bm_denoise_workspace_bytes(int width, int height, size_t* bytes);
/* accum_dev: width * height float4 (R, G, B, n) as bm_render_frame leaves them; hits_dev: one bm_ray_hit per pixel; out_dev: width * height
 * float4, may be accum_dev itself; workspace_dev: the caller's, not used by anything else until the call has finished on its stream -- the
 * scene holds no state for a denoise, so calls on different streams with workspaces of their own are independent.  Asynchronous on
 * hip_stream like bm_resolve.  Refused with BM_EINVAL, launching nothing: iterations outside 0 ... 8, sigma_l not finite or <= 0, width or
 * height < 1 or > 65535, non-zero flags or reserved, a NULL buffer, a workspace smaller than bm_denoise_workspace_bytes, a buffer that is
 * not 16-byte aligned, a workspace that overlaps an image. */
BM_API int bm_denoise(bm_scene* scene, const bm_denoise_params* params, const float* accum_dev, const bm_ray_hit* hits_dev, float* out_dev,
                      void* workspace_dev, size_t workspace_bytes, void* hip_stream);
/* measuring door: bm_denoise with a hipEvent between its kernels; waits, then kernel_ms[0 ... 1 + iterations] = the durations in ms of
 * prepare, the variance pass and every a-trous pass (iterations == 0: prepare alone, the second entry 0) */
BM_API int bm_debug_denoise_times(bm_scene* scene, const bm_denoise_params* params, const float* accum_dev, const bm_ray_hit* hits_dev, float* out_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* hip_stream, float* kernel_ms);
/* the same filter on host memory, as plain loops (no device needed); the refusals of bm_denoise that concern params and NULL buffers */
BM_API int bm_host_denoise(const bm_denoise_params* params, const float* accum, const bm_ray_hit* hits, float* out);

/* ---- temporal accumulation for a moving camera (no reference counterpart: the reference accumulates only while the camera rests):
 * the samples of earlier frames are carried to where the same surface point is now.  A surface is the exact integer key of the denoise
 * (face plane, axis, side), and the previous camera's ray through a point P of an axis-aligned plane meets that plane only in P, so "the
 * previous pixel carries the same key" is an exact disocclusion test -- no depth or normal threshold.  All arithmetic is fp32 IEEE
 * + - * / sqrt floor in a fixed order, without contraction, so bm_reproject and bm_host_reproject agree bit for bit (csrc/reproject.h
 * holds the rules once).
 * A HISTORY of a width x height image is one buffer, 16-byte aligned: width * height float4 (R, G, B, n) row-major -- an accumulation
 * buffer, which bm_denoise and bm_resolve take unchanged -- then width * height uint32 surface keys: 20 bytes per pixel.
 * Both cameras' bases (origin o, dir D, right Rt, up U) are those of the frames for this width and height; for the previous camera
 * (marked ') also dd = (D.x*D.x + D.y*D.y) + D.z*D.z, and rr, uu likewise for Rt, U.  Per pixel p = (x, y):
 *  1. key_p = the denoise's surface key of (accum n, hit); history_out.key[p] = key_p always.
 *  2. without history_prev, or with the special key: history_out.image[p] = accum[p], all four words unchanged ("no history").
 *  3. dhat = the direction of bm_camera_pixel_rays for (x + 0.5, y + 0.5); P[k] = o[k] + dhat[k] * distance.
 *  4. e[k] = P[k] - o'[k]; t = ((e.x*D'.x + e.y*D'.y) + e.z*D'.z) / dd; !(t > 0): no history.  a = ((e.x*Rt'.x + e.y*Rt'.y) + e.z*Rt'.z) / (t * rr),
 *     b likewise with U', uu.  u = (a + 0.5) * W + 0.5, v = (H - (b + 0.5) * H) + 0.5: continuous coordinates in which pixel centres
 *     are integers.
 *  5. x0f = floor(u), fx = u - x0f, y0f = floor(v), fy = v - y0f; !(x0f >= -1 && x0f <= W - 1 && y0f >= -1 && y0f <= H - 1), tested in
 *     float: no history.  Four taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with weights (1-fx)*(1-fy), fx*(1-fy), (1-fx)*fy,
 *     fx*fy.  A tap counts when it lies inside the image, prev.key[q] == key_p, prev.n[q] > 0 and its weight > 0; any other tap is skipped,
 *     not multiplied by zero.  From 0 in tap order: Ws += w, C += w * (prev.rgb[q] / prev.n[q]), N += w * prev.n[q].
 *  6. no tap counted: no history.  Else c_h = C / Ws, n_h = N / Ws, n_h = n_h < max_history ? n_h : max_history,
 *     out.rgb = c_h * n_h + accum.rgb (a multiply, then an add), out.n = n_h + accum.n.
 * So a surface that was hidden, off-screen or behind the previous camera starts again at the frame's own samples.  A moved sun, or an
 * edit that changes the light without changing keys, is the caller's reason to pass a NULL history_prev. */
typedef struct bm_reproject_params {
	int32_t width, height;
	float max_history;    /* finite, >= 1: the most samples a pixel takes over from the history; 32 is a good default */
	uint32_t flags;       /* 0 */
	uint32_t reserved;    /* 0 */
} bm_reproject_params;
/* bytes of a history: 20 per pixel */
BM_API int bm_history_bytes(int width, int height, size_t* bytes);
/* accum_dev: the frame just rendered with `camera`, width * height float4 (R, G, B, n); hits_dev: one bm_ray_hit per pixel for that
 * camera's pixel-centre rays (what bm_denoise takes); history_prev_dev: the history of the frame before, made with camera_prev, or NULL
 * (camera_prev may then be NULL too); history_out_dev: the new history.  Asynchronous on hip_stream like bm_denoise; the scene keeps no
 * state, so calls on different streams are independent.  Refused with BM_EINVAL, launching nothing: width or height < 1 or > 65535,
 * max_history not finite or < 1, non-zero flags or reserved, a NULL camera, accum, hits or history_out, a NULL camera_prev with a
 * history_prev, a buffer that is not 16-byte aligned, history_out overlapping history_prev, accum or hits (taps read neighbours: the
 * caller ping-pongs two histories).  A degenerate camera (dir parallel to up) is not refused: its NaNs fail every comparison, which
 * gives "no history". */
BM_API int bm_reproject(bm_scene* scene, const bm_reproject_params* params, const bm_camera* camera, const bm_camera* camera_prev,
                        const float* accum_dev, const bm_ray_hit* hits_dev, const void* history_prev_dev, void* history_out_dev, void* hip_stream);
/* the same on host memory, as plain loops (no device needed); the refusals of bm_reproject that concern params and NULL pointers */
BM_API int bm_host_reproject(const bm_reproject_params* params, const bm_camera* camera, const bm_camera* camera_prev, const float* accum,
                             const bm_ray_hit* hits, const void* history_prev, void* history_out);

/* ---- volume queries against the live scene (no reference counterpart): how much is solid in a box or a sphere, and where.
 * Is this box free, how much does this sphere hold, where is the ground under this column, how far can this box move before it
 * touches something -- questions a ray, which has no width, answers badly.  For each of n records in device memory: the number of
 * solid voxels inside the shape, their tight bounding box, and how many brick cells could not be answered.  All integers, all exact.
 *  - The shape is clipped to the world exactly like an edit's shape; one wholly outside gives zeros and -1 bounds, and so does an
 *    empty box.  Per brick cell, with cover = the clipped shape's voxels in the cell: a resident cell (the device index word has
 *    BM_BRICK_LOADED_BIT; the brick is at arena[pool_base + slot]) contributes popcount(brick & cover) and the bounds of those bits;
 *    a cell that is empty in the world contributes nothing; a cell that holds a brick which is not resident adds 1 to `unresolved`,
 *    provided cover is not empty.  In a preloaded scene unresolved is always 0 and the answer is exact.
 *  - BM_VOLUME_ANY: a yes / no probe that may stop early.  solid = 1 if any solid voxel would be counted, else 0; the bounds are all
 *    -1; unresolved = 1 if solid == 0 and at least one cell was unresolved, else 0 -- whatever the order of evaluation.
 *  - Malformed records are marked, not refused (the records live in device memory and the call stays asynchronous, as for
 *    bm_ray.reserved): status = 1, solid = 0, bounds -1, unresolved = 0 for an unknown shape, a box with hi < lo on an axis, a
 *    sphere with radius < 0 (the checks of bm_scene_edit), or reserved != 0.  Other records are not affected.
 *  - The call writes every byte of every result record.  It files no brick request and writes no index word: it only reads the world.
 *  - Ordering: issued like a ray query on hip_stream -- it sees every edit, region write and upload issued before it, on any
 *    stream; later edits and bm_scene_process_load_queue order themselves behind it; asynchronous to the host.  Volume queries of one
 *    scene run one after another, also when issued on different streams (they share the temporary memory below).
 *  - n == 0 is a no-op.  n < 0, n > 2^24, NULL buffers, unknown flag bits, volumes_dev not 4-byte or results_dev not 8-byte aligned:
 *    BM_EINVAL; a scene not on the device, or a failed one: BM_ESTATE.  Nothing is launched on an error.
 *  - Temporary device memory: 8 bytes per record and 8 per 256 records (at least 64 KiB; 128.5 MiB for 2^24 records), kept and
 *    grown on demand. */
typedef struct bm_volume {        /* 48 bytes -- the shape part of bm_edit, same meaning field by field */
	int32_t shape;                /* BM_EDIT_BOX / BM_EDIT_SPHERE */
	int32_t lo[3], hi[3];         /* box: lo <= v < hi */
	int32_t center[3];            /* sphere: sum (v - center)^2 <= radius^2, 64-bit integers, as bm_edit */
	int32_t radius;
	uint32_t reserved;            /* 0 */
} bm_volume;
typedef struct bm_volume_result { /* 40 bytes */
	uint64_t solid;               /* solid voxels of the shape, clipped to the world, in resident bricks */
	int32_t lo[3], hi[3];         /* tight half-open bounds of those voxels; all six -1 when solid == 0 */
	uint32_t unresolved;          /* brick cells that hold a brick in the world, contain a voxel of the clipped shape, and are not resident */
	uint32_t status;              /* 0 ok; 1 malformed record (then solid = 0, bounds -1, unresolved = 0) */
} bm_volume_result;
#define BM_VOLUME_ANY 1u
BM_API int bm_scene_query_volumes(bm_scene* scene, int64_t n, const bm_volume* volumes_dev, bm_volume_result* results_dev, uint32_t flags,
                                  void* hip_stream);

/* ---- connected components of a box of the live scene (no reference counterpart): which voxels hang together.  Carve a tunnel through a
 * pillar and its top stays in the air; these calls say so, how big the piece is and which voxels belong to it.  All integers, all exact.
 * For a half-open box lo <= v < hi with (nx, ny, nz) = hi - lo, bm_scene_label_region fills a tight int32 volume labels[z][y][x].
 *  - Occupancy is exactly what bm_scene_read_region gives for the box: voxels outside the world are empty; in a streaming scene the
 *    bricks the device does not hold are taken from the host world by the read route's staging; a preloaded scene stages nothing and the
 *    call is asynchronous to the host.
 *  - Connectivity is by faces (6 neighbours), inside the box only: voxels that touch along an edge or at a corner are not joined, and
 *    voxels outside the box join nothing.
 *  - The label of an empty voxel is 0; the label of a solid voxel is 1 + index(first voxel of its component), with
 *    index(x, y, z) = ((z - lo.z) * ny + (y - lo.y)) * nx + (x - lo.x) and "first" the smallest index.  This does not depend on
 *    scheduling: two runs give identical bytes.
 *  - *count_dev (a uint64 in device memory) receives the number of components.
 *  - Refused with BM_EINVAL, nothing launched: hi < lo on an axis; nx * ny * nz > 2^31 - 2 (computed in 64 bits); flags other than 0 (18- and
 *    26-connectivity do not exist); a null buffer; labels_dev not 4-byte aligned, or its span not inside one allocation of the scene's
 *    device; count_dev not 8-byte aligned (or not memory of that device).  A scene not on the device, or a failed one: BM_ESTATE.
 *  - An empty box (hi == lo on some axis) writes count 0 and is otherwise a no-op.
 *  - Ordering: issued like a query on hip_stream.  It sees every edit, region write and upload issued before it; later edits and
 *    bm_scene_process_load_queue order themselves behind it.  It files no request and writes no index word.
 *  - Temporary device memory is the scene's, kept and grown on demand: none per voxel -- the label volume is the parent array of the
 *    union-find while the call runs (csrc/label.h) -- 8 bytes per 1024 voxels for bm_scene_label_components, and the list of non-resident
 *    bricks of a streaming scene.  Label calls of one scene run one after another, also when issued on different streams.
 * The component table: one record per component, in ascending label. */
typedef struct bm_component {   /* 40 bytes */
	int32_t  label;
	uint32_t faces;             /* bit 0 ... 5: has a voxel on the -x, +x, -y, +y, -z, +z face of (box intersected with the world) */
	uint64_t voxels;
	int32_t  lo[3], hi[3];      /* tight half-open bounds, world voxel coordinates */
} bm_component;
BM_API int bm_scene_label_region(bm_scene* scene, const int32_t lo[3], const int32_t hi[3], uint32_t flags, int32_t* labels_dev, uint64_t* count_dev,
                                 void* hip_stream);
/* The table of a label volume made by bm_scene_label_region for the same box: the first min(capacity, count) records in ascending label;
 * records past that are left untouched, and voxels of components beyond the capacity contribute nothing.  comps_dev: 8-byte aligned,
 * min(capacity, nx * ny * nz) records inside one allocation.  It reads only the label volume, not the world, so it is ordered by
 * hip_stream alone (and behind the scene's previous label call).  An empty box or capacity 0 is a no-op. */
BM_API int bm_scene_label_components(bm_scene* scene, const int32_t lo[3], const int32_t hi[3], const int32_t* labels_dev, bm_component* comps_dev,
                                     int64_t capacity, void* hip_stream);
/* mask_dev[z][y][x] (tight, one byte per voxel: what bm_scene_write_region / bm_scene_read_region take) = chosen_dev[slot] where the voxel's
 * label is that of record `slot` of the n records at comps_dev; 0 for empty voxels and for labels not in the table.  chosen is the
 * caller's choice per record: by faces, by size, by anything computed on the small table. */
BM_API int bm_scene_label_mask(bm_scene* scene, const int32_t lo[3], const int32_t hi[3], const int32_t* labels_dev, const bm_component* comps_dev,
                               int64_t n, const uint8_t* chosen_dev, uint8_t* mask_dev, void* hip_stream);
/* device times of the last bm_scene_label_region that launched its kernels, in ms (hipEvents on its stream; waits for it): the
 * in-brick labelling, the merge across cell faces, and flatten + count.  BM_ESTATE when there was none. */
BM_API int bm_scene_last_label_ms(bm_scene* scene, float* local_ms, float* merge_ms, float* flatten_ms);
/* the same labelling of a dense host volume voxels[z][y][x] (non-zero = solid, tight) in plain loops, no device needed (csrc/label_host.cpp,
 * by the rules of csrc/label.h): labels as above, *count = the number of components.  BM_EINVAL for a negative extent, more than 2^31 - 2
 * voxels or a null pointer. */
BM_API int bm_host_label_volume(const uint8_t* voxels, int64_t nx, int64_t ny, int64_t nz, int32_t* labels, uint64_t* count);

/* ---- triangle meshes -> voxels (no reference counterpart): a triangle soup in device memory -- n x 9 floats, xyz per vertex, in world
 * voxel units -- fills a dense byte volume V[z][y][x] with 0 / 1: the volume bm_scene_write_region takes (voxel [0][0][0] at world voxel
 * lo, x contiguous, rows and slices at the given pitches).  Integers only after the snap, the same bytes on every run, and bm_voxelize ==
 * bm_host_voxelize byte for byte (csrc/voxelize.h holds the rules once).  S = 256.
 *  - Snap.  A triangle with a coordinate v whose fp32 product v * 256 is not finite or above 2^30 in magnitude is REJECTED.  Otherwise
 *    q = rint(v * 256.0f) (an exact product, rounded half to even) as an integer, minus 256 * lo.  A triangle is also rejected when
 *    any |q| > 2^22 or when max q - min q on an axis exceeds 2^19 (2048 voxels).  Within these bounds every expression below fits 64
 *    bits: |n| < 2^40, |n . d| < 2^62.
 *  - Normal.  n = (q1 - q0) x (q2 - q0); n == 0: the triangle is DEGENERATE and skipped.
 *  - BM_VOXELIZE_SURFACE marks every voxel whose closed cube meets the triangle (conservative: nothing leaks through).  Voxel k stands
 *    for the cube [k S, (k + 1) S]^3 and is set when all three hold:
 *      1. per axis a: k_a S <= max q_a and (k_a + 1) S >= min q_a;
 *      2. with d = n . (k S - q0): d + sum min(n_a S, 0) <= 0 <= d + sum max(n_a S, 0);
 *      3. for each axis ax, with (u, v) the cyclic other two axes ((y, z), (z, x), (x, y)), sgn = (n_ax >= 0 ? 1 : -1), and for each edge
 *         p0 -> p1 (q0 q1, q1 q2, q2 q0) with e = p1 - p0, a = -e_v sgn, b = e_u sgn:
 *         a (k_u S - p0_u) + b (k_v S - p0_v) + max(a S, 0) + max(b S, 0) >= 0.
 *  - BM_VOXELIZE_SOLID marks every voxel whose centre lies inside the closed mesh, by parity along x.  Only triangles with n_x != 0 take
 *    part; sgn = sign(n_x), (u, v) = (y, z).  Column (y, z) has the centre (U, V) = (256 y + 128, 256 z + 128) and is COVERED by a triangle
 *    when for every edge, with a = -(p1_v - p0_v) sgn, b = (p1_u - p0_u) sgn and E = a (U - p0_u) + b (V - p0_v): E > 0, or E == 0 and
 *    (a > 0, or a == 0 and b > 0) -- so an edge or a vertex that two triangles share counts once.  A covered column has one crossing, at
 *    k = the smallest x with |n_x| (256 x + 128 - q0_x) >= -sgn (n_y (U - q0_y) + n_z (V - q0_z)); k < 0 counts as 0, k >= nx as nx (outside
 *    the volume).  Voxel x is solid when the number of crossings with k <= x is odd.
 *  - Output.  byte = surface | solid as the mode asks (0 or 1); with BM_VOXELIZE_KEEP byte = old | that (non-zero stays non-zero).  Every
 *    byte of the box's rows is written; the bytes between rows and slices are never touched.
 *  - Result (optional, 16 bytes on the device): triangles rejected, degenerate, and open_columns = the columns whose total number of
 *    crossings, those at nx included, is odd -- 0 for a closed mesh: the leak detector (0 without BM_VOXELIZE_SOLID).
 *  - Refusals, BM_EINVAL with nothing launched and nothing written: an extent below 1 or above 16384; a pitch below the extent it spans
 *    (0 = tight) or a volume spanning more than 2^46 bytes; a mode of 0, an unknown mode or flag bit; n < 0 or > 2^30; a null triangle
 *    pointer with n > 0, a null volume or workspace; triangles or the result not 4-byte (8-byte) aligned, a workspace not 16-byte aligned;
 *    a workspace below bm_voxelize_workspace_bytes; a workspace that overlaps the volume, the triangles or the result; a span (volume:
 *    (nz - 1) slice_pitch + (ny - 1) row_pitch + nx bytes) that does not lie inside one allocation of the scene's device. */
#define BM_VOXELIZE_SURFACE 1u
#define BM_VOXELIZE_SOLID 2u
#define BM_VOXELIZE_KEEP 1u /* flag: OR into what the volume holds */
typedef struct bm_voxelize_params {
	int32_t lo[3];       /* world voxel of V[0][0][0], (x, y, z) */
	int32_t extent[3];   /* nx, ny, nz: 1 ... 16384 */
	int64_t row_pitch;   /* bytes from one x-row to the next y; 0 = tight (nx) */
	int64_t slice_pitch; /* bytes from one z-slice to the next; 0 = tight (row_pitch * ny) */
	uint32_t mode;       /* BM_VOXELIZE_SURFACE | BM_VOXELIZE_SOLID, at least one */
	uint32_t flags;      /* 0 or BM_VOXELIZE_KEEP */
} bm_voxelize_params;
typedef struct bm_voxelize_result {
	uint32_t rejected, degenerate;
	uint64_t open_columns;
} bm_voxelize_result;
/* bytes of device memory bm_voxelize needs beside its buffers: two bit planes of ny * nz rows of ceil((nx + 1) / 32) words, and two
 * 64-bit words per triangle and per 256 triangles */
BM_API int bm_voxelize_workspace_bytes(const bm_voxelize_params* params, int64_t n, size_t* bytes);
/* the buffers and the workspace are the caller's and the scene keeps no state (the scene names the device): calls on different streams
 * with workspaces of their own are independent.  Asynchronous on hip_stream; the workspace is zeroed by the call.  Nothing of the world
 * is read. */
BM_API int bm_voxelize(bm_scene* scene, const bm_voxelize_params* params, int64_t n, const float* triangles_dev, uint8_t* volume_dev,
                       bm_voxelize_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream);
/* measuring door: bm_voxelize with a hipEvent between its stages; waits, then kernel_ms[0 ... 4] = the durations in ms of zeroing the
 * workspace, plan + scan, the surface items, the solid items and the dense pass; a stage the mode does not ask for takes 0 */
BM_API int bm_debug_voxelize_times(bm_scene* scene, const bm_voxelize_params* params, int64_t n, const float* triangles_dev, uint8_t* volume_dev,
                                   bm_voxelize_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream, float* kernel_ms);
/* the same on host memory, as plain loops (csrc/voxelize_host.cpp; no device needed); the refusals that concern params and null pointers */
BM_API int bm_host_voxelize(const bm_voxelize_params* params, int64_t n, const float* triangles, uint8_t* volume, bm_voxelize_result* result);

/* ---- voxels -> the quads of their surface (no reference counterpart): the counterpart of bm_voxelize.  A dense byte volume V[z][y][x] in
 * device memory (any non-zero byte is solid; x contiguous, rows and slices at the given pitches, any base alignment; voxel [0][0][0] at
 * world voxel lo) gives the quads of its surface as 16-byte records.  All integers, the same bytes on every run, and bm_mesh_quads ==
 * bm_host_mesh_quads byte for byte (csrc/mesh.h holds the rules once).
 *  - Faces.  A face is a pair (solid voxel p, direction d) whose neighbour p + d is empty; directions 0 ... 5 = -x, +x, -y, +y, -z, +z.
 *    Without flags every voxel outside the volume is empty, so the surface is closed.  With BM_MESH_HALO the outermost one-voxel shell of
 *    the volume is context only: faces are emitted for the voxels with index 1 ... n - 2 on every axis, their neighbours are read from the
 *    shell, and every extent must be at least 3 -- tiles of a larger world meshed this way have no walls between them.
 *  - Cells.  The meshed voxels are cut into the world's 8^3 brick cells: a boundary lies where lo + index is a multiple of 8 (floor
 *    division: lo may be negative); the first and last cell of an axis may be ragged.  Cells are numbered in (z, y, x) order over the
 *    cells the meshed box spans.
 *  - Masks.  Inside a cell, direction d on axis a and slice s = 0 ... 7 (the solid voxel's cell-local coordinate along a) have an 8 x 8
 *    mask: bit 8 v + u is the face at in-slice position (u, v), the other two axes in ascending order -- (y, z) for x, (x, z) for y,
 *    (x, y) for z.
 *  - Greedy cover, until the mask is empty: take the lowest set bit (u0, v0); w = the length of the run of set bits from u0 in row v0 (it
 *    does not pass u = 7); h = 1 + the number of following rows that have all bits u0 ... u0 + w - 1 set; clear the rectangle; emit a
 *    quad.  With BM_MESH_UNIT_FACES w = h = 1 always.  At most 64 rounds.
 *  - Quad.  x, y, z = the world voxel of the quad's lowest solid voxel; shape = d | w << 4 | h << 8.
 *  - Order: by cell, then direction, then slice, then the greedy order -- a total order without a sort.
 *  - Capacity.  The first min(capacity, total) quads are written; records past that are never touched.  capacity == 0 with a null quad
 *    pointer is the counting call.
 *  - Result (16 bytes on the device), always the full totals: quads, and faces = the sum of w h.
 *  - Triangles.  bm_mesh_triangles writes 2 n triangles of 9 floats, the format bm_voxelize reads.  The quad's plane is at coordinate c_a
 *    for a negative direction and c_a + 1 for a positive one; its corners are c00, c10 = c00 + w e_u, c11 and c01 = c00 + h e_v.  If
 *    e_u x e_v points along d the triangles are (c00, c10, c11) and (c00, c11, c01), otherwise (c00, c01, c11) and (c00, c11, c10):
 *    counter-clockwise seen from outside.  A record whose direction is above 5 gives 18 zeros.  Voxelized again with BM_VOXELIZE_SOLID
 *    the triangles of a volume give back the volume, with open_columns == 0.
 *  - Refusals, BM_EINVAL with nothing launched and nothing written: an extent below 1 (below 3 with BM_MESH_HALO) or above 16384; more
 *    than 2^31 - 2 voxels; a pitch below the extent it spans (0 = tight) or a volume spanning more than 2^46 bytes; a span ((nz - 1)
 *    slice_pitch + (ny - 1) row_pitch + nx bytes) or any other buffer that does not lie inside one allocation of the scene's device; an
 *    unknown flag bit or a non-zero `reserved`; a null volume, result or workspace; a null quad pointer with capacity > 0; quads not
 *    4-byte, a result not 8-byte or a workspace not 16-byte aligned; a workspace below bm_mesh_workspace_bytes; a workspace that overlaps
 *    the volume, the quads or the result; a box that does not lie within +-2^23 voxels (every corner is an exact fp32 integer). */
#define BM_MESH_HALO 1u
#define BM_MESH_UNIT_FACES 2u
typedef struct bm_mesh_params {
	int32_t lo[3];       /* world voxel of V[0][0][0], (x, y, z) */
	int32_t extent[3];   /* nx, ny, nz: 1 ... 16384 */
	int64_t row_pitch;   /* bytes from one x-row to the next y; 0 = tight (nx) */
	int64_t slice_pitch; /* bytes from one z-slice to the next; 0 = tight (row_pitch * ny) */
	uint32_t flags;      /* BM_MESH_HALO | BM_MESH_UNIT_FACES */
	uint32_t reserved;   /* 0 */
} bm_mesh_params;
typedef struct bm_quad {
	int32_t x, y, z;
	uint32_t shape; /* d | w << 4 | h << 8 */
} bm_quad;
typedef struct bm_mesh_result {
	uint64_t quads, faces;
} bm_mesh_result;
/* bytes of device memory bm_mesh_quads needs beside its buffers: 4 bytes per cell (rounded up to 16) and 8 per 256 cells, plus 8 */
BM_API int bm_mesh_workspace_bytes(const bm_mesh_params* params, size_t* bytes);
/* the buffers and the workspace are the caller's and the scene keeps no state (the scene names the device): calls on different streams
 * with workspaces of their own are independent.  Asynchronous on hip_stream.  Nothing of the world is read. */
BM_API int bm_mesh_quads(bm_scene* scene, const bm_mesh_params* params, const uint8_t* volume_dev, bm_quad* quads_dev, uint64_t capacity,
                         bm_mesh_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream);
/* n quads (4-byte aligned) -> 2 n triangles of 9 floats (4-byte aligned), each inside one allocation of the scene's device; n <= 2^32 */
BM_API int bm_mesh_triangles(bm_scene* scene, const bm_quad* quads_dev, int64_t n, float* triangles_dev, void* hip_stream);
/* measuring door: bm_mesh_quads with a hipEvent between its stages; waits, then kernel_ms[0 ... 2] = the durations in ms of count, scan
 * and emit (0 for the counting call's emit) */
BM_API int bm_debug_mesh_times(bm_scene* scene, const bm_mesh_params* params, const uint8_t* volume_dev, bm_quad* quads_dev, uint64_t capacity,
                               bm_mesh_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream, float* kernel_ms);
/* the same on host memory, as plain loops (csrc/mesh_host.cpp; no device needed); the refusals that concern params and null pointers */
BM_API int bm_host_mesh_quads(const bm_mesh_params* params, const uint8_t* volume, bm_quad* quads, uint64_t capacity, bm_mesh_result* result);
BM_API int bm_host_mesh_triangles(const bm_quad* quads, int64_t n, float* triangles);

/* ---- voxels -> their exact squared distance to the nearest source (no reference counterpart).  A dense byte volume V[z][y][x] in device
 * memory (any non-zero byte is solid; x contiguous, rows and slices at the given pitches, 0 = tight; any base alignment; extents and voxel
 * limit those of bm_mesh_params: 1 ... 16384 per axis, at most 2^31 - 2 voxels) gives a tight uint32_t field D[z][y][x], 4-byte aligned.
 * All integers, a minimum and therefore unique: the same bytes on every run, and bm_distance_field == bm_host_distance_field byte for
 * byte (csrc/distance.h holds the rules once).
 *  - D(p) = the minimum over all sources q of (px - qx)^2 + (py - qy)^2 + (pz - qz)^2, or BM_DISTANCE_NONE = 0x7FFFFFFF when there is no
 *    source.  The largest finite value is 3 * 16383^2 < 2^30: the field reads as non-negative int32.  A source has D = 0.
 *  - Sources.  Without flags the solid voxels of the volume; with BM_DISTANCE_TO_EMPTY its empty voxels.  With BM_DISTANCE_OUTSIDE every
 *    voxel outside the volume is a source too: the nearest of those is always axis-aligned, so the flag is D = min(D, m^2) with m = the
 *    minimum over the three axes of min(i + 1, n - i), i the voxel's index and n the extent on that axis.
 *  - Result (32 bytes on the device, 8-byte aligned): sources = how many voxels of the volume are sources; max_sq = the largest finite D
 *    (0 when every voxel is a source, BM_DISTANCE_NONE when no value is finite); max_at = the linear index (z ny + y) nx + x of the
 *    lowest-indexed voxel that has that value (0 when there is none); the rest 0.  max_at and max_sq are the centre and the squared
 *    radius of the largest ball of non-sources in the box.
 *  - Mask.  bm_distance_mask writes the tight byte volume out[i] = (D[i] <= limit_sq) ? 1 : 0 -- what bm_scene_write_region takes -- and
 *    with BM_DISTANCE_MASK_ABOVE the opposite.  BM_DISTANCE_NONE is above every limit.  out may begin at any address.
 *  - Refusals, BM_EINVAL with nothing launched and nothing written: an extent below 1 or above 16384; more than 2^31 - 2 voxels; a pitch
 *    below the extent it spans or a volume spanning more than 2^46 bytes; a span ((nz - 1) slice_pitch + (ny - 1) row_pitch + nx bytes) or
 *    any other buffer that does not lie inside one allocation of the scene's device; an unknown flag bit or a non-zero `reserved`; a null
 *    pointer; a field not 4-byte, a result not 8-byte or a workspace not 16-byte aligned; a workspace below bm_distance_workspace_bytes; a
 *    workspace that overlaps the volume, the field or the result; a field that overlaps the volume.  For the mask: a count of 0 or above
 *    2^31 - 2, an unknown flag, a null pointer, a field not 4-byte aligned, an output that overlaps the field. */
#define BM_DISTANCE_TO_EMPTY 1u
#define BM_DISTANCE_OUTSIDE 2u
#define BM_DISTANCE_MASK_ABOVE 1u
#define BM_DISTANCE_NONE 0x7FFFFFFFu
typedef struct bm_distance_params {
	int32_t extent[3];   /* nx, ny, nz: 1 ... 16384 (four bytes of padding follow) */
	int64_t row_pitch;   /* bytes from one x-row to the next y; 0 = tight (nx) */
	int64_t slice_pitch; /* bytes from one z-slice to the next; 0 = tight (row_pitch * ny) */
	uint32_t flags;      /* BM_DISTANCE_TO_EMPTY | BM_DISTANCE_OUTSIDE */
	uint32_t reserved;   /* 0 */
} bm_distance_params;
typedef struct bm_distance_result {
	uint64_t sources;
	uint32_t max_sq, reserved0;
	uint64_t max_at;
	uint64_t reserved1;
} bm_distance_result;
/* bytes of device memory bm_distance_field needs beside its buffers: 4 bytes per voxel for the plane between the line passes and 4 bytes
 * per voxel for the lanes' stacks, each rounded up to 16, plus 32 */
BM_API int bm_distance_workspace_bytes(const bm_distance_params* params, size_t* bytes);
/* the buffers and the workspace are the caller's and the scene keeps no state (the scene names the device): calls on different streams
 * with workspaces of their own are independent.  Asynchronous on hip_stream.  Nothing of the world is read. */
BM_API int bm_distance_field(bm_scene* scene, const bm_distance_params* params, const uint8_t* volume_dev, uint32_t* dist_dev, bm_distance_result* result_dev,
                             void* workspace_dev, size_t workspace_bytes, void* hip_stream);
/* count voxels of a field -> count bytes */
BM_API int bm_distance_mask(bm_scene* scene, uint64_t count, const uint32_t* dist_dev, uint32_t limit_sq, uint32_t flags, uint8_t* volume_out_dev, void* hip_stream);
/* measuring door: bm_distance_field with a hipEvent between its stages; waits, then kernel_ms[0 ... 2] = the durations in ms of the x
 * pass, the y pass and the z pass with the finishing thread */
BM_API int bm_debug_distance_times(bm_scene* scene, const bm_distance_params* params, const uint8_t* volume_dev, uint32_t* dist_dev, bm_distance_result* result_dev,
                                   void* workspace_dev, size_t workspace_bytes, void* hip_stream, float* kernel_ms);
/* the same on host memory, as plain loops (csrc/distance_host.cpp; no device needed); the refusals that concern params and null pointers */
BM_API int bm_host_distance_field(const bm_distance_params* params, const uint8_t* volume, uint32_t* dist, bm_distance_result* result);
BM_API int bm_host_distance_mask(uint64_t count, const uint32_t* dist, uint32_t limit_sq, uint32_t flags, uint8_t* volume_out);

/* ---- voxels + seeds -> exact shortest face-step distances and paths (no reference counterpart).  A dense byte volume V[z][y][x] in device
 * memory (any non-zero byte is blocked; x contiguous, rows and slices at the given pitches, 0 = tight; any base alignment; extents and
 * voxel limit those of bm_distance_params) and n >= 0 seeds, int32 seeds[n][3] = (x, y, z) in device memory (the pointer may be null when
 * n is 0), give a tight uint32_t field T[z][y][x], 4-byte aligned.  All integers, and a breadth-first distance is unique: the same bytes
 * on every run whatever order anything ran in, and bm_travel_field == bm_host_travel_field byte for byte (csrc/travel.h holds the rules
 * once).
 *  - T(p) = the least number of face steps (6-neighbourhood, inside the volume only) from any accepted seed to p through voxels that are
 *    not blocked, or BM_TRAVEL_NONE = 0x7FFFFFFF when p is blocked or unreachable -- and, with max_steps != 0, when p is farther than
 *    max_steps.  max_steps == 0 means no limit.  Every finite value is below 2^31 - 2: the field reads as non-negative int32.
 *  - Seeds.  A seed is accepted when it lies inside the volume on a voxel that is not blocked; the others are counted.  Duplicates are
 *    fine.  An accepted seed has T = 0.
 *  - Result (32 bytes on the device, 8-byte aligned): reached = the voxels with a finite value; farthest = the largest finite value,
 *    BM_TRAVEL_NONE when none is finite; seeds_rejected; farthest_at = the lowest linear index (z ny + y) nx + x that holds `farthest`, 0
 *    when there is none; the rest 0.
 *  - Waiting.  Unlike the other operators bm_travel_field RETURNS WHEN THE FIELD STANDS: it enqueues rounds of relaxation in batches on
 *    hip_stream and between batches waits on that stream for one word, the number of tiles still listed.  It therefore cannot be captured
 *    into a graph.  bm_travel_paths is asynchronous on hip_stream like everything else.
 *  - Paths.  bm_travel_paths takes a field, n >= 0 starts (int32 starts[n][3]), a per-path capacity >= 1, int32 path[n][capacity][3] and
 *    int32 lengths[n].  lengths[q] = T(start) + 1, the voxels of the path with both ends, or 0 when the start is outside the volume or has
 *    no finite value.  The first min(length, capacity) voxels are written: they begin at the start and descend -- from p the next voxel is
 *    the first neighbour in the order -x, +x, -y, +y, -z, +z that lies inside the volume and holds T(p) - 1 -- so a truncated path still
 *    gives an agent its next steps, and a full one ends on a seed.  If no neighbour qualifies the field was not made by bm_travel_field:
 *    the walk stops and lengths[q] = -1.  The loop is bounded by T(start) and by capacity.
 *  - Refusals, BM_EINVAL with nothing launched and nothing written: an extent below 1 or above 16384; more than 2^31 - 2 voxels; a pitch
 *    below the extent it spans or a volume spanning more than 2^46 bytes; a span or any other buffer that does not lie inside one
 *    allocation of the scene's device; a null pointer; a field, seeds, starts, path or lengths not 4-byte, a result not 8-byte or a
 *    workspace not 16-byte aligned; a workspace below bm_travel_workspace_bytes; a workspace that overlaps the volume, the seeds, the field
 *    or the result; a field that overlaps the volume, the seeds or the result; an unknown flag bit (none is defined) or a non-zero
 *    `reserved`; a negative n or one above 2^31 - 1; a capacity below 1; more than 2^40 path voxels (n * capacity); a path or lengths buffer that overlaps the field or the starts. */
#define BM_TRAVEL_NONE 0x7FFFFFFFu
typedef struct bm_travel_params {
	int32_t extent[3];   /* nx, ny, nz: 1 ... 16384 */
	uint32_t max_steps;  /* 0 = no limit */
	int64_t row_pitch;   /* bytes from one x-row to the next y; 0 = tight (nx) */
	int64_t slice_pitch; /* bytes from one z-slice to the next; 0 = tight (row_pitch * ny) */
	uint32_t flags;      /* 0 */
	uint32_t reserved;   /* 0 */
} bm_travel_params;
typedef struct bm_travel_result {
	uint64_t reached;
	uint32_t farthest, seeds_rejected;
	uint64_t farthest_at;
	uint64_t reserved;
} bm_travel_result;
/* bytes of device memory bm_travel_field needs beside its buffers: per 8^3 tile 64 bytes of blocked bits, a round stamp and two work-list
 * entries (each part rounded up to 16), plus 64 */
BM_API int bm_travel_workspace_bytes(const bm_travel_params* params, size_t* bytes);
/* the buffers and the workspace are the caller's, nothing is allocated on the device and the scene keeps no state (the scene names the
 * device).  Nothing of the world is read.  Returns when the field and the result stand (see Waiting). */
BM_API int bm_travel_field(bm_scene* scene, const bm_travel_params* params, const uint8_t* volume_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev,
                           bm_travel_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream);
BM_API int bm_travel_paths(bm_scene* scene, const int32_t extent[3], const uint32_t* field_dev, const int32_t* starts_dev, int64_t n, int32_t capacity, int32_t* path_dev,
                           int32_t* lengths_dev, void* hip_stream);
/* measuring door: bm_travel_field with a hipEvent between its stages and `batch` rounds between two looks of the host (0 = the default);
 * stage_ms[0 ... 2] = the durations in ms of the set-up (fill, bit bricks, seeds), the rounds and the finish; counts[0] = the rounds
 * enqueued, counts[1] = the looks of the host */
BM_API int bm_debug_travel_times(bm_scene* scene, const bm_travel_params* params, const uint8_t* volume_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev,
                                 bm_travel_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream, uint32_t batch, float* stage_ms,
                                 uint32_t* counts);
/* the same on host memory, as plain loops (csrc/travel_host.cpp; no device needed); the refusals that concern params, n, capacity and null pointers */
BM_API int bm_host_travel_field(const bm_travel_params* params, const uint8_t* volume, const int32_t* seeds, int64_t n, uint32_t* field, bm_travel_result* result);
BM_API int bm_host_travel_paths(const int32_t extent[3], const uint32_t* field, const int32_t* starts, int64_t n, int32_t capacity, int32_t* path, int32_t* lengths);

/* ---- rigid settling: floating pieces fall and land (no reference counterpart).  The step between bm_scene_label_components and
 * bm_scene_write_region: the pieces the caller chooses fall straight down, each as one rigid body, until they rest on the floor, on
 * something that does not move, or on each other.  All integers; the answer is unique and does not depend on any order, so the same
 * bytes on every run, and bm_settle == bm_host_settle byte for byte (csrc/settle.h holds the rules once).
 *  - Inputs.  labels_dev: a tight int32 volume L[z][y][x] in device memory, 0 = empty, equal non-zero values = one rigid piece (what
 *    bm_scene_label_region writes, but nothing relies on that).  comps_dev: n >= 0 bm_component records in ascending label, as
 *    bm_scene_label_components writes them (only `label` is read).  chosen_dev: one byte per record.  With n == 0 the three pointers
 *    comps_dev, chosen_dev and drops_dev may be null.  extent = (nx, ny, nz), 1 ... 16384 each, at most 2^31 - 2 voxels.  z is up.
 *  - Who moves.  A solid voxel is MOVING when a binary search of the table (the lower bound of its label, then one comparison) finds
 *    its label at a slot with chosen[slot] != 0.  Every other solid voxel is STATIC, also one whose label is not in the table.  Every
 *    kernel and the host routine use the same search, so a malformed table still gives every label one answer and nothing can fault.
 *  - Contacts.  In a column (x, y), a moving voxel at height z whose nearest solid voxel below lies at z' and carries a different label
 *    -- if there is none, the floor at z' = -1 -- is a contact with gap g = z - z' - 1.  A pair with the same label is no contact: a
 *    piece is rigid.
 *  - Drops.  Every moving piece gets a drop >= 0; static pieces and the floor have drop 0.  The drops are the greatest values with
 *    drop(upper) <= drop(lower) + g for every contact.  That greatest solution exists and is unique: it is the shortest-path distance from
 *    "ground" in the contact graph, whose weights are not negative.  It is finite, at most nz: the voxel under a piece's lowest voxel
 *    belongs to the floor, to a static piece or to a piece that reaches lower.  Interlocked pieces (a hook through a ring) come out with
 *    the drops that keep them apart, a stack comes down as a stack.  No rotation, no sideways motion, no toppling, no friction.
 *    A chosen record at which no voxel's search arrives (a label without voxels, the second of two equal labels) has drop 0.
 *  - THE FLOOR IS THE BOTTOM OF THE VOLUME, wherever the caller took it from: a box that ends above the world's ground lets pieces land
 *    in mid-air at its lowest slice.  Take the box down to the ground.
 *  - Outputs.  out_dev[z][y][x], a tight uint8 volume (what bm_scene_write_region's replace takes): zeroed, then every solid voxel at z
 *    writes out[z - drop] = 1 when its drop is 0, 2 when it arrived by falling.  The order within a column is kept and the new gaps are
 *    g + drop(lower) - drop(upper) >= 0: no two voxels land on one and none lands below 0.  drops_dev[n]: int32 per record, 0 for records
 *    not chosen.  result_dev: the 32 bytes of a bm_settle_result.  `contacts` counts the contacts as defined above (one per such pair of
 *    voxels): a fact of the geometry, the same on every run.  The number of rounds is not in the record: it may differ between runs.
 *  - Waiting.  Like bm_travel_field the call RETURNS WHEN THE RESULT STANDS: it enqueues rounds of relaxation in batches on hip_stream
 *    and between batches waits on that stream for one small copy.  It cannot be captured into a graph.
 *  - Refusals, BM_EINVAL with nothing launched and nothing written: an extent below 1 or above 16384; more than 2^31 - 2 voxels; a
 *    negative n or one above 2^31 - 2; a null pointer (but see n == 0); labels, drops or workspace not 4-byte aligned, records or result
 *    not 8-byte aligned; a buffer that does not lie inside one allocation of the scene's device; a workspace below
 *    bm_settle_workspace_bytes; flags other than 0; out overlapping labels; a workspace overlapping anything else. */
typedef struct bm_settle_result {   /* 32 bytes */
	uint64_t moved_voxels;          /* the 2s of out */
	uint32_t chosen_pieces;         /* records with chosen != 0 */
	uint32_t moved_pieces;          /* of those, with drop > 0 */
	uint32_t largest_drop;
	uint32_t reserved;              /* 0 */
	uint64_t contacts;
} bm_settle_result;
/* bytes of device memory bm_settle needs beside its buffers: 4 per record, 4 per 64 columns (x, y) (each part rounded up to 16), plus 72.
 * Bytes per piece and per column group, none per voxel. */
BM_API int bm_settle_workspace_bytes(const int32_t extent[3], int64_t n, size_t* bytes);
/* the buffers and the workspace are the caller's, nothing is allocated on the device and the scene keeps no state (the scene names the
 * device).  Nothing of the world is read.  Returns when out, the drops and the result stand (see Waiting). */
BM_API int bm_settle(bm_scene* scene, const int32_t extent[3], const int32_t* labels_dev, const bm_component* comps_dev, int64_t n, const uint8_t* chosen_dev,
                     uint8_t* out_dev, int32_t* drops_dev, bm_settle_result* result_dev, void* workspace_dev, size_t workspace_bytes, uint32_t flags, void* hip_stream);
/* measuring door: bm_settle with a hipEvent between its stages and `batch` rounds between two looks of the host (0 = the default);
 * stage_ms[0 ... 2] = the durations in ms of the set-up, the rounds and the move (with the finish); counts[0] = the rounds enqueued,
 * counts[1] = the looks of the host */
BM_API int bm_debug_settle_times(bm_scene* scene, const int32_t extent[3], const int32_t* labels_dev, const bm_component* comps_dev, int64_t n, const uint8_t* chosen_dev,
                                 uint8_t* out_dev, int32_t* drops_dev, bm_settle_result* result_dev, void* workspace_dev, size_t workspace_bytes, uint32_t flags,
                                 void* hip_stream, uint32_t batch, float* stage_ms, uint32_t* counts);
/* the same on host memory, as plain loops (csrc/settle_host.cpp; no device needed); the refusals that concern the extents, n and null pointers */
BM_API int bm_host_settle(const int32_t extent[3], const int32_t* labels, const bm_component* comps, int64_t n, const uint8_t* chosen, uint8_t* out, int32_t* drops,
                          bm_settle_result* result);

/* ---- ground navigation: exact walk fields and paths for an agent on foot (no reference counterpart).  bm_travel_field answers "how do I
 * get there" for something that flies; these three answer it for something that stands on solid ground, is taller than one voxel, climbs a
 * step but not a wall, drops off a ledge it could never climb back, and bumps its head under a lintel.  All integers; every move costs 1, a
 * breadth-first distance in a directed graph of unit moves is unique, so the same bytes on every run whatever order anything ran in, and
 * bm_foot_* == bm_host_foot_* byte for byte (csrc/foot.h holds the rules once).
 *  - Input.  A dense byte volume V[z][y][x] in device memory: any non-zero byte is blocked, z is up; x contiguous, rows and slices at
 *    the given pitches, 0 = tight; any base alignment; extents and voxel limit those of bm_travel_params.  Only bm_foot_room reads it.
 *  - Room byte.  bm_foot_room writes a tight byte volume room[z][y][x].  Low 7 bits R: 0 for a blocked voxel, otherwise the number of
 *    consecutive free voxels from this one upwards, capped at 127.  Everything ABOVE the volume counts as free, so a free run that reaches
 *    the top is 127.  Bit 7, supported: set when the voxel is free and the voxel below it is blocked; at z = 0 it is set when the voxel is
 *    free, unless BM_FOOT_NO_FLOOR is given.  THE FLOOR IS THE BOTTOM OF THE BOX, as in bm_settle; the flag is for boxes that end above the
 *    ground.  The byte does not depend on the agent (height, climb, drop, max_steps and BM_FOOT_TOWARD are validated and otherwise unused).
 *  - Stand.  With height h in 1 ... 32 a voxel p is a STAND when it is supported and R(p) >= h.
 *  - Move.  p -> q is legal when q lies in one of the four columns (x +- 1, y), (x, y +- 1) inside the volume, p and q are both stands,
 *    -drop <= z(q) - z(p) <= climb with climb in 0 ... 32 and drop in 0 ... 64, and the LOWER of the two has R >= h + |dz|: the agent rises
 *    or falls in the lower voxel's column through free voxels and crosses sideways at the upper height.  Every move costs 1.  No
 *    diagonals.  Since h + 64 <= 96 < 127 the cap on R never decides a move.
 *  - Field.  bm_foot_field takes the room volume and n >= 0 seeds, int32 seeds[n][3] = (x, y, z) (the pointer may be null when n is 0),
 *    and gives a tight uint32_t field W[z][y][x], 4-byte aligned.  With flags 0, W(p) is the least number of moves of a walk from an
 *    accepted seed to p; with BM_FOOT_TOWARD the least number of moves from p to a seed (the same search with climb and drop exchanged).
 *    W(p) is BM_FOOT_NONE = 0x7FFFFFFF where p is no stand, where p is unreachable, and where p lies beyond max_steps (0 = no limit).  A
 *    seed is accepted when it lies inside the volume on a stand; the others are counted.  Duplicates are fine.  BM_FOOT_NO_FLOOR is
 *    ignored here: the room bytes carry it.
 *  - Result (32 bytes on the device, 8-byte aligned): reached = the voxels with a finite value; farthest = the largest finite value,
 *    BM_FOOT_NONE when none is finite; seeds_rejected; farthest_at = the lowest linear index (z ny + y) nx + x that holds `farthest`, 0
 *    when there is none; standable = the number of stands.
 *  - Paths.  bm_foot_paths takes the params, the room, a field, n >= 0 starts (int32 starts[n][3]), a per-path capacity >= 1,
 *    int32 path[n][capacity][3] and int32 lengths[n].  lengths[q] = W(start) + 1, or 0 when the start is outside the volume or has no
 *    finite value.  The first min(length, capacity) voxels are written, the start first: from p the next voxel is the first q that holds
 *    W(p) - 1 and whose move is legal, the columns in the order -x, +x, -y, +y and inside a column in ascending z.  Legal means p -> q with
 *    BM_FOOT_TOWARD and q -> p without it: without the flag the written path is the walk reversed.  If no q qualifies the walk stops and
 *    lengths[q] = -1.  The walk is bounded by W(start) and capacity; a truncated path keeps its first voxels.
 *  - Waiting.  bm_foot_room and bm_foot_paths are asynchronous on hip_stream like everything else.  Like bm_travel_field, bm_foot_field
 *    RETURNS WHEN THE FIELD STANDS: it enqueues rounds in batches on hip_stream and between batches waits on that stream for one word, the
 *    size of the next front.  It therefore cannot be captured into a graph.
 *  - Refusals, BM_EINVAL with nothing launched and nothing written: those of bm_travel_field and bm_travel_paths (extents, voxels,
 *    pitches, spans, null pointers, alignment -- field, seeds, starts, path, lengths 4-byte, result 8-byte, workspace 16-byte --, a workspace
 *    below bm_foot_workspace_bytes, the overlaps, n, capacity, n * capacity); a height outside 1 ... 32, a climb outside 0 ... 32, a drop
 *    outside 0 ... 64; a flag bit other than the two, a non-zero `reserved` or `reserved2`; a room volume that overlaps the byte volume,
 *    the field, the workspace, the result, the path or the lengths. */
#define BM_FOOT_NONE 0x7FFFFFFFu
#define BM_FOOT_TOWARD 1u   /* bm_foot_field, bm_foot_paths: W counts the moves from p to a seed */
#define BM_FOOT_NO_FLOOR 2u /* bm_foot_room: the bottom of the volume does not support */
typedef struct bm_foot_params { /* begins with the 40 bytes of a bm_travel_params */
	int32_t extent[3];   /* nx, ny, nz: 1 ... 16384 */
	uint32_t max_steps;  /* 0 = no limit */
	int64_t row_pitch;   /* of the byte volume: bytes from one x-row to the next y; 0 = tight (nx) */
	int64_t slice_pitch; /* bytes from one z-slice to the next; 0 = tight (row_pitch * ny) */
	uint32_t flags;      /* BM_FOOT_TOWARD | BM_FOOT_NO_FLOOR */
	uint32_t reserved;   /* 0 */
	int32_t height;      /* 1 ... 32 */
	int32_t climb;       /* 0 ... 32 */
	int32_t drop;        /* 0 ... 64 */
	int32_t reserved2;   /* 0 */
} bm_foot_params;
typedef struct bm_foot_result {
	uint64_t reached;
	uint32_t farthest, seeds_rejected;
	uint64_t farthest_at;
	uint64_t standable;
} bm_foot_result;
/* bytes of device memory bm_foot_field needs beside its buffers: the queue, 4 bytes for each of ceil(nz / 2) * ny * nx entries -- a
 * column holds at most that many stands, and a stand enters the queue once -- rounded up to 16, plus 64.  At most 2 bytes per voxel. */
BM_API int bm_foot_workspace_bytes(const bm_foot_params* params, size_t* bytes);
/* the buffers and the workspace are the caller's, nothing is allocated on the device and the scene keeps no state (the scene names the
 * device).  Nothing of the world is read. */
BM_API int bm_foot_room(bm_scene* scene, const bm_foot_params* params, const uint8_t* volume_dev, uint8_t* room_dev, void* hip_stream);
/* returns when the field and the result stand (see Waiting) */
BM_API int bm_foot_field(bm_scene* scene, const bm_foot_params* params, const uint8_t* room_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev,
                         bm_foot_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream);
BM_API int bm_foot_paths(bm_scene* scene, const bm_foot_params* params, const uint8_t* room_dev, const uint32_t* field_dev, const int32_t* starts_dev, int64_t n,
                         int32_t capacity, int32_t* path_dev, int32_t* lengths_dev, void* hip_stream);
/* measuring door: bm_foot_field with a hipEvent between its stages and `batch` rounds between two looks of the host (0 = the default);
 * stage_ms[0 ... 2] = the durations in ms of the set-up (fill, count of stands, seeds), the rounds and the finish; counts[0] = the rounds
 * enqueued, counts[1] = the looks of the host */
BM_API int bm_debug_foot_times(bm_scene* scene, const bm_foot_params* params, const uint8_t* room_dev, const int32_t* seeds_dev, int64_t n, uint32_t* field_dev,
                               bm_foot_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream, uint32_t batch, float* stage_ms,
                               uint32_t* counts);
/* the same on host memory, as plain loops (csrc/foot_host.cpp; no device needed); the refusals that concern params, n, capacity and null pointers */
BM_API int bm_host_foot_room(const bm_foot_params* params, const uint8_t* volume, uint8_t* room);
BM_API int bm_host_foot_field(const bm_foot_params* params, const uint8_t* room, const int32_t* seeds, int64_t n, uint32_t* field, bm_foot_result* result);
BM_API int bm_host_foot_paths(const bm_foot_params* params, const uint8_t* room, const uint32_t* field, const int32_t* starts, int64_t n, int32_t capacity, int32_t* path,
                              int32_t* lengths);

/* ---- where water stands: exact spill levels and pools of a voxel volume (no reference counterpart).  WHAT THIS IS: water stands wherever
 * it could not run off, if it were supplied.  The field does not model how much rain reaches a cave or whether trapped air stops it, nor
 * finite amounts of water: every basin is full to its lowest rim.  All integers; a spill level is a minimum of integers and therefore
 * unique, so the same bytes on every run whatever order anything ran in, and bm_water_field == bm_host_water_field byte for byte
 * (csrc/water.h holds the rules once).
 *  - Input.  A dense byte volume V[z][y][x] in device memory: any non-zero byte is solid, z is up; x contiguous, rows and slices at the
 *    given pitches, 0 = tight; any base alignment; extents and voxel limit those of bm_travel_params.
 *  - Outlets.  The free voxels that lie on the OPEN faces of the box: flags bit 0 ... 5 opens the -x, +x, -y, +y, -z, +z face (the bits of
 *    bm_component.faces).  And the accepted DRAINS: n >= 0 drains, int32 drains[n][3] = (x, y, z) in device memory (the pointer may be
 *    null when n is 0); a drain inside the volume on a free voxel is accepted, the others are counted.  Duplicates are fine.  With no open
 *    face and no accepted drain nothing is an outlet.
 *  - Field.  A tight uint32_t field L[z][y][x], 4-byte aligned.  For a free voxel p with a face-connected path of free voxels
 *    (6-neighbourhood, inside the volume only) to an outlet, L(p) = max(sea_level, the least over all such paths of the largest z on the
 *    path); p and the outlet both count as on the path.  sea_level is in box-local z, 0 = none.  L(p) = BM_WATER_NONE = 0x7FFFFFFF where p
 *    is solid, or CLOSED: free, but with no path to an outlet.  Always L(p) >= z(p).  p is DRY when L(p) == z(p): water in it runs off
 *    without rising.  p is WET when z(p) < L(p) < BM_WATER_NONE: the surface of its pool is the bottom of slice L(p), and L(p) - z(p) is
 *    the depth.
 *  - Result (32 bytes on the device, 8-byte aligned): wet = the wet voxels; deepest = the largest depth, 0 when nothing is wet;
 *    drains_rejected; deepest_at = the lowest linear index (z ny + y) nx + x that holds `deepest`, 0 when nothing is wet; closed = the
 *    closed voxels.
 *  - Mask.  bm_water_mask takes a field and min_depth >= 1 and writes the tight byte volume that bm_scene_write_region and bm_mesh_quads
 *    take: 1 where the voxel is wet and L - z >= min_depth, otherwise 0.  The mask may not overlap the field.  Asynchronous on hip_stream.
 *  - Waiting.  Like bm_travel_field, bm_water_field RETURNS WHEN THE FIELD STANDS: it enqueues rounds of relaxation in batches on
 *    hip_stream and between batches waits on that stream for one word, the number of tiles still listed.  It therefore cannot be captured
 *    into a graph.
 *  - Refusals, BM_EINVAL with nothing launched and nothing written: those of bm_travel_field (extents, voxels, pitches, a non-zero
 *    `reserved`, spans, null pointers, alignment -- field and drains 4-byte, result 8-byte, workspace 16-byte --, a workspace below
 *    bm_water_workspace_bytes, the overlaps among volume, drains, field, result and workspace, n); a flag bit other than the six; a
 *    sea_level above extent[2]; a min_depth below 1; a mask that overlaps the field. */
#define BM_WATER_NONE 0x7FFFFFFFu
typedef struct bm_water_params { /* the 40 bytes of a bm_travel_params, with sea_level where max_steps is */
	int32_t extent[3];   /* nx, ny, nz: 1 ... 16384 */
	uint32_t sea_level;  /* box-local z, 0 ... nz; 0 = none */
	int64_t row_pitch;   /* bytes from one x-row to the next y; 0 = tight (nx) */
	int64_t slice_pitch; /* bytes from one z-slice to the next; 0 = tight (row_pitch * ny) */
	uint32_t flags;      /* bit 0 ... 5: the -x, +x, -y, +y, -z, +z face of the box is open */
	uint32_t reserved;   /* 0 */
} bm_water_params;
typedef struct bm_water_result {
	uint64_t wet;
	uint32_t deepest, drains_rejected;
	uint64_t deepest_at;
	uint64_t closed;
} bm_water_result;
/* bytes of device memory bm_water_field needs beside its buffers: what bm_travel_workspace_bytes gives for the same extents */
BM_API int bm_water_workspace_bytes(const bm_water_params* params, size_t* bytes);
/* the buffers and the workspace are the caller's, nothing is allocated on the device and the scene keeps no state (the scene names the
 * device).  Nothing of the world is read.  Returns when the field and the result stand (see Waiting). */
BM_API int bm_water_field(bm_scene* scene, const bm_water_params* params, const uint8_t* volume_dev, const int32_t* drains_dev, int64_t n, uint32_t* field_dev,
                          bm_water_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream);
BM_API int bm_water_mask(bm_scene* scene, const int32_t extent[3], const uint32_t* field_dev, uint32_t min_depth, uint8_t* mask_dev, void* hip_stream);
/* measuring door: bm_water_field with a hipEvent between its stages and `batch` rounds between two looks of the host (0 = the default);
 * stage_ms[0 ... 2] = the durations in ms of the set-up (fill, bit bricks, outlets, drains), the rounds and the finish; counts[0] = the
 * rounds enqueued, counts[1] = the looks of the host, counts[2] = the tile visits (the sum of the rounds' list lengths) */
BM_API int bm_debug_water_times(bm_scene* scene, const bm_water_params* params, const uint8_t* volume_dev, const int32_t* drains_dev, int64_t n, uint32_t* field_dev,
                                bm_water_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream, uint32_t batch, float* stage_ms,
                                uint32_t* counts);
/* the same on host memory, as a plain priority flood (csrc/water_host.cpp; no device needed); the refusals that concern params, n, min_depth and null pointers */
BM_API int bm_host_water_field(const bm_water_params* params, const uint8_t* volume, const int32_t* drains, int64_t n, uint32_t* field, bm_water_result* result);
BM_API int bm_host_water_mask(const int32_t extent[3], const uint32_t* field, uint32_t min_depth, uint8_t* mask);

/* host-only world-build doors (no device needed): the terrain generator behind Scene::generate */
BM_API int bm_host_column_heights(int grid_size, int grid_height, int sx, int sy, float* heights128x128);
BM_API int bm_host_generate_supercell(int grid_size, int grid_height, int sx, int sy, int sz, uint32_t* indices4096,
                                      uint32_t* brick_count, uint32_t* bricks, uint32_t brick_capacity);
/* the host half of bm_scene_edit on one supercell's arrays, in place (no device needed): indices4096 and bricks[*brick_count][16]
 * as bm_host_generate_supercell returns them; a slot that no index word names is free and reused first.  *brick_count may grow
 * (up to brick_capacity, else BM_EINVAL); on any error the arrays are left unchanged. */
BM_API int bm_host_edit_supercell(int grid_size, int grid_height, int sx, int sy, int sz, uint32_t* indices4096,
                                  uint32_t* brick_count, uint32_t* bricks, uint32_t brick_capacity, int count, const bm_edit* edits);

/* the host half of bm_scene_write_region on one supercell's arrays, in place (no device needed; the arrays as for
 * bm_host_edit_supercell): `voxels` is the region's volume in host memory.  On any error the arrays are left unchanged. */
BM_API int bm_host_write_region_supercell(int grid_size, int grid_height, int sx, int sy, int sz, uint32_t* indices4096,
                                          uint32_t* brick_count, uint32_t* bricks, uint32_t brick_capacity, const bm_region* region, int op,
                                          const uint8_t* voxels);

/* the host route of bm_scene_load_voxels on one supercell (no device needed): voxels is the whole volume of a grid_size x grid_size x
 * grid_height world; indices4096 and bricks[4096][16] receive the supercell's canonical build, *brick_count its bricks */
BM_API int bm_host_load_supercell(int grid_size, int grid_height, int sx, int sy, int sz, const uint8_t* voxels, uint32_t* indices4096,
                                  uint32_t* bricks, uint32_t* brick_count);

/* test door: the constants with which the walk divides a cube-field offset by the slice pitch (floor(n / divisor) ==
 * (uint64(n) * magic >> 32) >> shift for every n < 2^30; 3 <= divisor < 2^23) */
BM_API int bm_debug_division_magic(uint32_t divisor, uint32_t* magic, int* shift);
/* The octant cube field the GPU walk reads instead of index words while it crosses empty space (no reference
 * counterpart: the reference loads one index word per visited cell, voxel.cuh:192-200).  8 planes of
 * (cells+2)^2 x (cells_height+2) bytes, x fastest, one border cell all round; plane o (bit 0 / 1 / 2 = direction
 * negative in x / y / z), cell c: edge (<= 254) of the largest cube of empty brick cells inside the grid with c as
 * its near corner, 0 = the cell holds a brick, 255 = border.  Builds the world on the host; *bytes = size needed
 * (call with field = NULL to query). */
BM_API int bm_host_cube_field(int grid_size, int grid_height, uint8_t* field, size_t capacity, size_t* bytes);

/* ---- State (state.h:5-34): the accumulation ("blit") buffer lives in device memory the
 * caller owns; these helpers exist for callers without their own allocator. */
BM_API int bm_buffer_alloc(int device, size_t bytes, void** dev_ptr);
BM_API int bm_buffer_free(int device, void* dev_ptr);
BM_API int bm_buffer_zero(int device, void* dev_ptr, size_t bytes, void* hip_stream);
BM_API int bm_buffer_read(int device, void* host_dst, const void* dev_src, size_t bytes);
BM_API int bm_buffer_write(int device, void* dev_dst, const void* host_src, size_t bytes);

/* ---- launch_kernels (launch.h:6, kernel.cu:366-439) */
/* rows of the frame owned by this shard */
BM_API int bm_local_rows(const bm_frame_params* params);
/* Adds `spp` paths per pixel into accum_dev (float4 per pixel, local_rows*width, rgb = sum of
 * radiance, a = number of terminated paths; state.h:22, kernel.cu:301,319-322,341-343).
 * debug_dev: NULL or 8 uint32 per pixel (hit records).  hip_stream: the hipStream_t to
 * launch on, used as given (NULL = the device's default stream, like the reference's <<<>>> launches).
 * Asynchronous with respect to the host.
 * Memory and ordering contract: accum_dev (and debug_dev) must be ordinary coarse-grained device memory
 * (hipMalloc / bm_buffer_alloc / a torch CUDA tensor): the wavefront mode accumulates with hardware float
 * atomics, which are not defined on fine-grained or host-mapped allocations.  A scene is not thread-safe.
 * Frames of one scene that accumulate into the SAME buffer may overlap in time (issued on different streams) only
 * with BM_FLAG_SAMPLE_ITEMS, which adds samples with float atomics; without it a pixel is read when a lane takes it
 * and written back when it is done, so such frames must be ordered (one stream, or events).  Every launch has its
 * own ticket counters and constants (a ring of 1024 frames / 256 launches in flight).  Scenes that stream bricks may have frames on
 * several streams as well: every stream is ordered behind the brick uploads it has not seen, and
 * bm_scene_process_load_queue orders itself behind the frames of all of them.  Width and height are limited to 65535, a
 * shard to 2^32 pixels. */
BM_API int bm_render_frame(bm_scene* scene, const bm_camera* camera, const bm_frame_params* params,
                           float* accum_dev, uint32_t* debug_dev, void* hip_stream);
/* The reference's frame loop -- launch_kernels once per frame, main.cpp:117-147 / kernel.cu:416-420 -- for `count` (1 ... 256)
 * consecutive frames as ONE launch of the persistent kernel (the "frame ring", csrc/trace.hip): frame i is exactly
 * bm_render_frame(scene, &cameras[i], &params[i], accum_dev[i], debug_dev ? debug_dev[i] : NULL), but a wave that finds frame i's
 * ticket counters used up finishes its own paths and starts on frame i+1 by itself, so the end of a frame -- the latency of the
 * paths that started last, a sixth of a 1080p / 1-spp frame -- is covered by the beginning of the next one instead of an idle GPU
 * (1080p / 1 spp: 1.01 ms per frame as single launches, see DESIGN.md 4.6 for the ring).  Camera, sun_position, sample_base,
 * base_frame and the buffers may differ from frame to frame; width, height, spp, max_bounces, flags and the shard must be the
 * same (BM_EINVAL otherwise).  Frames of a launch OVERLAP in time: ordered frames (BM_FLAG_ORDERED, hit records, primary-only)
 * write pixels back with plain stores and need accumulation buffers of their own; production frames add with float atomics
 * and may share one buffer, like consecutive frames of the reference's accumulation.  debug_dev: NULL, or `count` entries, each
 * NULL or a hit-record buffer of its own (BM_FLAG_RAY_DIGEST frames of one view whose sample_base steps by a constant and that share
 * their accumulation buffer may also share ONE hit-record buffer: it then holds the digest of the whole launch, samples counted from
 * the first frame's sample_base -- for sample_base stepping by spp, the digest of one frame of count x spp samples).  Results of ordered
 * frames are bit-identical to `count` single launches.  Production frames of one view whose sample_base and buffers step by
 * constants (a resting camera accumulating) are handed out in GROUPS of bm_frame_plan.ring_group consecutive frames, whose lanes
 * share a wave: such frames complete group by group rather than one after the other, and no frame of a group is complete before the
 * launch is -- as with every launch, read results only after the launch has finished.  Ray-digest frames that share one hit-record
 * buffer must keep count x spp x (max_bounces + 1) < 65536 and sample_base stride x (count - 1) + spp < 2^24 (BM_EINVAL otherwise).  Bricks
 * requested by any frame of the launch are serviced by the next bm_scene_process_load_queue.  bm_render_times /
 * bm_last_render_ms report the launch as one duration. */
BM_API int bm_render_frames(bm_scene* scene, int count, const bm_camera* cameras, const bm_frame_params* params,
                            float* const* accum_dev, uint32_t* const* debug_dev, void* hip_stream);

/* What the library decides for a frame with these parameters (host only, no device needed): the flags after its own choice of
 * work items, whether the frame is ordered, runs helper lanes, takes the XCD-aware hand-out, and when its waves refill.
 * hit_records: the frame will be given a debug_dev buffer. */
typedef struct bm_frame_plan {
	uint32_t flags;        /* params->flags, plus BM_FLAG_SAMPLE_ITEMS where the library schedules (chunk, sample) items by itself */
	int32_t ordered;       /* 1: one lane accumulates a pixel's events in path order (reproducible sums)                          */
	int32_t helpers;       /* 1: shadow rays on helper lanes, float-atomic adds (csrc/trace.hip HELP)                             */
	int32_t sample_items;  /* 1: (4x4 chunk, sample) work items                                                                  */
	int32_t xcd_handout;   /* 1: 256x256-pixel super-tiles dealt to the eight XCDs' ticket counters (big frames)                 */
	int32_t refill_min;    /* a wave takes new work items once this many of its lanes are idle                                    */
	int32_t refill_min_in_ring; /* ... when the frame is one of several of a bm_render_frames launch (later: its end is covered)     */
	int32_t instrumented;  /* 1: the instrumented instantiation (hit records / BM_FLAG_COUNTERS) runs                             */
	int32_t tiles_x, tiles_y, local_rows;
	int32_t ring_group;    /* frames handed out together, as (chunk, pixel part, frame) items, when such frames make a uniform
	                          bm_render_frames launch (one view, sample_base and buffers stepping by constants); 1: frame after frame */
} bm_frame_plan;
BM_API int bm_frame_plan_of(const bm_frame_params* params, int hit_records, bm_frame_plan* out);
/* What the library decides for a bm_render_frames launch with these arguments (host only: no device, no scene; grid_size and
 * grid_height are the world's, as for bm_scene_create).  This is how a host learns the ring mode its launch gets -- which the
 * library decides from the frames' views and from the ADDRESSES of the buffers, never by reading them: accum_dev / debug_dev
 * are only compared and subtracted here.  Accepts and refuses exactly what bm_render_frames does on a scene of that world, with
 * the same error text; a refused plan leaves *out all zero. */
typedef struct bm_launch_plan {
	int32_t  ring_mode;       /* 0: one frame; 1: frame ring, waves change frame when idle; 2: uniform frame ring, frames share waves */
	int32_t  ring_group;      /* frames handed out together (1 unless ring_mode == 2)                                                 */
	int32_t  sample_stride;   /* ring_mode 2: sample_base step from frame to frame                                                    */
	uint32_t pixel_stride;    /* ring_mode 2: buffer step from frame to frame, in pixels                                              */
	int32_t  shared_digest;   /* 1: ray-digest frames that all write one hit-record buffer                                            */
	int32_t  instrumented;    /* 1: the instrumented instantiation (hit records / BM_FLAG_COUNTERS) runs                              */
	int32_t  counter_blocks;  /* ticket-counter blocks the launch zeroes: one per frame, or per group of frames when ring_mode == 2   */
	int32_t  refill_min;      /* a wave takes new work items once this many of its lanes are idle                                     */
	int64_t  workgroups;      /* before the cap by what the device keeps resident                                                     */
} bm_launch_plan;
BM_API int bm_launch_plan_of(int count, const bm_camera* cameras, const bm_frame_params* params, float* const* accum_dev,
                             uint32_t* const* debug_dev, int grid_size, int grid_height, bm_launch_plan* out);
/* resident waves per SIMD of the trace_paths instantiation <instrumented, xcd_handout, helpers> on `device` (what the register
 * budget allows: hipOccupancyMaxActiveBlocksPerMultiprocessor of the 256-thread workgroup = one wave per SIMD each) */
BM_API int bm_trace_waves_per_simd(int device, int instrumented, int xcd_handout, int helpers, int* waves);
/* The tuning overrides this process runs under, as "NAME=value NAME=value" ("" when none is set): BM_REFILL_MIN,
 * BM_XCD_HANDOUT, BM_HELPERS, BM_TRACE_BLOCKS_PER_CU, BM_RING_GROUP -- A/B knobs read from the environment once; a measurement should echo them. */
BM_API int bm_tuning_overrides(char* buf, size_t buflen);

/* blit_onto_framebuffer (kernel.cu:348-364) into an offscreen float4 buffer: rgb/a, a=1, gamma 1/2.2 */
BM_API int bm_resolve(bm_scene* scene, const float* accum_dev, float* out_dev, int64_t n_pixels, void* hip_stream);
/* cudaDeviceSynchronize of launch_kernels:431 */
BM_API int bm_synchronize(bm_scene* scene);
/* duration of the most recent bm_render_frame kernel, measured with hipEvents on its stream (blocks) */
BM_API int bm_last_render_ms(bm_scene* scene, float* ms);
/* durations (ms) of the most recent (up to 256) bm_render_frame kernels, oldest first; blocks until they finished */
BM_API int bm_render_times(bm_scene* scene, float* ms, int capacity, int* count);
BM_API int bm_counters_read(bm_scene* scene, bm_counters* out);
BM_API int bm_counters_reset(bm_scene* scene);
BM_API int bm_sched_stats_read(bm_scene* scene, bm_sched_stats* out);
/* profiling builds (-DBM_PHASE_TIMING) only, zeros otherwise.  out8 = shader-clock ticks, summed over waves, a shade pass spends
 * in: connect, shade (hit branch), the sky model, pixel hand-back + primary ray, ray set-up; then the candidate passes that
 * walked an 8^3 brick, the sum of their loop lengths (longest walk among the lanes of the pass) and the sum of all lanes' walk lengths */
BM_API int bm_sched_detail_read(bm_scene* scene, uint64_t* out8);

/* ---- multi-GPU: the frame's interleaved row bands, one rank per GPU, gathered to the root over RCCL / xGMI.
 * No counterpart in the reference (single GPU: src/main.cpp:89 computes `multi_gpu` and never uses it).  Every rank holds a full
 * scene replica and renders its shard (band_rows / shard_rank / shard_count of bm_frame_params) into a packed local buffer;
 * bm_gather_frame is the one exchange per frame: ncclGroupStart / the root's ncclRecv from every peer into one stacked buffer /
 * the peers' ncclSend / ncclGroupEnd, then one kernel on the root that puts row y where it belongs.  RCCL is bound at run time
 * (dlopen of librccl.so.1 on the first call): a process that already holds an RCCL (torch.distributed, a host linked against
 * /opt/rocm/lib/librccl.so) shares it.  Error codes: 20000 + ncclResult_t. */
typedef struct bm_comm bm_comm;
#define BM_COMM_ID_BYTES 128 /* sizeof(ncclUniqueId) */
/* ncclGetUniqueId: called by ONE rank; the 128 bytes reach the others by the host's own means (MPI_Bcast, a file, a socket) */
BM_API int bm_comm_unique_id(void* id128);
/* ncclCommInitRank on `device`: collective over all `world` ranks (one process or thread per GPU) */
BM_API int bm_comm_create(int device, int rank, int world, const void* id128, bm_comm** out);
BM_API void bm_comm_destroy(bm_comm* comm);
/* rank and size AS THE LIBRARY REPORTS THEM (ncclCommUserRank / ncclCommCount) -- "did RCCL see N ranks" -- or, for a transport
 * without those entry points, what the communicator was created with */
BM_API int bm_comm_info(bm_comm* comm, int* rank, int* world);
/* 1 if the RCCL library can be bound in this process (dlopen + the entry points), 0 if not; starts nothing, allocates nothing */
BM_API int bm_comm_available(void);
/* packed_dev: this rank's bm_local_rows x width float4 (what bm_render_frame accumulated for its shard); frame_dev: height x width
 * float4 on the root (ignored elsewhere).  Enqueued on hip_stream: ordered behind the frame that produced packed_dev; the host
 * does not wait.  The row-to-rank map is that of bm_frame_params: row y belongs to rank (y / band_rows) % world. */
BM_API int bm_gather_frame(bm_comm* comm, const float* packed_dev, float* frame_dev, int height, int width, int band_rows, int root,
                           void* hip_stream);
/* The same exchange for a batch of `count` (1 ... 256) frames -- what a rank rendered with ONE bm_render_frames launch into ONE
 * allocation: packed_dev = count x bm_local_rows x width float4 (frame 0's rows, then frame 1's, ...), frames_dev = count x height x
 * width float4 on the root.  One ncclSend per peer for the whole batch, one group, one assembly kernel. */
BM_API int bm_gather_frames(bm_comm* comm, const float* packed_dev, float* frames_dev, int count, int height, int width, int band_rows,
                            int root, void* hip_stream);
/* sample-sharded frames (every rank renders the whole frame with its own sample_base slice): ncclReduce(sum) to the root */
BM_API int bm_reduce_frame(bm_comm* comm, const float* in_dev, float* out_dev, int64_t n_floats, int root, void* hip_stream);
/* all ranks have reached this point (an all-reduce of one word, then the host waits for the stream) */
BM_API int bm_comm_barrier(bm_comm* comm, void* hip_stream);
/* start-up check of the transport: a grouped send / receive round the ring of ranks and an all-reduce, data verified */
BM_API int bm_comm_selftest(bm_comm* comm, void* hip_stream);
/* Streams that demonstrably run side by side.  HIP maps streams onto a few hardware queues and a queue runs its packets in order:
 * two streams that share a queue do not overlap, and an exchange that waits for its frame at the head of a queue holds up whatever
 * another stream queued behind it.  A host that pipelines frames over two streams with bm_gather_frame on a third (INTEGRATION.md 1a;
 * measured: 0.98 against 1.20 ms per 1/8-shard step) takes its streams from here: `count` (1 ... 4) non-blocking streams on `device`,
 * picked from a few more candidates by timing a short spin kernel on every combination.  The caller owns them
 * (bm_release_streams, or hipStreamDestroy on each). */
BM_API int bm_probe_streams(int device, int count, void** streams_out);
BM_API void bm_release_streams(int count, void** streams);
/* test door: the root's assembly kernel alone, on one GPU -- frame row y <- packed row of rank (y / band_rows) % world, taken from
 * own_packed_dev for rank `me` and from stacked_dev (world x max_rows x width float4, rank-major) for everybody else */
BM_API int bm_debug_assemble_frame(int device, const float* own_packed_dev, const float* stacked_dev, float* frame_dev, int height, int width,
                                   int band_rows, int world, int me, int max_rows, void* hip_stream);

/* ---- wavefront mode: launch_kernels exactly as the reference schedules it (kernel.cu:366-439) --
 * one call traces ONE segment of every path in flight: primary_rays tops the work queue up to `queue_size`
 * (ray_queue_buffer_size, variables.h:61), extend, shade (survivors -> next queue, shadow rays -> shadow queue),
 * connect; then the queues are swapped (main.cpp:146).  The reference's statics / __device__ globals (frame,
 * start_position, primary_ray_cnt; kernel.cu:106-119,369) live in the bm_wavefront object.  Of `params` the
 * fields width, height, max_bounces, sun_position and flags (BM_FLAG_COUNTERS) are used; the frame number is
 * the object's own counter (starts at 1).  Survivors and shadow rays are compacted in slot order, i.e. the
 * order a sequential run of the reference produces.  Single GPU: the queue schedule does not shard. */
typedef struct bm_wavefront bm_wavefront;
/* the scene must stay alive while frames are issued on the wavefront object (destroying either first is safe) */
BM_API int bm_wavefront_create(bm_scene* scene, uint32_t queue_size, bm_wavefront** out);
BM_API void bm_wavefront_destroy(bm_wavefront* wf);
/* the reset_buffer branch of launch_kernels (:397-403): drop the paths in flight; the caller zeroes accum_dev */
BM_API int bm_wavefront_reset(bm_wavefront* wf);
BM_API int bm_wavefront_frame(bm_wavefront* wf, const bm_camera* camera, const bm_frame_params* params, float* accum_dev,
                              void* hip_stream);
/* out6 = survivors and shadow rays of the last frame, start_position, frame (next), primary rays generated by the
 * last frame, primary_ray_cnt; blocks until the device is idle */
BM_API int bm_wavefront_stats(bm_wavefront* wf, uint32_t* out6);
/* copy queue records to the host: which = 0 the work queue (64-byte RayQueue records, variables.h:43-52; after a
 * frame its first `survivors` slots hold the paths that continue), 1 the shadow queue (40-byte ShadowQueue records,
 * variables.h:54-59; first `shadow` slots) */
BM_API int bm_wavefront_read_queue(bm_wavefront* wf, int which, uint32_t first, uint32_t count, void* host_out);
/* hipEvent durations (ms) of the last frame: total, primary_rays + globals, extend, shade, connect */
BM_API int bm_wavefront_times(bm_wavefront* wf, float* ms5);
/* traversal counters of the frames run with BM_FLAG_COUNTERS: which = 0 the extend kernel, 1 the connect kernel, 2 both */
BM_API int bm_wavefront_counters_read(bm_wavefront* wf, int which, bm_counters* out);
BM_API int bm_wavefront_counters_reset(bm_wavefront* wf);
/* wave-scheduler statistics of the BM_FLAG_COUNTERS frames for kernel `which` (0 extend, 1 connect): out6 = brick-grid
 * move rounds and the lanes active in them, candidate rounds and lanes, refills and rays handed out */
BM_API int bm_wavefront_sched_stats_read(bm_wavefront* wf, int which, uint64_t* out6);

/* ---- numeric-contract probes used by the parity tests (device side of detmath.h etc.) */
BM_API int bm_debug_sincos(int device, int n, const float* x_host, float* sin_host, float* cos_host);
BM_API int bm_debug_sky(int device, const float sun_position[2], int n, const float* viewdirs_host /*3n*/,
                        float* sun_host /*3n*/, float* sky_host /*3n*/, float* sunsky_host /*3n*/);

#ifdef __cplusplus
}
#endif
#endif /* BRICKMAP_H */
